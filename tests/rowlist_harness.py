"""What the GPU tests of the row-list family (ragged, labelled, masked, wide, labelled evaluation and its gradients) share: the
constants, the gates and the C-ABI calls on the guarded buffers of tests/guarded.py (a plain helper module, no fixtures, no
tests; tests/rowlist_cases.py builds the inputs).

Every call follows one protocol: inputs between NaN / sentinel guards, outputs poisoned, the workspace exactly as long as the
entry's size query says (a positive multiple of 256) between guard bands and filled with `pattern`; after the call the return
code is 0, the workspace guards are intact, no requested output keeps poison, every input guard is intact and the inputs
are unmodified.

The gate `check_rows` is the exact-fp32 row of dense_harness.TOL (loss 5e-6, dE 1e-5, dw 2e-5) through the formulas of
dense_harness.check_dense(..., strict=False), restated with nm = R because per is [R]:
    |loss - ref| <= 5e-6 |ref| + 3e-7 sum|per| + 1e-6 + 2e-7 R;    per: rtol 1e-4, atol 2e-5
    dE: rel-Frobenius <= 1e-5 (or max-abs <= 1e-8 for a vanishing gradient) and max-abs <= 4e-5 max(1, max|dE|)
    |dw - ref| <= 2e-5 |ref| + 1e-5 + 1e-7 R;    |db - ref| <= 1e-4 + 3e-7 R           (strict: without the R terms)
"""
import numpy as np
import torch

import ragged_ref as rr
from conftest import rel_fro
from guarded import Buf, IntBuf, Workspace, same_bits

DEV = "cuda:0"
LT, GT, WT = 5e-6, 1e-5, 2e-5        # dense_harness.TOL["generic"] == TOL["fused_f32"] == TOL["wave"]: exact fp32
W, BIAS = 10.0, -5.0
EPS, EPS_COS = rr.EPS, rr.EPS_COS
VARIANTS = ("softmax", "contrast")
VAR = {"softmax": 0, "contrast": 1}
KEYS = ("loss", "per", "dE", "dw", "db")


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def batch_of(o, i):
    return {k: v[i] for k, v in o.items()}


# ---- gates -------------------------------------------------------------------------------------------------------------------
def check_rows(o, ref, what, strict=False, factor=1.0, quiet=False):
    """The gate of the module docstring on ONE batch (o: outputs of that batch, forward-only ones have loss and per only).
    `factor` scales every bound (2 where two fp32 results are compared with each other)."""
    R = int(np.asarray(ref["per"]).size)
    per_ref = np.asarray(ref["per"], np.float64).reshape(-1)
    loss_ref = float(ref["loss"])
    floor = 3e-7 * np.abs(per_ref).sum()
    lerr, lbound = abs(float(o["loss"]) - loss_ref), factor * (LT * abs(loss_ref) + floor + 1e-6 + 2e-7 * R)
    perr = np.abs(np.asarray(o["per"], np.float64).reshape(-1) - per_ref)
    pbound = factor * (2e-5 + 20 * LT * np.abs(per_ref))
    line = f"{what}: loss {lerr:.3e} / {lbound:.3e}  per worst share {float((perr / pbound).max()):.3f}"
    if "dE" in o:
        dE_ref = np.asarray(ref["dE"], np.float64).reshape(np.asarray(o["dE"]).shape)
        scale = max(1.0, float(np.abs(dE_ref).max()))
        fro, mabs = rel_fro(o["dE"], dE_ref), float(np.abs(o["dE"] - dE_ref).max())
        rowfloor = 0.0 if strict else 1.0
        dw_ref, db_ref = float(ref["dw"]), float(ref["db"])
        werr, wbound = abs(float(o["dw"]) - dw_ref), factor * (WT * abs(dw_ref) + 1e-5 + 1e-7 * R * rowfloor)
        berr, bbound = abs(float(o["db"]) - db_ref), factor * (1e-4 + 3e-7 * R * rowfloor)
        line += (f"  dE fro {fro:.3e} / {factor * GT:.0e} max-abs {mabs:.3e} / {factor * 4 * GT * scale:.3e}"
                 f"  dw {werr:.3e} / {wbound:.3e}  db {berr:.3e} / {bbound:.3e}")
    if not quiet:
        print(line)
    assert lerr <= lbound, f"{what} loss {float(o['loss'])} vs {loss_ref}"
    assert np.all(perr <= pbound), f"{what} per"
    if "dE" in o:
        # (a gradient that vanishes -- one speaker: p_jj = 1 - O(eps) -- is held to an absolute bound instead)
        assert fro <= factor * GT or mabs <= factor * 1e-8, f"{what} dE rel-fro {fro}"
        assert mabs <= factor * 4 * GT * scale, f"{what} dE max-abs {mabs}"
        assert werr <= wbound, f"{what} dw {float(o['dw'])} vs {dw_ref}"
        assert berr <= bbound, f"{what} db {float(o['db'])} vs {db_ref}"


def is_zero(a, plus):
    a = np.atleast_1d(np.asarray(a))
    return not a.any() and not (plus and np.signbit(a).any())


def check_masked(o, ref, what, quiet=False, plus=True):
    """One batch against masked_ref: `active` exactly, the rows that do not count exactly 0, and check_rows.
    `plus`: the zeros are +0, as the kernel writes them (False where autograd has scaled them by a negative gradient)."""
    idx = ref["index"]
    if "active" in o:
        assert o["active"].tolist() == idx["active"].tolist(), f"{what}: active {o['active']} vs {idx['active']}"
    rest = ~idx["active_row"]
    for k in ("per", "dE"):
        if k in o:
            assert is_zero(o[k][rest], plus), f"{what}: {k} is not 0 on a row that does not count"
    if idx["active"][0] == 0:
        for k in KEYS:
            if k in o:
                assert is_zero(o[k], plus), f"{what}: {k} is not 0 though nothing counts"
        return
    check_rows({k: o[k] for k in KEYS if k in o}, ref, what, quiet=quiet)


def two_part(o, ref, deg, active_row, what, factor=1.0):
    """The gate where one speaker's gradients are 1e6 to 1e9 times the others':
      loss rtol 1e-5, and dE on the degenerate speaker's rows max-abs <= 1e-5 max|dE_ref| (the rule of g8_degenerate);
      every other speaker's rows at the ordinary row bound of check_rows, max-abs <= 4e-5 max(1, max|dE_ref| over
      THOSE rows), so that the large entries cannot hide them, and per there at check_rows' per bound: these rows get terms of
      ordinary size only."""
    rest = active_row & ~deg
    dref = np.asarray(ref["dE"], np.float64)
    top, plain = float(np.abs(dref).max()), max(1.0, float(np.abs(dref[rest]).max()))
    derr, rerr = float(np.abs(o["dE"][deg] - dref[deg]).max()), float(np.abs(o["dE"][rest] - dref[rest]).max())
    lerr, lref = abs(float(o["loss"]) - float(ref["loss"])), abs(float(ref["loss"]))
    per_ref = np.asarray(ref["per"], np.float64)[rest]
    pshare = float((np.abs(o["per"][rest] - per_ref) / (factor * (2e-5 + 20 * LT * np.abs(per_ref)))).max())
    print(f"{what}: loss {lerr:.3e} / {factor * 1e-5 * lref:.3e}  per worst share {pshare:.3f}"
          f"  dE degenerate rows max-abs {derr:.3e} / {factor * 1e-5 * top:.3e}  other rows max-abs {rerr:.3e} / {factor * 4 * GT * plain:.3e}")
    assert lerr <= factor * 1e-5 * lref, f"{what}: loss {float(o['loss'])} vs {float(ref['loss'])}"
    assert derr <= factor * 1e-5 * top, f"{what}: dE of the degenerate speaker's rows {derr} of {top}"
    assert rerr <= factor * 4 * GT * plain, f"{what}: dE of the other speakers' rows {rerr}"
    assert pshare <= 1.0, f"{what}: per of the other speakers' rows"


def poisoned(E, idx):
    """E with NaN and +-Inf, in turn, on every row that does not count."""
    bad = E.copy()
    rest = np.flatnonzero(~idx["active_row"])
    bad[rest] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(len(rest)) % 3][:, None]
    return bad


# ---- the loss calls ----------------------------------------------------------------------------------------------------------
ROW_ENTRIES = {
    # name: (entry, size query, `table` is offsets (B, N + 1) and not labels (B, R), an `active` argument, E holds only finite rows)
    "ragged": ("ge2e_loss_fwd_bwd_ragged", "ge2e_workspace_bytes_ragged", True, False, True),
    "labeled": ("ge2e_loss_fwd_bwd_labeled", "ge2e_workspace_bytes_labeled", False, False, True),
    "masked": ("ge2e_loss_fwd_bwd_labeled_masked", "ge2e_workspace_bytes_labeled_masked", False, True, False),
    "wide": ("ge2e_loss_fwd_bwd_labeled_wide", "ge2e_workspace_bytes_labeled_wide", False, True, False),
}


def call_rows_loss(lib, entry, E, table, N, variant, want_grad=True, pattern=0xFF, want_per=True, want_active=True, w=W, b=BIAS,
                   finite=True):
    """One call of a ROW_ENTRIES loss on guarded buffers, by the protocol of the module docstring.  E (B, R, D) float32, `table`
    int32: the offsets or the labels -> numpy outputs (`active` among them where the entry has it and `want_active`).
    `finite=False`: the outputs may hold NaN or Inf (the guards are checked all the same)."""
    symbol, size_query, is_offsets, has_active, finite_E = ROW_ENTRIES[entry]
    E = np.ascontiguousarray(E, dtype=np.float32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    B, R, D = E.shape
    tname = "offsets" if is_offsets else "labels"
    what = f"{entry} B{B} N{N} R{R} D{D} {variant} {'fwd+bwd' if want_grad else 'fwd'} fill {pattern:#04x}"
    e, tab, wb, bb = Buf(E.shape, E), IntBuf(table.shape, table), Buf((1,), [w]), Buf((1,), [b])
    outs = {"loss": Buf((B,))}
    if want_per:
        outs["per"] = Buf((B, R))
    if want_grad:
        outs.update(dE=Buf(E.shape), dw=Buf((B,)), db=Buf((B,)))
    act = IntBuf((B, 2)) if has_active and want_active else None
    nbytes = int(getattr(lib, size_query)(B, N, R, D, VAR[variant]))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    active_arg = (act.ptr if act else None,) if has_active else ()
    code = getattr(lib, symbol)(e.ptr, tab.ptr, B, N, R, D, wb.ptr, bb.ptr, EPS_COS, EPS, VAR[variant], ptr("loss"), ptr("per"),
                                ptr("dE"), ptr("dw"), ptr("db"), *active_arg, ws.ptr, nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {k: v.get(f"{what} {k}", finite=finite) for k, v in outs.items()}       # guards intact, no NaN poison left
    if act:
        res["active"] = act.get(what + " active")                                  # ... no sentinel poison left
    for k, v in (("E", e), (tname, tab), ("w", wb), ("b", bb)):
        assert v.guards_intact(), f"{what}: guard of {k} overwritten"
    assert same_bits(e.get(what + " E", finite=finite_E), E), f"{what}: E was modified"
    # (offsets never reach the sentinel; labels may hold any int32)
    assert np.array_equal(tab.get(f"{what} {tname}", written=is_offsets), table), f"{what}: the {tname} were modified"
    return res


def run_ragged(lib, E, offsets, variant, want_grad=True, pattern=0xFF, w=W, b=BIAS, finite=True):
    """One ge2e_loss_fwd_bwd_ragged call.  E (B, R, D) float32, offsets (B, N+1) int32 -> numpy outputs."""
    return call_rows_loss(lib, "ragged", E, offsets, np.shape(offsets)[1] - 1, variant, want_grad, pattern, w=w, b=b, finite=finite)


def run_labeled(lib, E, labels, N, variant, want_grad=True, pattern=0xFF, w=W, b=BIAS, finite=True):
    """One ge2e_loss_fwd_bwd_labeled call.  E (B, R, D) float32, labels (B, R) int32 -> numpy outputs."""
    return call_rows_loss(lib, "labeled", E, labels, N, variant, want_grad, pattern, w=w, b=b, finite=finite)


def run_masked(lib, E, labels, N, variant, want_grad=True, pattern=0xFF, want_per=True, want_active=True, w=W, b=BIAS):
    """One ge2e_loss_fwd_bwd_labeled_masked call.  E (B, R, D) float32 (rows that do not count may hold NaN), labels (B, R)
    int32 -> numpy outputs, `active` among them."""
    return call_rows_loss(lib, "masked", E, labels, N, variant, want_grad, pattern, want_per, want_active, w, b)


def run_wide(lib, E, labels, N, variant, want_grad=True, pattern=0xFF, want_per=True, want_active=True, w=W, b=BIAS):
    """One ge2e_loss_fwd_bwd_labeled_wide call.  E (B, R, D) float32 (rows that do not count may hold NaN or Inf), labels
    (B, R) int32 -> numpy outputs, `active` among them."""
    return call_rows_loss(lib, "wide", E, labels, N, variant, want_grad, pattern, want_per, want_active, w, b)


def ragged_on_compacted(lib, E, ref, variant, w=W, b=BIAS):
    """ge2e_loss_fwd_bwd_ragged on the rows that count, per and dE scattered back (zeros elsewhere): what the masked call
    must return bit for bit."""
    idx = ref["index"]
    n_act, r_act = (int(v) for v in idx["active"])
    rows = idx["order"][:r_act]
    want = run_ragged(lib, np.ascontiguousarray(E[rows])[None], idx["offsets"][:n_act + 1][None], variant, True, 0xFF, w=w, b=b)
    out = {k: want[k] for k in ("loss", "dw", "db")}
    for k in ("per", "dE"):
        back = np.zeros((1,) + E.shape[:1] + want[k].shape[2:], dtype=np.float32)
        back[0, rows] = want[k][0]
        out[k] = back
    return out


# ---- the index calls ---------------------------------------------------------------------------------------------------------
def run_index(lib, labels, N, pattern=0xFF, masked=False):
    """One ge2e_label_index (`masked`: ge2e_label_index_masked) call on guarded buffers: labels (B, R) int32 ->
    (offsets (B, N+1), order (B, R)); masked: a dict of offsets, order, speakers (B, N), active (B, 2)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    B, R = labels.shape
    symbol = "ge2e_label_index_masked" if masked else "ge2e_label_index"
    what = f"{symbol[5:]} B{B} N{N} R{R} fill {pattern:#04x}"
    lab = IntBuf(labels.shape, labels)
    outs = {"offsets": IntBuf((B, N + 1)), "order": IntBuf((B, R))}
    if masked:
        outs.update(speakers=IntBuf((B, N)), active=IntBuf((B, 2)))
    nbytes = int(getattr(lib, symbol + "_workspace_bytes")(B, N, R))
    assert nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    code = getattr(lib, symbol)(lab.ptr, B, N, R, *(v.ptr for v in outs.values()), ws.ptr if nbytes else None, nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {k: v.get(f"{what} {k}") for k, v in outs.items()}                  # guards intact, no sentinel poison left
    assert lab.guards_intact() and np.array_equal(lab.get(what + " labels", written=False), labels), f"{what}: labels modified"
    return res if masked else (res["offsets"], res["order"])


# ---- the evaluation and gradient calls ---------------------------------------------------------------------------------------
def run_cos(lib, E, labels, N, thr=None, want_cos=True, pattern=0xFF, want_index=True):
    """One ge2e_cos_sim_labeled call on guarded buffers.  E (B, R, D) float32 (rows that do not count may hold NaN), labels
    (B, R) int32 -> dict of numpy outputs."""
    E = np.ascontiguousarray(E, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    B, R, D = E.shape
    T = 0 if thr is None else len(thr)
    what = f"cos_sim_labeled B{B} N{N} R{R} D{D} T{T} {'cos' if want_cos else 'no cos'} fill {pattern:#04x}"
    e, lab = Buf(E.shape, E), IntBuf(labels.shape, labels)
    th = Buf((T,), np.asarray(thr, dtype=np.float64).astype(np.float32)) if T else None
    fouts, iouts = {}, {}
    if want_cos:
        fouts["cos"] = Buf((B, R, N))
    if want_index:
        iouts.update(col=IntBuf((B, R)), speakers=IntBuf((B, N)), active=IntBuf((B, 2)))
    if T:
        iouts["counts"] = IntBuf((B, T, 2))
    nbytes = int(lib.ge2e_cos_sim_labeled_workspace_bytes(B, N, R, D))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    ptr = lambda d, k: d[k].ptr if k in d else None  # noqa: E731
    code = lib.ge2e_cos_sim_labeled(e.ptr, lab.ptr, B, N, R, D, EPS_COS, EPS, th.ptr if T else None, T, ptr(fouts, "cos"),
                                    ptr(iouts, "col"), ptr(iouts, "speakers"), ptr(iouts, "active"), ptr(iouts, "counts"),
                                    ws.ptr, nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {k: v.get(f"{what} {k}") for k, v in fouts.items()}       # guards intact, every element written and finite
    res.update({k: v.get(f"{what} {k}") for k, v in iouts.items()})  # ... no sentinel poison left
    assert e.guards_intact() and lab.guards_intact() and (th is None or th.guards_intact()), f"{what}: an input's guard"
    assert same_bits(e.get(what + " E", finite=False), E), f"{what}: E was modified"
    assert np.array_equal(lab.get(what + " labels", written=False), labels), f"{what}: the labels were modified"
    return res


def run_counts(lib, sim, col, active, thr):
    """One ge2e_eer_counts_labeled call on guarded buffers: sim (B, R, N) float32 of any content -> counts (B, T, 2)."""
    sim = np.ascontiguousarray(sim, dtype=np.float32)
    B, R, N = sim.shape
    T = len(thr)
    what = f"eer_counts_labeled B{B} N{N} R{R} T{T}"
    s, c, a = Buf(sim.shape, sim), IntBuf((B, R), col), IntBuf((B, 2), active)
    th = Buf((T,), np.asarray(thr, dtype=np.float64).astype(np.float32))
    out = IntBuf((B, T, 2))
    code = lib.ge2e_eer_counts_labeled(s.ptr, c.ptr, a.ptr, B, N, R, th.ptr, T, out.ptr, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    got = out.get(what + " counts")
    assert s.guards_intact() and c.guards_intact() and a.guards_intact() and th.guards_intact(), f"{what}: an input's guard"
    assert same_bits(s.get(what + " sim", finite=False), sim), f"{what}: sim was modified"
    return got


def run_bwd(lib, E, labels, N, g_cos, pattern=0xFF, want_active=True, g_offset=0):
    """One ge2e_cos_sim_labeled_bwd call on guarded buffers.  E (B, R, D) and g_cos (B, R, N) float32 (NaN where they must not be
    read), labels (B, R) int32 -> {"dE", "active"}.  `g_offset`: g_cos starts that many floats past a 16-byte boundary."""
    E = np.ascontiguousarray(E, dtype=np.float32)
    g_cos = np.ascontiguousarray(g_cos, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    B, R, D = E.shape
    what = f"cos_sim_labeled_bwd B{B} N{N} R{R} D{D} fill {pattern:#04x} g_cos+{g_offset}"
    e, lab, g = Buf(E.shape, E), IntBuf(labels.shape, labels), Buf(g_cos.shape, g_cos, offset=g_offset)
    dE = Buf(E.shape)
    act = IntBuf((B, 2)) if want_active else None
    nbytes = int(lib.ge2e_cos_sim_labeled_bwd_workspace_bytes(B, N, R, D))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    code = lib.ge2e_cos_sim_labeled_bwd(e.ptr, lab.ptr, g.ptr, B, N, R, D, EPS_COS, dE.ptr, act.ptr if act else None, ws.ptr,
                                        nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {"dE": dE.get(what + " dE")}                      # guards intact, every element written and finite
    if act:
        res["active"] = act.get(what + " active")
    assert e.guards_intact() and lab.guards_intact() and g.guards_intact(), f"{what}: an input's guard"
    assert same_bits(e.get(what + " E", finite=False), E), f"{what}: E was modified"
    assert same_bits(g.get(what + " g_cos", finite=False), g_cos), f"{what}: g_cos was modified"
    assert np.array_equal(lab.get(what + " labels", written=False), labels), f"{what}: the labels were modified"
    return res


def run_calc(lib, sim, col, active, eps, variant, gl=None, gp=None, want_loss=True):
    """ge2e_calc_loss_labeled and ge2e_calc_loss_labeled_bwd on guarded buffers: sim (B, R, N) -> loss (B,), per (B, R), dS."""
    sim = np.ascontiguousarray(sim, dtype=np.float32)
    B, R, N = sim.shape
    what = f"calc_loss_labeled B{B} N{N} R{R} {variant} eps {eps}"
    s, c, a = Buf(sim.shape, sim), IntBuf((B, R), col), IntBuf((B, 2), active)
    loss, per, dS = Buf((B,)), Buf((B, R)), Buf(sim.shape)
    bl = Buf((B,), gl) if gl is not None else None
    bp = Buf((B, R), gp) if gp is not None else None
    code = lib.ge2e_calc_loss_labeled(s.ptr, c.ptr, a.ptr, B, N, R, eps, VAR[variant], loss.ptr if want_loss else None,
                                      per.ptr, None)
    assert code == 0, f"{what} returned {code}"
    code = lib.ge2e_calc_loss_labeled_bwd(s.ptr, c.ptr, a.ptr, B, N, R, eps, VAR[variant], bl.ptr if bl else None,
                                          bp.ptr if bp else None, dS.ptr, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} (backward) returned {code}"
    out = {"per": per.get(what + " per"), "dS": dS.get(what + " d_sim")}        # every element written and finite
    if want_loss:
        out["loss"] = loss.get(what + " loss")
    for v in (s, c, a, bl, bp):
        assert v is None or v.guards_intact(), f"{what}: an input's guard"
    assert same_bits(s.get(what + " sim", finite=False), sim), f"{what}: sim was modified"
    return out
