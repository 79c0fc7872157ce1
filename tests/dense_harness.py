"""What the tests of the dense (B, N, M, D) loss share: the tolerance table and its gate, the call through `functional` on
poisoned outputs, the call through the C ABI on the guarded buffers of tests/guarded.py, and the committed launch plans (a plain
helper module, no fixtures, no tests).

Tolerances (BASELINE.json north_star: loss rtol 1e-4; SURVEY 8d parity gate):
    loss  rtol 1e-4      (the exact-fp32 impls are held to 5e-6)
    dE    rel-Frobenius <= 1e-4 and max-abs <= 1e-4 * max|dE|   (exact-fp32: 5e-6)
    dw    rtol 1e-4 (+ tiny atol)   db  atol 1e-4 (cancellation residue, never rtol)
"""
import os

import numpy as np
import torch

import bounds_cases as bc
from capi import ok
from conftest import rel_fro
from guarded import Buf, Workspace, same_bits
from oracle import ge2e_oracle as orc

TOL = {  # impl -> (loss rtol, dE rel-fro / relative max-abs, dw rtol, cos atol)
    "generic": (5e-6, 1e-5, 2e-5, 2e-6),
    "fused_f32": (5e-6, 1e-5, 2e-5, 2e-6),
    "fused_split": (2e-5, 2e-5, 5e-5, 5e-6),
    "tiled": (2e-5, 2e-5, 5e-5, 5e-6),
    "team": (2e-5, 2e-5, 5e-5, 5e-6),
    "wave": (5e-6, 1e-5, 2e-5, 2e-6),
    "auto": (1e-4, 1e-4, 1e-4, 1e-5),
}
EPS_COS, EPS = orc.EPS_COS, orc.SMALL_ERR
FILLS = (0xFF, 0x00)
WORST = {}
PLANS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans.json")


# ---- through `functional` ----------------------------------------------------------------------------------------------------
def impls_for(GF, B, N, M, D, variant="softmax"):
    out = []
    for name in ("generic", "fused_f32", "fused_split", "tiled", "team", "wave"):
        try:
            GF.resolve_impl(B, N, M, D, variant, name)
            out.append(name)
        except RuntimeError:
            pass
    assert out, "no implementation accepts this shape"
    return out + ["auto"]


def run_hip(GF, E, w, b, variant="softmax", impl="auto", eps=1e-6):
    dev = torch.device("cuda:0")
    e = torch.as_tensor(E, device=dev)
    wt = torch.tensor(float(w), device=dev)
    bt = torch.tensor(float(b), device=dev)
    # poison every output first: a kernel that skips rows must not pass on stale allocator memory
    shp = tuple(e.shape) if e.dim() == 4 else (1,) + tuple(e.shape)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    out = GF.LossOutputs(loss=nan(shp[0]), per=nan(*shp[:3]), dE=nan(*shp), dw=nan(shp[0]), db=nan(shp[0]))
    o = GF.loss_fwd_bwd(e, wt, bt, variant=variant, impl=impl, eps=eps, out=out)
    torch.cuda.synchronize()
    squeeze = (lambda t: t[0]) if e.dim() == 3 else (lambda t: t)
    return {k: squeeze(getattr(o, k)).cpu().numpy() for k in ("loss", "per", "dE", "dw", "db")}


# ---- gates -------------------------------------------------------------------------------------------------------------------
def check_dense(o, ref, impl, what="", strict=False):
    """strict = the BASELINE configs and the reference's own fixtures: the stated gate with no per-row floors --
    db atol 1e-4 flat, dw rtol + 1e-5.  The floors that scale with the row count are for fuzz / ragged shapes only, where
    dw and db are sums of thousands of terms of both signs that cancel to ~0."""
    lt, gt, wt, _ = TOL[impl]
    loss_ref = np.asarray(ref["loss"], np.float64)
    # loss is a sum of NM terms of size ~|S|: fp32 noise floor scales with that, not with |loss|
    floor = 3e-7 * np.abs(np.asarray(ref["per"], np.float64)).sum(axis=(-1, -2))
    nm = int(np.prod(np.asarray(ref["per"]).shape[-2:]))   # rows per batch: an absolute fp32 floor per row (log(1 + tiny) at N = 1)
    assert np.all(np.abs(o["loss"] - loss_ref) <= lt * np.abs(loss_ref) + floor + 1e-6 + 2e-7 * nm), \
        f"{what} loss {o['loss']} vs {loss_ref}"
    assert np.allclose(o["per"], ref["per"], rtol=20 * lt, atol=2e-5), f"{what} per"
    scale = max(1.0, float(np.abs(ref["dE"]).max()))
    # (a gradient that vanishes -- one speaker: p_jj = 1 - O(eps) -- is held to an absolute bound instead)
    assert rel_fro(o["dE"], ref["dE"]) <= gt or np.abs(o["dE"] - ref["dE"]).max() <= 1e-8, \
        f"{what} dE rel-fro {rel_fro(o['dE'], ref['dE'])}"
    assert np.abs(o["dE"] - ref["dE"]).max() <= 4 * gt * scale, f"{what} dE max-abs"
    dw_ref = np.asarray(ref["dw"], np.float64)
    # dw = sum G (cos + eps) cancels when the rows' terms have both signs: an absolute floor per row beside the relative bound
    rowfloor = 0.0 if strict else 1.0
    assert np.all(np.abs(o["dw"] - dw_ref) <= wt * np.abs(dw_ref) + 1e-5 + 1e-7 * nm * rowfloor), f"{what} dw {o['dw']} vs {dw_ref}"
    # db cancels row by row: an fp32 floor per row -- for the non-BASELINE shapes only
    assert np.allclose(o["db"], ref["db"], rtol=0, atol=1e-4 + 3e-7 * nm * rowfloor), f"{what} db {o['db']} vs {ref['db']}"


def check_forward(o, ref, impl, what):
    """The loss and per lines of check_dense, with the same numbers (forward-only calls have nothing else)."""
    lt = TOL[impl][0]
    loss_ref = np.asarray(ref["loss"], np.float64)
    floor = 3e-7 * np.abs(np.asarray(ref["per"], np.float64)).sum(axis=(-1, -2))
    nm = int(np.prod(np.asarray(ref["per"]).shape[-2:]))
    assert np.all(np.abs(o["loss"] - loss_ref) <= lt * np.abs(loss_ref) + floor + 1e-6 + 2e-7 * nm), \
        f"{what} loss {o['loss']} vs {loss_ref}"
    if "per" in o:
        assert np.allclose(o["per"], ref["per"], rtol=20 * lt, atol=2e-5), f"{what} per"


def note(impl, **errs):
    """Keep and print the worst figure of every kind seen for `impl` so far."""
    w = WORST.setdefault(impl, {})
    for k, v in errs.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(f"[bounds worst] {impl:>12s} " + "  ".join(f"{k} {v:.3e}" for k, v in sorted(w.items())))


# ---- through the C ABI ---------------------------------------------------------------------------------------------------------
def ids():
    from speaker_embedding_ge2e_loss_amd import _lib
    return _lib.VARIANTS, _lib.IMPLS, _lib.IMPL_NAMES


def call_loss(lib, case, E, combo, pattern):
    """One ge2e_loss_fwd_bwd call on guarded buffers; returns the outputs that were asked for (numpy)."""
    VAR, IMPL, _ = ids()
    impl, B, N, M, D, variant = case
    name, want_per, want_grad, misaligned = combo
    what = f"{bc.case_id(case)}/{name}/fill {pattern:#04x}"
    off = 1 if misaligned else 0          # the header promises 16-byte alignment for E and dE only
    e, w, b = Buf(E.shape, E), Buf((1,), [bc.W]), Buf((1,), [bc.BIAS])
    outs = {"loss": Buf((B,), offset=off)}
    if want_per:
        outs["per"] = Buf((B, N, M), offset=off)
    if want_grad:
        outs.update(dE=Buf(E.shape), dw=Buf((B,), offset=off), db=Buf((B,), offset=off))
    if misaligned:
        assert all(outs[k].ptr % 16 == 4 for k in ("loss", "per", "dw", "db")) and outs["dE"].ptr % 16 == 0
    nbytes = int(lib.ge2e_workspace_bytes(B, N, M, D, VAR[variant], IMPL[impl]))     # for the REQUESTED impl, as a caller would
    ws = Workspace(nbytes, pattern)
    ok(lib.ge2e_workspace_init(ws.ptr, nbytes, None), what + " ge2e_workspace_init")
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    code = lib.ge2e_loss_fwd_bwd(e.ptr, B, N, M, D, w.ptr, b.ptr, EPS_COS, EPS, VAR[variant], IMPL[impl], ptr("loss"),
                                 ptr("per"), ptr("dE"), ptr("dw"), ptr("db"), ws.ptr, nbytes, None)
    torch.cuda.synchronize()
    ok(code, what + " ge2e_loss_fwd_bwd")
    ws.check(what)
    res = {k: v.get(f"{what} {k}") for k, v in outs.items()}        # guards intact, no NaN / inf left
    for k, v in (("E", e), ("w", w), ("b", b)):
        assert v.guards_intact(), f"{what}: guard of {k} overwritten"
    assert same_bits(e.get(what + " E"), E), f"{what}: E was modified"
    return res


# ---- the launch plans ----------------------------------------------------------------------------------------------------------
def current_plans(lib):
    plans = bc.table_plans(lib)
    return {what: ",".join(plan) for t in ("LOSS_CASES", "PLAN_CASES") for what, plan in plans[t]}
