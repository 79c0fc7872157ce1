"""GPU: every fp32 loss kernel between guard bands on a workspace of exactly the advertised size.

ge2e_loss_fwd_bwd, ge2e_cos_sim, ge2e_loss_fwd_bwd_raw, ge2e_normalize_unperm (+ _bwd), ge2e_eer_counts and
ge2e_sample_batch are called through _lib.load() with raw pointers into the guarded buffers of tests/guarded.py, so the
sizes the kernels see are exactly the ones include/ge2e_hip.h documents -- not what torch's allocator rounds them up to:

  - inputs sit between NaN (int32: sentinel) guards, outputs are NaN-poisoned between guards, the workspace is exactly
    ge2e_workspace_bytes long (that same number is passed as workspace_bytes), 256-byte aligned, between 256-byte guards;
  - every guard must come back bit for bit, no requested output may keep poison, E must be unchanged;
  - results pass the existing gate (check_dense / TOL of tests/dense_harness.py, non-strict, against the fp64 closed form);
  - every case runs on a workspace filled with 0xFF bytes (NaN as fp32 and as fp16 halves) and on one filled with 0x00,
    ge2e_workspace_init after each fill: the two runs must agree bit for bit on every output (test_gpu_determinism.py
    holds the kernels to bitwise repeatability, so a difference means workspace contents leak into a result).

The shapes (tests/bounds_cases.py, checked on the CPU by tests/test_bounds_cases.py) sit on each kernel's padding edges.

Limits of the method.  A read outside a buffer whose value is then masked or discarded does not show as a NaN, so it is
not seen here, and the tests do not try to make the hardware fault instead.  A store that lands inside the workspace but
in another batch's region is not seen by the guards either: wrong results from that are the parity tests' business.
bench.py, tests/conftest.py and the pytest settings are untouched; nothing reads the reference project.

Every test prints its worst errors per implementation (`-s`), next to the bound they are held to.
"""
import numpy as np
import pytest
import torch

import bounds_cases as bc
from capi import lib, ok  # noqa: F401
from conftest import rel_fro
from dense_harness import EPS, EPS_COS, FILLS, TOL, call_loss, check_dense, check_forward, ids, note
from guarded import SENTINEL, Buf, IntBuf, Workspace, same_bits
from oracle import ge2e_oracle as orc

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("case", bc.LOSS_CASES, ids=bc.case_id)
def test_loss_between_guards_on_an_exact_workspace(lib, case):
    VAR, IMPL, NAMES = ids()
    impl, B, N, M, D, variant = case
    ran = NAMES[lib.ge2e_resolve_impl(B, N, M, D, VAR[variant], IMPL[impl])]
    if impl not in bc.AUTO_REACHES:
        assert ran == impl, f"{case}: resolves to {ran}"
    E = bc.loss_inputs(case)
    ref = bc.loss_reference(case)
    for combo in bc.COMBOS:
        what = f"{bc.case_id(case)}/{combo[0]}"
        o, o0 = (call_loss(lib, case, E, combo, p) for p in FILLS)
        for k in o:
            assert same_bits(o[k], o0[k]), f"{what}: {k} depends on what the workspace held before the call"
        if "dE" in o:                      # per = NULL: its line of the gate has nothing to look at
            check_dense(o if "per" in o else dict(o, per=ref["per"]), ref, ran, what)
        else:
            check_forward(o, ref, ran, what)
        errs = {"loss": np.max(np.abs(o["loss"] - ref["loss"]) / np.maximum(np.abs(ref["loss"]), 1e-30))}
        if "per" in o:
            errs["per abs"] = np.abs(o["per"] - ref["per"]).max()
        if "dE" in o:
            errs.update({"dE fro": rel_fro(o["dE"], ref["dE"]),
                         "dw": np.max(np.abs(o["dw"] - ref["dw"]) / np.maximum(np.abs(ref["dw"]), 1e-30)),
                         "db abs": np.abs(o["db"] - ref["db"]).max()})
        print(f"{what} ({ran}): " + "  ".join(f"{k} {float(v):.3e}" for k, v in errs.items()))
        if not (N == 1 or np.abs(ref["dw"]).min() < 1e-3):      # (vanishing references: absolute floors of the gate apply)
            note(ran, **errs)
    print(f"TOL[{ran}] = {TOL[ran]} (loss rtol, dE rel-fro, dw rtol, cos atol); per atol 2e-5, db atol 1e-4 + 3e-7 N M")


# ---- ge2e_cos_sim ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.COS_CASES, ids=lambda c: "B{}_N{}_M{}_D{}".format(*c))
def test_cos_sim_between_guards_on_both_workspace_sizes(lib, case):
    """The workspace of ge2e_cos_sim_workspace_bytes (matrix cores where the shape allows) and the documented smaller one,
    ge2e_workspace_bytes(.., generic): where that is smaller than what the matrix-core route needs, the exact-fp32 VALU
    kernel has to run, so the result is held to the VALU tolerance."""
    _, IMPL, _ = ids()
    B, N, M, D = case
    E = orc.synth_embeddings(case, "raw", seed=sum(case))
    ref = orc.closed_form(E, want_grad=False)["cos"]
    big = int(lib.ge2e_cos_sim_workspace_bytes(B, N, M, D))
    small = int(lib.ge2e_workspace_bytes(B, N, M, D, 0, IMPL["generic"]))
    mfma_shape = N >= 16 and lib.ge2e_resolve_impl(B, N, M, D, 0, IMPL["tiled"]) == IMPL["tiled"]
    # Which kernel ran is not observable from the values (1e-6 passes either tolerance).  The evidence that the smaller
    # workspace takes the VALU kernel is the guard: it is too small for tiled_layout, so the matrix-core route on it would
    # write past its end.
    for nbytes in sorted({big, small}, reverse=True):
        route = "tiled" if (mfma_shape and nbytes == big) else "generic"
        got = []
        for pattern in FILLS:
            what = f"cos {case} ws {nbytes} fill {pattern:#04x}"
            e, cos, ws = Buf(E.shape, E), Buf((B, N, M, N)), Workspace(nbytes, pattern)
            ok(lib.ge2e_workspace_init(ws.ptr, nbytes, None), what)
            code = lib.ge2e_cos_sim(e.ptr, B, N, M, D, EPS_COS, EPS, cos.ptr, ws.ptr, nbytes, None)
            torch.cuda.synchronize()
            ok(code, what)
            ws.check(what)
            got.append(cos.get(what))
            assert e.guards_intact() and same_bits(e.get(what + " E"), E)
        assert same_bits(got[0], got[1]), f"cos {case} ws {nbytes}: depends on what the workspace held before the call"
        err = float(np.abs(got[0] - ref).max())
        print(f"cos {case} ws {nbytes} ({route}): max|diff| {err:.3e}  bound TOL[{route}][3] = {TOL[route][3]:.0e}")
        note("cos/" + route, cos=err)
        assert err <= TOL[route][3], f"cos {case} ws {nbytes}: {err:.3e}"


# ---- ge2e_loss_fwd_bwd_raw through the C ABI -----------------------------------------------------------------------------------
def call_raw(lib, case, Y, src, want_grad):
    VAR, _, _ = ids()
    B, N, M, D, variant = case
    what = f"raw {case} src={'perm' if src is not None else 'NULL'} {'fwd+bwd' if want_grad else 'fwd'}"
    y, w, b = Buf(Y.shape, Y), Buf((1,), [bc.W]), Buf((1,), [bc.BIAS])
    s = IntBuf(src.shape, src) if src is not None else None
    outs = {"loss": Buf((B,)), "per": Buf((B, N, M))}
    if want_grad:
        outs.update(dY=Buf(Y.shape), dw=Buf((B,)), db=Buf((B,)))
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    code = lib.ge2e_loss_fwd_bwd_raw(y.ptr, s.ptr if s else None, B, N, M, D, w.ptr, b.ptr, EPS_COS, EPS, VAR[variant],
                                     ptr("loss"), ptr("per"), ptr("dY"), ptr("dw"), ptr("db"), None)
    torch.cuda.synchronize()
    ok(code, what)
    res = {k: v.get(f"{what} {k}") for k, v in outs.items()}
    assert y.guards_intact() and w.guards_intact() and b.guards_intact() and same_bits(y.get(what + " Y"), Y), what
    if s is not None:
        assert np.array_equal(s.get(what + " src"), src), what
    return res, what


@pytest.mark.parametrize("case", bc.RAW_CASES, ids=bc.raw_id)
def test_raw_entry_batched_with_per_batch_src(lib, case):
    """ge2e_loss_fwd_bwd_raw with B > 1, a different permutation per batch, src = NULL, per_emb_loss requested, and forward
    only (dY = NULL), against fp64 numpy (bounds_cases.raw_reference).  Tolerances: those test_gpu_tail.py holds this
    path to (loss rtol 5e-6 + atol 2e-6, dY relative norm 2e-5, dw rtol 1e-4 + atol 1e-5, db atol 1e-4), per: TOL["wave"]."""
    c = bc.resolve_raw(lib, case)
    B, N, M, D, variant = c
    assert lib.ge2e_raw_supported(N, M, D) and (N == 1 or not lib.ge2e_raw_supported(N + 1, M, D) or case[1] != "max")
    Y, perm = bc.raw_inputs(c)
    for src in (perm, None):
        ref = bc.raw_reference(c, Y, src)
        full, what = call_raw(lib, c, Y, src, True)
        fwd, _ = call_raw(lib, c, Y, src, False)
        assert same_bits(full["loss"], fwd["loss"]) and same_bits(full["per"], fwd["per"]), f"{what}: forward-only differs"
        nref = np.linalg.norm(ref["dY"])
        errs = {"loss": np.max(np.abs(full["loss"] - ref["loss"]) / np.maximum(np.abs(ref["loss"]), 1e-30)),
                "per abs": np.abs(full["per"] - ref["per"]).max(),
                "dY norm": np.linalg.norm(full["dY"] - ref["dY"]) / max(nref, 1e-30),
                "dw": np.max(np.abs(full["dw"] - ref["dw"]) / np.maximum(np.abs(ref["dw"]), 1e-30)),
                "db abs": np.abs(full["db"] - ref["db"]).max()}
        print(f"{what}: " + "  ".join(f"{k} {float(v):.3e}" for k, v in errs.items()))
        if N > 1:                                                   # (N = 1: loss ~ eps, gradients ~ 0 -- the atol terms decide)
            note("raw", **errs)
        assert np.allclose(full["loss"], ref["loss"], rtol=5e-6, atol=2e-6), f"{what} loss"
        assert np.allclose(full["per"], ref["per"], rtol=20 * TOL["wave"][0], atol=2e-5), f"{what} per"
        assert np.linalg.norm(full["dY"] - ref["dY"]) <= 2e-5 * nref + 1e-9, f"{what} dY"
        assert np.allclose(full["dw"], ref["dw"], rtol=1e-4, atol=1e-5), f"{what} dw"
        assert np.allclose(full["db"], ref["db"], rtol=0, atol=1e-4), f"{what} db"
    print("bounds: loss rtol 5e-6 + 2e-6, per rtol 1e-4 + 2e-5, dY norm 2e-5, dw rtol 1e-4 + 1e-5, db atol 1e-4")


# ---- the callers either side of the loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(33, 7), (5, 1), (97, 129), (1, 3), (21, 1031), (7, 255)])
@pytest.mark.parametrize("identity", [False, True], ids=["perm", "identity"])
def test_normalize_unperm_between_guards(lib, rows, D, identity):
    """Odd rows and D.  fp64 numpy reference; the backward is fed the reference's e and rnorm rounded to fp32, so that it
    is tested on its own.  Tolerances: test_gpu_tail.py's (e rtol 2e-6 + 2e-7, dy rtol 2e-5 + 2e-6)."""
    rng = np.random.default_rng(rows * 1000 + D)
    y = (rng.standard_normal((rows, D)) * 3.0).astype(np.float32)
    g = rng.standard_normal((rows, D)).astype(np.float32)
    src = None if identity else rng.permutation(rows).astype(np.int32)
    idx = np.arange(rows) if identity else src
    y64 = y.astype(np.float64)
    rn_ref = 1.0 / np.linalg.norm(y64[idx], axis=1)
    e_ref = y64[idx] * rn_ref[:, None]
    yb, s = Buf(y.shape, y), (None if identity else IntBuf((rows,), src))
    e, rn = Buf((rows, D)), Buf((rows,))
    ok(lib.ge2e_normalize_unperm(yb.ptr, s.ptr if s else None, rows, D, e.ptr, rn.ptr, None), "ge2e_normalize_unperm")
    eo, rno = e.get("e"), rn.get("rnorm")
    assert yb.guards_intact() and same_bits(yb.get("y"), y) and (s is None or np.array_equal(s.get("src"), src))
    print(f"normalize_unperm {rows}x{D}: e max|diff| {np.abs(eo - e_ref).max():.3e}  rnorm rel {np.abs(rno / rn_ref - 1).max():.3e}")
    assert np.allclose(eo, e_ref, rtol=2e-6, atol=2e-7)
    assert np.allclose(rno, rn_ref, rtol=2e-6, atol=0)
    e32, rn32 = e_ref.astype(np.float32), rn_ref.astype(np.float32)
    e64, r64, g64 = e32.astype(np.float64), rn32.astype(np.float64), g.astype(np.float64)
    dy_ref = np.zeros((rows, D))
    dy_ref[idx] = (g64 - e64 * (e64 * g64).sum(axis=1, keepdims=True)) * r64[:, None]
    gb, eb, rb, dy = Buf(g.shape, g), Buf(e32.shape, e32), Buf((rows,), rn32), Buf((rows, D))
    ok(lib.ge2e_normalize_unperm_bwd(gb.ptr, eb.ptr, rb.ptr, s.ptr if s else None, rows, D, dy.ptr, None), "ge2e_normalize_unperm_bwd")
    dyo = dy.get("dy")
    assert gb.guards_intact() and eb.guards_intact() and rb.guards_intact() and (s is None or s.guards_intact())
    print(f"normalize_unperm_bwd {rows}x{D}: dy max|diff| {np.abs(dyo - dy_ref).max():.3e} max|ref| {np.abs(dy_ref).max():.3e}")
    assert np.allclose(dyo, dy_ref, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("B,N,M,T", [(2, 3, 5, 1), (1, 7, 3, 50), (3, 5, 2, 4096), (1, 1, 3, 50), (2, 9, 7, 50)])
def test_eer_counts_between_guards(lib, B, N, M, T):
    """Exact integer counts of the reference's fp32 `S > thres` (numpy in fp32); N M N is no multiple of 64; counts and all
    guards hold an int32 sentinel."""
    assert (N * M * N) % 64 != 0
    rng = np.random.default_rng(B * 100 + N * 10 + M + T)
    sim = rng.uniform(0.3, 1.1, size=(B, N, M, N)).astype(np.float32)
    thr = np.float32(0.5) + np.float32(0.01) * np.arange(T, dtype=np.float32) * np.float32(50.0 / T)
    thr = np.sort(thr.astype(np.float32))
    sim[0, 0, 0, 0] = thr[T // 2]                       # an exact tie: `>` is strict
    own = np.zeros((N, M, N), bool)
    own[np.arange(N), :, np.arange(N)] = True
    gt = sim[:, None] > thr[None, :, None, None, None]                       # (B,T,N,M,N), fp32 comparison
    ref = np.stack([(gt & ~own).sum(axis=(2, 3, 4)), (gt & own).sum(axis=(2, 3, 4))], axis=-1).astype(np.int32)
    s, t, counts = Buf(sim.shape, sim), Buf((T,), thr), IntBuf((B, T, 2))
    ok(lib.ge2e_eer_counts(s.ptr, B, N, M, t.ptr, T, counts.ptr, None), "ge2e_eer_counts")
    got = counts.get("counts")
    assert s.guards_intact() and t.guards_intact()
    print(f"eer_counts B{B} N{N} M{M} T{T}: {int((got != ref).sum())} of {ref.size} counts differ")
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("N,M,T,L,F", [(3, 3, 20, 20, 5), (3, 5, 30, 7, 40), (1, 1, 9, 9, 1), (5, 3, 17, 16, 33)])
def test_sample_batch_between_guards(lib, f64, N, M, T, L, F):
    """L = T and clip_start = T - L; the last speaker draws its last utterance, so the final element of `store` is read
    with a NaN guard right behind it; N M is odd.  The result is a cast: compared exactly."""
    assert (N * M) % 2 == 1
    rng = np.random.default_rng(N * 1000 + M * 100 + T + L + F)
    U = [2 + (j % 3) for j in range(N)]
    offs = np.concatenate([[0], np.cumsum([u * T * F for u in U])]).astype(np.int64)
    store = rng.standard_normal(int(offs[-1])) * (1.0 + 1e-9 * rng.standard_normal(int(offs[-1])))
    store = store.astype(np.float64 if f64 else np.float32)
    utt = np.stack([rng.integers(0, U[j], size=M) for j in range(N)]).astype(np.int32)
    utt[N - 1, M - 1] = U[N - 1] - 1
    clip = np.full((N,), T - L, np.int32)
    ref = np.empty((N, M, L, F), np.float32)
    for j in range(N):
        arr = store[offs[j]:offs[j + 1]].reshape(U[j], T, F)
        for i in range(M):
            ref[j, i] = arr[utt[j, i], clip[j]:clip[j] + L].astype(np.float32)
    st = Buf(store.shape, store, dtype=torch.float64 if f64 else torch.float32)
    so, ut, cl = IntBuf((N,), offs[:-1], dtype=torch.int64), IntBuf(utt.shape, utt), IntBuf(clip.shape, clip)
    out = Buf((N, M, L, F))
    ok(lib.ge2e_sample_batch(st.ptr, int(f64), so.ptr, ut.ptr, cl.ptr, N, M, T, L, F, out.ptr, None), "ge2e_sample_batch")
    got = out.get("out")
    assert st.guards_intact() and so.guards_intact() and ut.guards_intact() and cl.guards_intact()
    assert SENTINEL not in utt and SENTINEL not in offs
    print(f"sample_batch N{N} M{M} T{T} L{L} F{F} {'f64' if f64 else 'f32'}: {int((got != ref).sum())} of {ref.size} differ")
    assert np.array_equal(got, ref)
