"""GPU: every helper entry point of the C ABI ON ITS OWN against the fp64 reference of tests/helpers_ref.py.

ge2e_cos_sim_centroids / _rows (+ _bwd), ge2e_calc_loss / _rows (+ _bwd), ge2e_centroids (+ _bwd), ge2e_utterance_centroids
and ge2e_scale_grads are called through _lib.load() with data_ptr()s, so B > 1 reaches the *_rows entry points.  Inputs --
the saved `cos` and the incoming gradients included -- are the test's own data (the saved cos is the REFERENCE's, rounded to
fp32), so no stage can mask another.  Every output and the cos_sim_bwd workspace (at exactly *_workspace_bytes) is
NaN-filled and sits between NaN guard bands that must stay NaN; inputs sit between NaN guards too, so a read outside them
shows as a NaN in a result.

Tolerances are the project's for exact-fp32 VALU paths (test_gpu_parity.py): cos atol 3e-6, helper gradients rel-Frobenius
< 1e-5, per rtol 2e-4 atol 2e-5, loss rtol 2e-5 + (3e-7 sum|per| + 2e-7 rows), degenerate 1e8-scale gradients
1e-5 max|ref|.  Where a result vanishes by cancellation the bound is stated beside the case, from the reference's own
fp32 error or from the format's precision, never from a kernel's output.
"""
import numpy as np
import pytest
import torch

import helpers_ref as hr
from capi import functional as GF  # noqa: F401
from capi import ok
from conftest import rel_fro
from guarded import Buf, dev

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24  # fp32 unit round-off


@pytest.fixture(scope="module")
def lib(GF):
    from speaker_embedding_ge2e_loss_amd import _lib
    return _lib.load()


def grad_close(got, ref, what, floor=0.0, tol=1e-5):
    """helper gradients: rel-Frobenius < 1e-5; `floor` = an absolute bound for gradients that vanish by cancellation."""
    rf, mx = rel_fro(got, ref), float(np.abs(np.asarray(got, np.float64) - ref).max())
    print(f"{what}: rel_fro {rf:.3e} max|diff| {mx:.3e} max|ref| {np.abs(ref).max():.3e} floor {floor:.3e}")
    assert rf < tol or mx <= floor, f"{what}: rel_fro {rf:.3e}, max|diff| {mx:.3e} (floor {floor:.3e})"


# ---- get_cos_sim with the caller's centroids -------------------------------------------------------------------------------
def hip_cos_fwd(lib, E, C, N, j0, whole_entry, eps=hr.SMALL_ERR, eps_cos=hr.EPS_COS):
    B, n, M, D = E.shape
    e, c, cos = Buf(E.shape, E), Buf(C.shape, C), Buf((B, n, M, N))
    if whole_entry:
        ok(lib.ge2e_cos_sim_centroids(e.ptr, c.ptr, B, N, M, D, eps_cos, eps, cos.ptr, None), "ge2e_cos_sim_centroids")
    else:
        ok(lib.ge2e_cos_sim_rows(e.ptr, c.ptr, B, n, N, j0, M, D, eps_cos, eps, cos.ptr, None), "ge2e_cos_sim_rows")
    out = cos.get("cos")
    assert e.guards_intact() and c.guards_intact()
    return out


def hip_cos_bwd(lib, E, C, cos_saved, g, N, j0, whole_entry, eps=hr.SMALL_ERR, eps_cos=hr.EPS_COS):
    B, n, M, D = E.shape
    e, c, cs, gg = Buf(E.shape, E), Buf(C.shape, C), Buf(cos_saved.shape, cos_saved), Buf(g.shape, g)
    dE, dC = Buf(E.shape), Buf(C.shape)
    if whole_entry:
        nbytes = int(lib.ge2e_cos_sim_bwd_workspace_bytes(B, N, M, D))
    else:
        nbytes = int(lib.ge2e_cos_sim_rows_bwd_workspace_bytes(B, n, N, M, D))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Buf((nbytes // 4,))
    if whole_entry:
        ok(lib.ge2e_cos_sim_bwd(e.ptr, c.ptr, cs.ptr, gg.ptr, B, N, M, D, eps_cos, eps, dE.ptr, dC.ptr, ws.ptr, nbytes, None),
           "ge2e_cos_sim_bwd")
    else:
        ok(lib.ge2e_cos_sim_rows_bwd(e.ptr, c.ptr, cs.ptr, gg.ptr, B, n, N, j0, M, D, eps_cos, eps, dE.ptr, dC.ptr, ws.ptr,
                                     nbytes, None), "ge2e_cos_sim_rows_bwd")
    oE, oC = dE.get("dE"), dC.get("dC")
    ws.get("workspace", finite=False)
    for b in (e, c, cs, gg):
        assert b.guards_intact()
    return oE, oC


def cancel_floors(E, C, g, j0):
    """Absolute floors for D = 1, where every unit vector is +-1 and both gradients are EXACTLY zero (g - (g . x^) x^ = 0):
    the kernel subtracts two fp32 numbers of the size of the uncancelled term, each a sum of up to N (or n M) rounded
    products, so what is left is a few ulp of  sum |g| / |x|.  4 ulp of that sum; 0 (no floor) for D > 1."""
    if E.shape[-1] != 1:
        return 0.0, 0.0
    ne = np.maximum(np.abs(E.astype(np.float64))[..., 0], hr.EPS_COS)                       # (B,n,M)
    M = E.shape[2]
    loo = np.maximum(np.abs((E.sum(axis=2, keepdims=True) - E).astype(np.float64))[..., 0] / (M - 1), hr.EPS_COS)
    own = np.abs(g[:, np.arange(E.shape[1]), :, j0 + np.arange(E.shape[1])]).transpose(1, 0, 2)  # (B,n,M): |g| on the own column
    fe = float((np.abs(g).sum(axis=-1) / ne).max() + (own / loo).sum(axis=-1).max())
    nc = np.maximum(np.abs(C.astype(np.float64))[..., 0], hr.EPS_COS)                       # (B,N)
    fc = float((np.abs(g).sum(axis=(1, 2)) / nc).max())
    return 4 * ULP * fe, 4 * ULP * fc


@pytest.mark.parametrize("case", hr.COS_CASES, ids=lambda c: "B{}_N{}_M{}_D{}_n{}_j{}".format(*c))
def test_cos_sim_forward_and_backward(lib, case):
    B, N, M, D, n, j0 = case
    E, C, g = hr.cos_inputs(case)
    ref = hr.cos_rows_np(E, C, j0, g)
    saved = ref["cos"].astype(np.float32)
    fe, fc = cancel_floors(E, C, g, j0)
    for whole_entry in ((True, False) if (n == N and j0 == 0) else (False,)):
        tag = f"{case} {'whole' if whole_entry else 'rows'}"
        cos = hip_cos_fwd(lib, E, C, N, j0, whole_entry)
        print(f"{tag}: cos max|diff| {np.abs(cos - ref['cos']).max():.3e}")
        assert np.abs(cos - ref["cos"]).max() <= 3e-6, tag
        dE, dC = hip_cos_bwd(lib, E, C, saved, g, N, j0, whole_entry)
        grad_close(dE, ref["dE"], tag + " dE", fe)
        grad_close(dC, ref["dC"], tag + " dC", fc)
        if n < N:       # a slice's dC is PARTIAL: nothing from rows outside it, and exactly nothing on its own columns when n = 1
            if n == 1:
                assert np.all(dC[:, j0] == 0) and np.all(ref["dC"][:, j0] == 0), tag


@pytest.mark.parametrize("shape,cuts", [((1, 65, 2, 33), (0, 1, 64, 65)), ((3, 130, 2, 20), (0, 50, 90, 129, 130)), ((1, 7, 17, 65), (0, 3, 4, 7))],
                         ids=["N65", "N130", "N7"])
def test_shards_partial_dC_sums_to_the_whole_batch_dC(lib, shape, cuts):
    B, N, M, D = shape
    E, C, g = hr.cos_inputs((B, N, M, D, N, 0), seed=1)
    ref = hr.cos_rows_np(E, C, 0, g)
    saved = ref["cos"].astype(np.float32)
    tot = np.zeros((B, N, D), np.float64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        dE, dC = hip_cos_bwd(lib, E[:, a:b], C, saved[:, a:b], g[:, a:b], N, a, False)
        grad_close(dE, ref["dE"][:, a:b], f"{shape} shard {a}:{b} dE")
        part = hr.cos_rows_np(E[:, a:b], C, a, g[:, a:b])["dC"]
        grad_close(dC, part, f"{shape} shard {a}:{b} partial dC")
        tot += dC
    grad_close(tot, ref["dC"], f"{shape} summed dC")
    _, whole = hip_cos_bwd(lib, E, C, saved, g, N, 0, True)
    grad_close(tot, whole.astype(np.float64), f"{shape} summed dC vs ge2e_cos_sim_bwd")


@pytest.mark.parametrize("kind", hr.DEGENERATE)
def test_degenerate_vectors_follow_aten(lib, kind):
    """Zero and sub-eps_cos vectors, identical rows, an exactly-zero leave-one-out centroid: forward and backward against
    ATen's cosine_similarity in fp64 (gradients reach 1e8: compared relative to the largest entry, as the g8 fixture is)."""
    E, C, g = hr.degenerate_inputs(kind)
    _, N, M, D = E.shape
    ref = hr.cos_rows_np(E, C, 0, g)
    saved = ref["cos"].astype(np.float32)
    for whole_entry in (True, False):
        cos = hip_cos_fwd(lib, E, C, N, 0, whole_entry)
        assert np.abs(cos - ref["cos"]).max() <= 3e-6, kind
        dE, dC = hip_cos_bwd(lib, E, C, saved, g, N, 0, whole_entry)
        for got, want, what in ((dE, ref["dE"], "dE"), (dC, ref["dC"], "dC")):
            err, top = np.abs(got - want).max(), np.abs(want).max()
            print(f"{kind} {what}: max|diff| {err:.3e} max|ref| {top:.3e}")
            assert err <= 1e-5 * top, f"{kind} {what}: {err:.3e} vs max|ref| {top:.3e}"
    # a middle slice that holds the degenerate speaker
    j0 = {"zero_row": 1, "zero_centroid": 1, "tiny_row": 0, "tiny_centroid": 0, "identical_rows": 1, "loo_zero": 2}[kind]
    part = hr.cos_rows_np(E[:, j0:j0 + 1], C, j0, g[:, j0:j0 + 1])
    cos = hip_cos_fwd(lib, E[:, j0:j0 + 1], C, N, j0, False)
    assert np.abs(cos - part["cos"]).max() <= 3e-6, kind
    dE, dC = hip_cos_bwd(lib, E[:, j0:j0 + 1], C, part["cos"].astype(np.float32), g[:, j0:j0 + 1], N, j0, False)
    assert np.abs(dE - part["dE"]).max() <= 1e-5 * np.abs(part["dE"]).max(), kind
    assert np.abs(dC - part["dC"]).max() <= 1e-5 * np.abs(part["dC"]).max(), kind


# ---- calc_loss ---------------------------------------------------------------------------------------------------------------
def hip_calc_loss(lib, S, N, j0, eps, variant, whole_entry, want_per=True):
    from speaker_embedding_ge2e_loss_amd import _lib
    B, n, M, _ = S.shape
    s, loss, per = Buf(S.shape, S), Buf((B,)), Buf((B, n, M))
    v = _lib.VARIANTS[variant]
    if whole_entry:
        ok(lib.ge2e_calc_loss(s.ptr, B, N, M, eps, v, loss.ptr, per.ptr if want_per else None, None), "ge2e_calc_loss")
    else:
        ok(lib.ge2e_calc_loss_rows(s.ptr, B, n, N, j0, M, eps, v, loss.ptr, per.ptr if want_per else None, None), "ge2e_calc_loss_rows")
    out = loss.get("loss"), (per.get("per") if want_per else None)
    assert s.guards_intact() and per.guards_intact()
    return out


def hip_calc_loss_bwd(lib, S, N, j0, eps, variant, gl, gp, whole_entry):
    from speaker_embedding_ge2e_loss_amd import _lib
    B, n, M, _ = S.shape
    s, dS = Buf(S.shape, S), Buf(S.shape)
    bl = Buf(gl.shape, gl) if gl is not None else None
    bp = Buf(gp.shape, gp) if gp is not None else None
    v = _lib.VARIANTS[variant]
    args = (eps, v, bl.ptr if bl else None, bp.ptr if bp else None, dS.ptr, None)
    if whole_entry:
        ok(lib.ge2e_calc_loss_bwd(s.ptr, B, N, M, *args), "ge2e_calc_loss_bwd")
    else:
        ok(lib.ge2e_calc_loss_rows_bwd(s.ptr, B, n, N, j0, M, *args), "ge2e_calc_loss_rows_bwd")
    out = dS.get("d_sim")
    assert s.guards_intact() and (bl is None or bl.guards_intact()) and (bp is None or bp.guards_intact())
    return out


def check_loss(loss, per, ref, what):
    rows = ref["per"].shape[1] * ref["per"].shape[2]
    floor = 3e-7 * np.abs(ref["per"]).sum(axis=(1, 2)) + 2e-7 * rows
    print(f"{what}: loss max|diff| {np.abs(loss - ref['loss']).max():.3e} per max|diff| {np.abs(per - ref['per']).max():.3e}")
    assert np.all(np.abs(loss - ref["loss"]) <= 2e-5 * np.abs(ref["loss"]) + floor), f"{what} loss {loss} vs {ref['loss']}"
    assert np.allclose(per, ref["per"], rtol=2e-4, atol=2e-5), f"{what} per"


@pytest.mark.parametrize("case", hr.LOSS_CASES, ids=lambda c: "B{}_N{}_M{}_n{}_j{}_{}_eps{}_shift{}_{}".format(*c))
def test_calc_loss_forward_and_backward(lib, case):
    B, N, M, n, j0, variant, eps, shift, incoming = case
    S, gl, gp = hr.loss_inputs(case)
    ref = hr.calc_loss_rows_np(S, j0, eps, variant, gl, gp)
    floor = 0.0
    if variant == "softmax" and N == 1 and eps > 0:
        # one speaker: p_jj = 1 - O(eps), d_sim = g (p_jj - 1) is what fp32 leaves of 1/(1 + eps e^-s) - 1 -- the REFERENCE in
        # fp32 loses it the same way.  Measured on the CPU for these inputs: fp32-reference max error 1.70e-7 at max|d_sim|
        # 3.6e-3 (rel-Frobenius 1.1e-4); the kernel is allowed 4x the fp32 reference's max error = 6.8e-7 absolute.
        r32 = hr.calc_loss_rows_np(S, j0, eps, variant, gl, gp, dtype=torch.float32)
        floor = 4 * float(np.abs(r32["dS"].astype(np.float64) - ref["dS"]).max())
        print(f"{case}: fp32-reference d_sim max error {floor / 4:.3e}, max|ref| {np.abs(ref['dS']).max():.3e}")
    if variant == "softmax" and N == 1 and eps == 0:
        # log(exp s) - s: d_sim is EXACTLY zero (p_jj = 1); the fp64 reference leaves a 1e-16 residue.  A few fp32 ulp of g.
        floor = 4 * ULP * max(float(np.abs(x).max()) for x in (gl, gp) if x is not None)
    for whole_entry in ((True, False) if (n == N and j0 == 0) else (False,)):
        tag = f"{case} {'whole' if whole_entry else 'rows'}"
        loss, per = hip_calc_loss(lib, S, N, j0, eps, variant, whole_entry)
        check_loss(loss, per, ref, tag)
        loss2, _ = hip_calc_loss(lib, S, N, j0, eps, variant, whole_entry, want_per=False)     # per_emb_loss = NULL
        assert np.array_equal(loss, loss2), tag
        dS = hip_calc_loss_bwd(lib, S, N, j0, eps, variant, gl, gp, whole_entry)
        grad_close(dS, ref["dS"], tag + " d_sim", floor)


def test_contrast_exact_tie_between_the_two_largest_others(lib):
    """The two largest other-speaker entries of every row are bit-equal: forward equals the reference; the gradient of the
    max term lands on exactly ONE of the pair, and the pair's total equals the reference's."""
    S, gl, gp, pairs = hr.tie_inputs()
    B, N, M, _ = S.shape
    ref = hr.calc_loss_rows_np(S, 0, 1e-6, "contrast", gl, gp)
    for whole_entry in (True, False):
        loss, per = hip_calc_loss(lib, S, N, 0, 1e-6, "contrast", whole_entry)
        check_loss(loss, per, ref, "tie")
        dS = hip_calc_loss_bwd(lib, S, N, 0, 1e-6, "contrast", gl, gp, whole_entry)
        got_pair = np.take_along_axis(dS, pairs, axis=3)
        ref_pair = np.take_along_axis(ref["dS"], pairs, axis=3)
        assert np.all((got_pair != 0).sum(axis=3) == 1), "the max term's gradient must land on exactly one of the tied pair"
        assert np.all((ref_pair != 0).sum(axis=3) == 1)
        assert rel_fro(got_pair.sum(axis=3), ref_pair.sum(axis=3)) < 1e-5
        rest_got, rest_ref = dS.copy(), ref["dS"].copy()
        np.put_along_axis(rest_got, pairs, 0.0, axis=3)
        np.put_along_axis(rest_ref, pairs, 0.0, axis=3)
        grad_close(rest_got, rest_ref, "tie: columns outside the pair")


# ---- centroids, utterance centroids ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 2, 1), (3, 4, 2, 65), (2, 65, 17, 65), (1, 1, 2, 3)])
def test_centroids_and_their_backward(lib, shape):
    B, N, M, D = shape
    rng = np.random.default_rng(sum(shape))
    E = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal((B, N, D)).astype(np.float32)
    e = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    cent_ref = hr.centroids(e)
    cent_ref.backward(torch.tensor(g, dtype=torch.float64))
    be, cent = Buf(shape, E), Buf((B, N, D))
    ok(lib.ge2e_centroids(be.ptr, B, N, M, D, cent.ptr, None), "ge2e_centroids")
    assert np.allclose(cent.get("cent"), cent_ref.detach().numpy(), rtol=1e-5, atol=1e-7)
    bg, dE = Buf((B, N, D), g), Buf(shape)
    ok(lib.ge2e_centroids_bwd(bg.ptr, B, N, M, D, dE.ptr, None), "ge2e_centroids_bwd")
    grad_close(dE.get("dE"), e.grad.numpy(), f"{shape} centroids_bwd")
    assert be.guards_intact() and bg.guards_intact()


@pytest.mark.parametrize("shape", [(3, 5, 2, 1), (3, 4, 2, 65), (2, 65, 17, 65), (1, 1, 2, 3)])
def test_utterance_centroids_and_its_adjoint(lib, shape):
    B, N, M, D = shape
    rng = np.random.default_rng(sum(shape) + 1)
    E = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    e = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    u_ref = hr.utterance_centroids(e)
    u_ref.backward(torch.tensor(g, dtype=torch.float64))
    for data, want, what in ((E, u_ref.detach().numpy(), "U"), (g, e.grad.numpy(), "adjoint = the same call on g")):
        x, u = Buf(shape, data), Buf(shape)
        ok(lib.ge2e_utterance_centroids(x.ptr, B, N, M, D, u.ptr, None), "ge2e_utterance_centroids")
        got = u.get(what)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), what
        grad_close(got, want, f"{shape} {what}")
        assert x.guards_intact()


# ---- scale_grads -----------------------------------------------------------------------------------------------------------
def run_scale_grads(lib, dE, dw, db, g, want=("E", "w", "b"), offset=0):
    B = dE.shape[0]
    N, M, D = dE.shape[1:]
    bE, bw, bb, bg = Buf(dE.shape, dE, offset), Buf((B,), dw), Buf((B,), db), Buf(g.shape, g)
    gE, gw, gb = Buf(dE.shape, None, offset), Buf((1,)), Buf((1,))
    ok(lib.ge2e_scale_grads(bE.ptr, bw.ptr, bb.ptr, bg.ptr, g.size, B, N, M, D, gE.ptr if "E" in want else None,
                            gw.ptr if "w" in want else None, gb.ptr if "b" in want else None, None), "ge2e_scale_grads")
    torch.cuda.synchronize()
    out = {}
    for key, buf in (("E", gE), ("w", gw), ("b", gb)):
        if key in want:
            out[key] = buf.get("g" + key)
        else:                                       # a NULL output: its (unpassed) buffer is pure poison, trivially
            assert buf.guards_intact()
    # out of place: the inputs are exactly what they were
    assert np.array_equal(bE.get("dE in"), dE) and np.array_equal(bw.get("dw in"), dw) and np.array_equal(bb.get("db in"), db)
    return out


def check_scale_grads(out, dE, dw, db, g, what):
    gE, gw, gb, sw, sb = hr.scale_grads(dE, dw, db, g)
    if "E" in out:
        assert np.array_equal(out["E"], gE), f"{what}: gE is not fp32(dE) * fp32(g) bit for bit"
    if "w" in out:
        assert abs(float(out["w"][0]) - gw) <= 1e-6 * sw, f"{what}: gw {out['w'][0]} vs {gw}"
    if "b" in out:
        assert abs(float(out["b"][0]) - gb) <= 1e-6 * sb, f"{what}: gb {out['b'][0]} vs {gb}"


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("nmd", [(3, 4, 5), (1, 7, 3), (3, 2, 7), (5, 3, 1)], ids=lambda s: f"mod{s[0] * s[1] * s[2] % 4}")
def test_scale_grads(lib, B, nmd):
    """N M D % 4 in {0, 1, 2, 3} (the float4 and the scalar path); g_count 1 and B with a non-uniform g; every output NULL in
    turn; B around one wave for the dw / db sums; out of place."""
    rng = np.random.default_rng(B + sum(nmd))
    dE = rng.standard_normal((B,) + nmd).astype(np.float32)
    dw, db = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    for g in (rng.standard_normal(1).astype(np.float32), rng.standard_normal(B).astype(np.float32)):
        for want in (("E", "w", "b"), ("w", "b"), ("E", "b"), ("E", "w")):
            out = run_scale_grads(lib, dE, dw, db, g, want)
            assert set(out) == set(want)
            check_scale_grads(out, dE, dw, db, g, f"B{B} {nmd} g{g.size} {want}")


def test_scale_grads_on_a_view_that_is_not_16_byte_aligned(lib):
    """N M D % 4 == 0 but dE / gE start 4 bytes past a 16-byte boundary (a contiguous view at an odd storage offset): the
    entry point takes float alignment (include/ge2e_hip.h) -- same products, no 16-byte access."""
    rng = np.random.default_rng(8)
    B, nmd = 5, (3, 4, 5)
    dE = rng.standard_normal((B,) + nmd).astype(np.float32)
    dw, db, g = (rng.standard_normal(B).astype(np.float32) for _ in range(3))
    for offset in (1, 2, 3):
        out = run_scale_grads(lib, dE, dw, db, g, offset=offset)
        check_scale_grads(out, dE, dw, db, g, f"offset {offset}")


# ---- grid caps -----------------------------------------------------------------------------------------------------------
# Every kernel here is a grid-stride loop under a capped grid.  The caps as the code has them today -- whoever moves a cap
# moves its case:
#   grid_for (ge2e_helpers.hip): 65 535 blocks -- utt_centroids_kernel, centroids_bwd_kernel, cos_bwd_k2a: 256 items per
#       block = 16 776 960 items; calc_loss_bwd_kernel: 4 rows per block = 262 140 rows
#   launch_scale_grads: 4 096 blocks x 256 threads x float4 = 4 194 304 elements
#   launch_centroids: 4 096 x 256 = 1 048 576 items;  launch_cos_centroids: 4 096 x 4 rows = 16 384 rows
#   launch_calc_loss: 1 024 blocks, one batch each
# Each case crosses its cap by a few hundred items (not a multiple of the grid); the reference is evaluated on sampled
# batches: the first, one in the middle, the first whose items lie entirely beyond cap x block, and the last.
def randn_dev(shape, seed):
    gen = torch.Generator(device=dev()).manual_seed(seed)
    return torch.randn(*shape, generator=gen, device=dev())


def out_dev(shape):
    return torch.full(shape, float("nan"), device=dev())


def test_grid_cap_utterance_centroids_and_centroids(lib):
    B, N, M, D = 65538, 4, 2, 64                     # B N D = 16 777 728 = cap + 768; batches >= 65535 lie beyond the first pass
    assert B * N * D > 65535 * 256 and 65535 * 256 // (N * D) <= B - 3
    E = randn_dev((B, N, M, D), 1)
    U, cent = out_dev((B, N, M, D)), out_dev((B, N, D))
    ok(lib.ge2e_utterance_centroids(E.data_ptr(), B, N, M, D, U.data_ptr(), None), "ge2e_utterance_centroids")
    ok(lib.ge2e_centroids(E.data_ptr(), B, N, M, D, cent.data_ptr(), None), "ge2e_centroids")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(cent).all())
    for b in (0, 30011, 65535, B - 1):
        e = E[b:b + 1].cpu().double()
        assert np.allclose(U[b:b + 1].cpu().numpy(), hr.utterance_centroids(e).numpy(), rtol=1e-5, atol=1e-6), b
        assert np.allclose(cent[b:b + 1].cpu().numpy(), hr.centroids(e).numpy(), rtol=1e-5, atol=1e-7), b


def test_grid_cap_centroids_bwd(lib):
    B, N, M, D = 65538, 4, 2, 32                     # B N M D = 16 777 728 = cap + 768
    assert B * N * M * D > 65535 * 256 and 65535 * 256 // (N * M * D) <= B - 3
    g = randn_dev((B, N, D), 2)
    dE = out_dev((B, N, M, D))
    ok(lib.ge2e_centroids_bwd(g.data_ptr(), B, N, M, D, dE.data_ptr(), None), "ge2e_centroids_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dE).all())
    for b in (0, 30011, 65535, B - 1):
        want = (g[b].cpu().double() / M).unsqueeze(1).expand(N, M, D).numpy()
        assert rel_fro(dE[b].cpu().numpy(), want) < 1e-5, b


def test_grid_cap_cos_sim_rows_forward_and_backward(lib):
    """cos_bwd_k2a (the leave-one-out slot's += into dE) beyond 65 535 blocks, and ge2e_cos_centroids_kernel beyond 4 096."""
    B, N, M, D, n, j0 = 65538, 3, 2, 128, 2, 1       # B n D = 16 777 728 = cap + 768; B n M = 262 152 rows (forward cap 16 384)
    assert B * n * D > 65535 * 256 and 65535 * 256 // (n * D) <= B - 3
    E, C = randn_dev((B, n, M, D), 3), randn_dev((B, N, D), 4)
    g = randn_dev((B, n, M, N), 5)
    cos = out_dev((B, n, M, N))
    ok(lib.ge2e_cos_sim_rows(E.data_ptr(), C.data_ptr(), B, n, N, j0, M, D, 1e-8, 1e-6, cos.data_ptr(), None), "ge2e_cos_sim_rows")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cos).all())
    sample = (0, 30011, 65535, B - 1)
    refs = {}
    saved = cos.clone()              # the saved forward result: the reference's on the sampled batches (compared on their own)
    for b in sample:
        refs[b] = hr.cos_rows_np(E[b:b + 1].cpu().numpy(), C[b:b + 1].cpu().numpy(), j0, g[b:b + 1].cpu().numpy())
        assert np.abs(cos[b:b + 1].cpu().numpy() - refs[b]["cos"]).max() <= 3e-6, b
        saved[b:b + 1] = torch.as_tensor(refs[b]["cos"].astype(np.float32), device=dev())
    dE, dC = out_dev((B, n, M, D)), out_dev((B, N, D))
    nbytes = int(lib.ge2e_cos_sim_rows_bwd_workspace_bytes(B, n, N, M, D))
    ws = Buf((nbytes // 4,))
    ok(lib.ge2e_cos_sim_rows_bwd(E.data_ptr(), C.data_ptr(), saved.data_ptr(), g.data_ptr(), B, n, N, j0, M, D, 1e-8, 1e-6,
                                 dE.data_ptr(), dC.data_ptr(), ws.ptr, nbytes, None), "ge2e_cos_sim_rows_bwd")
    torch.cuda.synchronize()
    assert ws.guards_intact()
    assert bool(torch.isfinite(dE).all()) and bool(torch.isfinite(dC).all())
    for b in sample:
        grad_close(dE[b:b + 1].cpu().numpy(), refs[b]["dE"], f"batch {b} dE")
        grad_close(dC[b:b + 1].cpu().numpy(), refs[b]["dC"], f"batch {b} dC")


@pytest.mark.parametrize("variant", ["softmax", "contrast"])
def test_grid_cap_calc_loss_bwd(lib, variant):
    from speaker_embedding_ge2e_loss_amd import _lib
    B, N, M, n, j0 = 43750, 4, 2, 3, 1               # B n M = 262 500 rows = cap + 360; batches >= 43690 lie beyond the first pass
    assert B * n * M > 65535 * 4 and 65535 * 4 // (n * M) <= B - 3
    S = randn_dev((B, n, M, N), 6) * 3.0
    gl, gp = randn_dev((B,), 7), randn_dev((B, n, M), 8)
    dS = out_dev((B, n, M, N))
    ok(lib.ge2e_calc_loss_rows_bwd(S.data_ptr(), B, n, N, j0, M, 1e-6, _lib.VARIANTS[variant], gl.data_ptr(), gp.data_ptr(),
                                   dS.data_ptr(), None), "ge2e_calc_loss_rows_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dS).all())
    for b in (0, 20011, 43690, B - 1):
        ref = hr.calc_loss_rows_np(S[b:b + 1].cpu().numpy(), j0, 1e-6, variant, gl[b:b + 1].cpu().numpy(), gp[b:b + 1].cpu().numpy())
        grad_close(dS[b:b + 1].cpu().numpy(), ref["dS"], f"{variant} batch {b} d_sim")


@pytest.mark.parametrize("variant", ["softmax", "contrast"])
def test_grid_cap_calc_loss_forward(lib, variant):
    """B = 1024 + 300 batches on 1 024 workgroups: 300 workgroups take a second batch through the same red[] array."""
    B, N, M, n, j0 = 1324, 5, 3, 5, 0
    rng = np.random.default_rng(12)
    S = (rng.standard_normal((B, n, M, N)) * 3).astype(np.float32)
    ref = hr.calc_loss_rows_np(S, j0, 1e-6, variant)
    for whole_entry in (True, False):
        loss, per = hip_calc_loss(lib, S, N, j0, 1e-6, variant, whole_entry)
        check_loss(loss, per, ref, f"B{B} {variant}")


def test_grid_cap_scale_grads(lib):
    """More than 4 194 304 elements with a per-batch g: the grid-stride loop together with the i / p4 batch index."""
    B, N, M, D = 70, 3, 4, 5003                      # 60 036 per batch (% 4 == 0), 4 202 520 in all = cap + 8 216
    assert B * N * M * D > 4096 * 256 * 4 and (N * M * D) % 4 == 0
    dE, g = randn_dev((B, N, M, D), 9), randn_dev((B,), 10)
    dw, db = randn_dev((B,), 11), randn_dev((B,), 12)
    gE, gwb = out_dev((B, N, M, D)), out_dev((2,))
    ok(lib.ge2e_scale_grads(dE.data_ptr(), dw.data_ptr(), db.data_ptr(), g.data_ptr(), B, B, N, M, D, gE.data_ptr(),
                            gwb.data_ptr(), gwb.data_ptr() + 4, None), "ge2e_scale_grads")
    torch.cuda.synchronize()
    want, gw, gb, sw, sb = hr.scale_grads(dE.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), g.cpu().numpy())
    assert np.array_equal(gE.cpu().numpy(), want)
    assert abs(float(gwb[0]) - gw) <= 1e-6 * sw and abs(float(gwb[1]) - gb) <= 1e-6 * sb


# ---- through the wrappers: the autograd Functions' batched backward ------------------------------------------------------
def test_wrappers_batched_backward(GF):
    B, N, M, D = 3, 7, 3, 40
    E, C, g = hr.cos_inputs((B, N, M, D, N, 0), seed=2)
    ref = hr.cos_rows_np(E, C, 0, g)
    e = torch.as_tensor(E, device=dev()).requires_grad_(True)
    c = torch.as_tensor(C, device=dev()).requires_grad_(True)
    cos = GF.cos_sim(e, c)
    assert cos.shape == (B, N, M, N)
    assert np.abs(cos.detach().cpu().numpy() - ref["cos"]).max() <= 3e-6
    cos.backward(torch.as_tensor(g, device=dev()))
    grad_close(e.grad.cpu().numpy(), ref["dE"], "GF.cos_sim dE")
    grad_close(c.grad.cpu().numpy(), ref["dC"], "GF.cos_sim dC")

    rng = np.random.default_rng(6)
    for variant in ("softmax", "contrast"):
        S = (rng.standard_normal((B, N, M, N)) * 3).astype(np.float32)
        gl, gp = rng.standard_normal(B).astype(np.float32), rng.standard_normal((B, N, M)).astype(np.float32)
        r = hr.calc_loss_rows_np(S, 0, 1e-6, variant, gl, gp)
        s = torch.as_tensor(S, device=dev()).requires_grad_(True)
        loss, per = GF.calc_loss(s, variant=variant)
        assert loss.shape == (B,) and per.shape == (B, N, M)
        check_loss(loss.detach().cpu().numpy(), per.detach().cpu().numpy(), r, f"GF.calc_loss {variant}")
        ((loss * torch.as_tensor(gl, device=dev())).sum() + (per * torch.as_tensor(gp, device=dev())).sum()).backward()
        grad_close(s.grad.cpu().numpy(), r["dS"], f"GF.calc_loss {variant} d_sim")

    e64 = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    gc, gu = rng.standard_normal((B, N, D)).astype(np.float32), rng.standard_normal((B, N, M, D)).astype(np.float32)
    (hr.centroids(e64) * torch.as_tensor(gc).double()).sum().backward()
    e1 = torch.as_tensor(E, device=dev()).requires_grad_(True)
    cent = GF.centroids(e1)
    assert np.allclose(cent.detach().cpu().numpy(), hr.centroids(e64).detach().numpy(), rtol=1e-5, atol=1e-7)
    cent.backward(torch.as_tensor(gc, device=dev()))
    grad_close(e1.grad.cpu().numpy(), e64.grad.numpy(), "GF.centroids backward")
    e64.grad = None
    (hr.utterance_centroids(e64) * torch.as_tensor(gu).double()).sum().backward()
    e2 = torch.as_tensor(E, device=dev()).requires_grad_(True)
    u = GF.utterance_centroids(e2)
    assert np.allclose(u.detach().cpu().numpy(), hr.utterance_centroids(e64).detach().numpy(), rtol=1e-5, atol=1e-6)
    u.backward(torch.as_tensor(gu, device=dev()))
    grad_close(e2.grad.cpu().numpy(), e64.grad.numpy(), "GF.utterance_centroids backward")
