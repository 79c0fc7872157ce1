"""GPU: the ragged loss (ge2e_loss_fwd_bwd_ragged, functional.ge2e_loss_ragged, GE2ELoss(...)(e, counts=...)).

Reference: tests/ragged_ref.py (torch autograd in float64 on per-speaker slices) and the golden vectors -- never the kernel.
The C-ABI tests call through ctypes on the guarded buffers of tests/guarded.py: inputs between NaN / sentinel guards,
outputs NaN-poisoned, the workspace exactly ge2e_workspace_bytes_ragged bytes between guard bands, filled with 0xFF bytes
in one run and 0x00 in another (the two must agree bit for bit), every guard intact afterwards.

Gate: the exact-fp32 row of test_gpu_parity.TOL (loss 5e-6, dE 1e-5, dw 2e-5) through the formulas of its
check(..., strict=False), restated here with nm = R because per is [R]:
    |loss - ref| <= 5e-6 |ref| + 3e-7 sum|per| + 1e-6 + 2e-7 R;    per: rtol 1e-4, atol 2e-5
    dE: rel-Frobenius <= 1e-5 (or max-abs <= 1e-8 for a vanishing gradient) and max-abs <= 4e-5 max(1, max|dE|)
    |dw - ref| <= 2e-5 |ref| + 1e-5 + 1e-7 R;    |db - ref| <= 1e-4 + 3e-7 R           (strict: without the R terms)
Inputs: unit rows centre[speaker] + 0.5 noise, seeded; w = 10, b = -5.  `-s` prints every figure before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import ragged_ref as rr
from conftest import golden_names, load_golden, rel_fro
from guarded import Buf, IntBuf, Workspace

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LT, GT, WT = 5e-6, 1e-5, 2e-5        # test_gpu_parity.TOL["generic"] == TOL["fused_f32"] == TOL["wave"]: exact fp32
W, BIAS = 10.0, -5.0
EPS, EPS_COS = rr.EPS, rr.EPS_COS
VARIANTS = ("softmax", "contrast")
VAR = {"softmax": 0, "contrast": 1}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from speaker_embedding_ge2e_loss_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def GF(lib):
    from speaker_embedding_ge2e_loss_amd import functional
    return functional


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(counts, D, seed, variant):
    E = rr.ragged_inputs(counts, D, seed)
    E.setflags(write=False)
    ref = rr.ragged_loss(E, counts, W, BIAS, variant=variant)
    for v in ref.values():
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return E, ref


def case(counts, D, seed, variant):
    """Inputs and fp64 reference of one batch: computed once, shared, read-only."""
    return _case(tuple(int(c) for c in counts), int(D), int(seed), variant)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(o, ref, what, strict=False, factor=1.0, quiet=False):
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


def run(lib, E, offsets, variant, want_grad=True, pattern=0xFF, w=W, b=BIAS, finite=True):
    """One ge2e_loss_fwd_bwd_ragged call on guarded buffers.  E (B, R, D) float32, offsets (B, N+1) int32 -> numpy outputs."""
    B, R, D = E.shape
    N = offsets.shape[1] - 1
    what = f"ragged B{B} N{N} R{R} D{D} {variant} {'fwd+bwd' if want_grad else 'fwd'} fill {pattern:#04x}"
    e, off, wb, bb = Buf(E.shape, E), IntBuf(offsets.shape, offsets), Buf((1,), [w]), Buf((1,), [b])
    outs = {"loss": Buf((B,)), "per": Buf((B, R))}
    if want_grad:
        outs.update(dE=Buf(E.shape), dw=Buf((B,)), db=Buf((B,)))
    nbytes = int(lib.ge2e_workspace_bytes_ragged(B, N, R, D, VAR[variant]))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    code = lib.ge2e_loss_fwd_bwd_ragged(e.ptr, off.ptr, B, N, R, D, wb.ptr, bb.ptr, EPS_COS, EPS, VAR[variant], ptr("loss"),
                                        ptr("per"), ptr("dE"), ptr("dw"), ptr("db"), ws.ptr, nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {k: v.get(f"{what} {k}", finite=finite) for k, v in outs.items()}       # guards intact, no NaN poison left
    for k, v in (("E", e), ("offsets", off), ("w", wb), ("b", bb)):
        assert v.guards_intact(), f"{what}: guard of {k} overwritten"
    assert same_bits(e.get(what + " E"), E) and np.array_equal(off.get(what + " offsets"), offsets), f"{what}: an input was modified"
    return res


def batch_of(o, i):
    return {k: v[i] for k, v in o.items()}


# ---- 1. edge shapes ----------------------------------------------------------------------------------------------------------
EDGE = {
    "D20_long_and_2row_speakers": ([2, 17, 3, 65, 2], 20),     # D no multiple of 16 or 64, a speaker longer than a wave
    "N67": ([2] * 67, 36),                                     # more than 64 centroids
    "speaker_over_row_tiles": ([130, 2], 8),                   # one speaker over several 16-row tiles
    "N1": ([5], 12),                                           # one speaker: a vanishing gradient
    "many_short": (np.random.default_rng(0).integers(2, 12, size=33).tolist(), 100),
    "D1": ([3, 2], 1),
    "D5": ([2, 3, 4], 5),
}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes(lib, name, variant):
    counts, D = EDGE[name]
    E, ref = case(counts, D, 1000 + len(counts) + D, variant)
    off = offsets_of(counts)[None]
    full = run(lib, E[None], off, variant, True, 0xFF)
    zero = run(lib, E[None], off, variant, True, 0x00)
    fwd = run(lib, E[None], off, variant, False, 0xFF)
    for k in full:
        assert same_bits(full[k], zero[k]), f"{name}/{variant}: {k} depends on what the workspace held before the call"
    assert same_bits(fwd["loss"], full["loss"]) and same_bits(fwd["per"], full["per"]), f"{name}/{variant}: forward-only differs"
    check(batch_of(full, 0), ref, f"{name}/{variant}")
    check(batch_of(fwd, 0), ref, f"{name}/{variant}/fwd")


# ---- 2. B > 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_batches_with_different_offsets(lib, variant):
    counts = ([2, 2, 2, 34], [10, 10, 10, 10], [17, 3, 18, 2])
    cases = [case(c, 64, 2000 + i, variant) for i, c in enumerate(counts)]
    E = np.stack([c[0] for c in cases])
    off = np.stack([offsets_of(c) for c in counts])
    a = run(lib, E, off, variant, True, 0xFF)
    again = run(lib, E, off, variant, True, 0x00)
    flipped = run(lib, np.ascontiguousarray(E[::-1]), np.ascontiguousarray(off[::-1]), variant, True, 0xFF)
    for i in range(3):
        check(batch_of(a, i), cases[i][1], f"B3 batch {i} {counts[i]} {variant}")
    for k in a:
        assert same_bits(a[k], again[k]), f"{variant} {k}: two launches differ"
        for i in range(3):   # the batch at index 0 sits at index 2 of the flipped stack, and the other way round
            assert same_bits(a[k][i], flipped[k][2 - i]), f"{variant} {k}: batch {i} depends on its position in the launch"


# ---- 3. more batches than workgroups: the grid-stride loop reuses a workgroup's workspace slice ----------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_slice_reuse_past_the_grid(lib, variant):
    B, D = 515, 4
    pats = ([2, 4], [3, 3], [4, 2])
    cases = [case(pats[i % 3], D, 3000 + i, variant) for i in range(B)]
    E = np.stack([c[0] for c in cases])
    off = np.stack([offsets_of(pats[i % 3]) for i in range(B)])
    o = run(lib, E, off, variant, True, 0xFF)
    for i in range(B):
        check(batch_of(o, i), cases[i][1], f"B515 batch {i} {variant}", quiet=i % 103 != 0)
    fwd = run(lib, E, off, variant, False, 0x00)
    assert same_bits(fwd["loss"], o["loss"]) and same_bits(fwd["per"], o["per"])


# ---- 4. pinned to the reference project's own numbers ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_golden_vectors_as_equal_counts(lib, GF, name):
    g = load_golden(name)
    N, M, D = g["E"].shape
    R = N * M
    E = np.ascontiguousarray(g["E"].reshape(1, R, D), dtype=np.float32)
    off = offsets_of([M] * N)[None]
    ref = {"loss": g["loss64"], "per": g["per64"].reshape(R), "dE": g.get("dE64", g["dE"]).reshape(R, D),
           "dw": g["dw64"], "db": g["db64"]}
    o = batch_of(run(lib, E, off, "softmax", True, 0xFF, w=float(g["w"]), b=float(g["b"])), 0)
    if "degenerate" in name:
        # 1e8-scale gradients on the clamped rows: compare relative to the largest entry (as test_golden_vectors does)
        print(f"{name}: dE max-abs {np.abs(o['dE'] - ref['dE']).max():.3e} of max {np.abs(ref['dE']).max():.3e}")
        assert np.abs(o["dE"] - ref["dE"]).max() <= 1e-5 * np.abs(ref["dE"]).max()
        assert np.allclose(o["loss"], ref["loss"], rtol=1e-5)
        return
    check(o, ref, name, strict=True)
    if (N, M, D) == (64, 10, 256):
        dev = torch.device(DEV)
        gen = GF.loss_fwd_bwd(torch.as_tensor(g["E"], device=dev), torch.tensor(float(g["w"]), device=dev),
                              torch.tensor(float(g["b"]), device=dev), impl="generic", need_per=True)
        torch.cuda.synchronize()
        gref = {"loss": gen.loss[0].item(), "per": gen.per[0].cpu().numpy().reshape(R), "dE": gen.dE[0].cpu().numpy().reshape(R, D),
                "dw": gen.dw[0].item(), "db": gen.db[0].item()}
        check(o, gref, name + " vs generic", strict=True, factor=2.0)


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    dev = torch.device(DEV)
    counts = [2, 17, 3, 65, 2]
    D, R = 20, 89
    E, ref = case(counts, D, 1000 + len(counts) + D, "softmax")

    def leaves():
        return (torch.as_tensor(E, device=dev).requires_grad_(True), torch.tensor(W, device=dev, requires_grad=True),
                torch.tensor(BIAS, device=dev, requires_grad=True))

    # host counts and device offsets: the same launch
    e, w, b = leaves()
    loss = GF.ge2e_loss_ragged(e, counts, w, b)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (3 * loss).backward()
    e2, w2, b2 = leaves()
    off_dev = torch.as_tensor(offsets_of(counts), device=dev)
    loss2 = GF.ge2e_loss_ragged(e2, off_dev, w2, b2)
    (3 * loss2).backward()
    assert torch.equal(loss, loss2) and torch.equal(e.grad, e2.grad) and torch.equal(w.grad, w2.grad) and torch.equal(b.grad, b2.grad)
    # a repeated table is not uploaded again
    e3, w3, b3 = leaves()
    n_up = len(GF._ragged_uploads)
    assert torch.equal(GF.ge2e_loss_ragged(e3, torch.tensor(counts), w3, b3), loss) and len(GF._ragged_uploads) == n_up
    raw = GF.loss_fwd_bwd_ragged(e.detach(), counts, w.detach(), b.detach(), need_per=True)
    assert raw.per.shape == (1, R) and raw.dE.shape == (1, R, D) and torch.equal(raw.loss[0], loss.detach())
    three = {"loss": 3 * ref["loss"], "per": 3 * ref["per"], "dE": 3 * ref["dE"], "dw": 3 * ref["dw"], "db": 3 * ref["db"]}
    check({"loss": 3 * loss.item(), "per": 3 * raw.per[0].cpu().numpy(), "dE": e.grad.cpu().numpy(), "dw": w.grad.item(),
           "db": b.grad.item()}, three, "3 * ge2e_loss_ragged")

    # the module: GE2ELoss(hp)(e, counts=c) is the functional call, eager and with graph=True (eager too: nothing captured)
    for graph in (False, True):
        mod = GE2ELoss(HParams(DEV), graph=graph)
        for _ in range(3 if graph else 1):
            em = torch.as_tensor(E, device=dev).requires_grad_(True)
            mod.zero_grad(set_to_none=True)
            lm = mod(em, counts=counts)
            (3 * lm).backward()
            assert torch.equal(lm.detach(), loss.detach()) and torch.equal(em.grad, e.grad)
            assert torch.equal(mod.w.grad, w.grad) and torch.equal(mod.b.grad, b.grad)
        assert len(mod._steps) == 0

    # a (B, R, D) stack with per-batch counts and a vector of incoming gradients
    cs = ([2, 2, 2, 34], [10, 10, 10, 10], [17, 3, 18, 2])
    cases = [case(c, 64, 2000 + i, "softmax") for i, c in enumerate(cs)]
    es = torch.as_tensor(np.stack([c[0] for c in cases]), device=dev).requires_grad_(True)
    mod = GE2ELoss(HParams(DEV))
    losses = mod(es, counts=cs)
    assert losses.shape == (3,)
    g = [1.0, 2.0, -0.5]
    (losses * torch.tensor(g, device=dev)).sum().backward()
    for i in range(3):
        r = cases[i][1]
        check({"loss": g[i] * losses[i].item(), "per": g[i] * r["per"], "dE": es.grad[i].cpu().numpy(), "dw": g[i] * r["dw"],
               "db": g[i] * r["db"]},
              {"loss": g[i] * r["loss"], "per": g[i] * r["per"], "dE": g[i] * r["dE"], "dw": g[i] * r["dw"], "db": g[i] * r["db"]},
              f"stack batch {i}")
    want_dw = sum(g[i] * float(cases[i][1]["dw"]) for i in range(3))
    assert abs(mod.w.grad.item() - want_dw) <= 3 * (WT * max(abs(g[i] * float(cases[i][1]["dw"])) for i in range(3)) + 1e-5 + 1e-7 * 40)

    # equal counts: the dense loss
    N, M, D2 = 6, 4, 32
    Ed, refd = case([M] * N, D2, 77, "softmax")
    mod = GE2ELoss(HParams(DEV))
    ed = torch.as_tensor(Ed, device=dev).requires_grad_(True)
    lr = mod(ed, counts=[M] * N)
    lr.backward()
    gr, gw, gb = ed.grad.clone(), mod.w.grad.clone(), mod.b.grad.clone()
    ed.grad = None
    mod.zero_grad(set_to_none=True)
    ld = mod(ed.view(N, M, D2))
    ld.backward()
    dense = {"loss": ld.item(), "per": refd["per"], "dE": ed.grad.cpu().numpy(), "dw": mod.w.grad.item(), "db": mod.b.grad.item()}
    check({"loss": lr.item(), "per": refd["per"], "dE": gr.cpu().numpy(), "dw": gw.item(), "db": gb.item()}, dense,
          "ragged at equal counts vs GE2ELoss(e.view(N, M, D))")

    # dtypes: bf16 in, bf16 out (computed in fp32 behind differentiable casts); fp64 is not silently cast down
    eb = torch.as_tensor(E, device=dev).bfloat16().requires_grad_(True)
    mod = GE2ELoss(HParams(DEV))
    lb = mod(eb, counts=counts)
    lb.backward()
    assert lb.dtype == torch.bfloat16 and eb.grad.dtype == torch.bfloat16 and mod.w.grad.dtype == torch.float32
    # ... which is the fp32 launch on the rounded rows, rounded once more
    l32 = GF.ge2e_loss_ragged(eb.detach().float(), counts, w.detach(), b.detach())
    assert torch.equal(lb.detach(), l32.to(torch.bfloat16)) and bool(torch.isfinite(eb.grad).all())
    with pytest.raises(NotImplementedError, match="float64"):
        mod(torch.as_tensor(E, device=dev).double(), counts=counts)
    with pytest.raises(NotImplementedError, match="float64"):
        GF.ge2e_loss_ragged(torch.as_tensor(E, device=dev).double(), counts, w.detach(), b.detach())
    # host counts are validated before anything is launched
    with pytest.raises(ValueError):
        mod(torch.as_tensor(E, device=dev), counts=[2, 17, 3, 65, 1, 1])
    with pytest.raises(ValueError):
        mod(torch.as_tensor(E, device=dev), counts=[2, 17, 3, 65])
