"""GPU: the double-precision loss (ge2e_loss_fwd_bwd_f64 and the float64 route of functional.ge2e_loss / GE2ELoss).

Reference: the fp64 closed form (oracle.closed_form(dtype=np.float64)) only -- never the project's own fp32 kernels.
Inputs carry bits below fp32 (a seeded 1e-9 perturbation of the synthetic embeddings, renormalised in fp64 for the
unit-norm kinds), so an fp32 computation behind casts cannot pass.

Gate, per quantity q of a batch:  |q - q_ref| <= 1e-10 |q_ref| + 1e-13 S_q  (Frobenius norms for per and dE) with
    S_loss = S_dw = N M,   S_per = sqrt(N M),   S_dE = |w| sqrt(N M) / min_row |e|,   and   |d db| <= 1e-10 N M
(db is a cancelling sum of N M order-one terms: it is gated on that scale, not on its own size).  The absolute term is for
the degenerate cases, where a relative gate means nothing for the oracle either: `clustered` inputs at w = 200 saturate
the softmax (loss 0, |dE| ~ 1e-50 in one fp64 formulation and 1e-13 in another), and at D = 1 every cosine is +-1 and dE is
rounding noise.  Where the figures come from: on well-scaled cases the oracle's two independent fp64 formulations
(closed form, expand-form autograd) agree to <= 6.5e-15 on the loss, 2.4e-14 on per, 1.6e-14 on dE, 5.8e-15 on dw (relative)
and 1e-12 absolute on db; fp32 arithmetic on the same inputs is off by 5.7e-9 .. 3.1e-6 (loss) and 8.6e-8 .. 7.0e-6 (dE).
1e-10 is four orders above the first band and >= 50x below the second.

Worst errors measured on an MI355X (`-s` prints them per test; DESIGN.md section 3.8 keeps the table).
"""
import numpy as np
import pytest
import torch

from capi import functional as GF  # noqa: F401
from oracle import ge2e_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL, ABS = 1e-10, 1e-13
KINDS = ("unit", "raw", "clustered")
WS = (10.0, -3.0, 200.0)
VARIANTS = ("softmax", "contrast")
GRID = 512          # the kernel's largest grid: more batches than this and the stride loop runs


def inputs64(shape, kind, seed):
    """Synthetic embeddings with bits below fp32: float64(synth) + 1e-9 * randn, renormalised in fp64 where the kind is
    unit-norm.  The input must not sit on a pole of the gradient: where a centroid or a leave-one-out centroid vanishes
    (at D = 1 unit rows are exactly +-1, and a speaker with rows +1, -1 has the centroid 0), 1 / max(|c|, 1e-8) amplifies
    rounding residue by 1e8 in ANY formulation -- the oracle's two fp64 forms disagree at 1e-9 there -- so such a draw is
    skipped for the next seed (seed, seed + 1000, ...)."""
    for attempt in range(4000):
        E = orc.synth_embeddings(shape, kind, seed=seed + 1000 * attempt).astype(np.float64)
        E += 1e-9 * np.random.default_rng(seed + 101).standard_normal(shape)
        if kind in ("unit", "clustered"):
            E /= np.linalg.norm(E, axis=-1, keepdims=True)
        total = E.sum(axis=-2, keepdims=True)
        m = shape[-2]
        if min(np.linalg.norm(total / m, axis=-1).min(), np.linalg.norm((total - E) / (m - 1), axis=-1).min()) > 1e-3:
            break
    else:
        raise AssertionError(f"no regular draw for {shape} {kind}")
    # (a unit-norm "vector" of one element is exactly +-1: nothing below fp32 to carry)
    assert shape[-1] == 1 or np.any(E != E.astype(np.float32).astype(np.float64))
    return np.ascontiguousarray(E)


def run_f64(GF, E, w, b, variant="softmax", need_grad=True):
    e = torch.as_tensor(E, device=DEV)
    assert e.dtype == torch.float64
    wt = torch.tensor(float(w), device=DEV, dtype=torch.float64)
    bt = torch.tensor(float(b), device=DEV, dtype=torch.float64)
    shp = tuple(e.shape) if e.dim() == 4 else (1,) + tuple(e.shape)
    # poison every output first: a kernel that skips rows must not pass on stale allocator memory
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)  # noqa: E731
    out = GF.LossOutputs(loss=nan(shp[0]), per=nan(*shp[:3]), dE=nan(*shp) if need_grad else None,
                         dw=nan(shp[0]) if need_grad else None, db=nan(shp[0]) if need_grad else None)
    o = GF.loss_fwd_bwd(e, wt, bt, variant=variant, out=out, need_grad=need_grad)
    torch.cuda.synchronize()
    keys = ("loss", "per", "dE", "dw", "db") if need_grad else ("loss", "per")
    res = {k: getattr(o, k).cpu().numpy() for k in keys}
    for k, v in res.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), f"{k}: dtype {v.dtype}, finite {np.isfinite(v).all()}"
    return res                                                   # always batched: (B, ...)


WORST = {}


def gate(o, ref, E, w, what, worst=None):
    """The gate of the module docstring on every batch of a (B,N,M,D) result (o, ref: batched; E: (B,N,M,D))."""
    E4 = E
    B, N, M, _ = E4.shape
    nm = N * M
    worst = WORST.setdefault(worst or "all", {})
    for i in range(B):
        r = {k: np.asarray(v)[i] for k, v in ref.items()}
        min_norm = np.linalg.norm(E4[i].reshape(nm, -1), axis=1).min()
        checks = [("loss", abs(o["loss"][i] - r["loss"]), REL * abs(r["loss"]) + ABS * nm, abs(r["loss"])),
                  ("per", np.linalg.norm(o["per"][i] - r["per"]), REL * np.linalg.norm(r["per"]) + ABS * np.sqrt(nm),
                   np.linalg.norm(r["per"]))]
        if "dE" in o:
            checks += [("dE", np.linalg.norm(o["dE"][i] - r["dE"]),
                        REL * np.linalg.norm(r["dE"]) + ABS * abs(w) * np.sqrt(nm) / min_norm, np.linalg.norm(r["dE"])),
                       ("dw", abs(o["dw"][i] - r["dw"]), REL * abs(r["dw"]) + ABS * nm, abs(r["dw"])),
                       ("db", abs(o["db"][i] - r["db"]), REL * nm, float(nm))]
        for name, err, bound, size in checks:
            rel = err / size if size > 0 else 0.0
            # the table: the worst share of the bound over all cases, and the worst relative error over the well-scaled
            # ones (where the relative term is the larger part of the bound; db: relative to N M)
            if err / bound >= worst.get(name + " share", (-1.0,))[0]:
                worst[name + " share"] = (err / bound, err, what)
            if REL * size >= 0.5 * bound and rel >= worst.get(name, (-1.0,))[0]:
                worst[name] = (rel, err, what)
            assert err <= bound, f"{what} batch {i}: {name} off by {err:.3e} (relative {rel:.3e}), bound {bound:.3e}"


def report(key):
    for name, (rel, err, what) in sorted(WORST.get(key, {}).items()):
        print(f"[f64 worst] {key:>24s} {name:>10s}: {rel:.2e} (absolute {err:.2e}) at {what}")


def b_for(w):
    return -0.5 * w


SMALL_SHAPES = [(4, 5, 256), (7, 3, 36), (5, 2, 12), (5, 2, 3), (5, 2, 1), (16, 4, 64), (130, 4, 64), (64, 10, 256),
                (17, 16, 20), (33, 3, 130)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_vs_fp64_closed_form(GF, shape, variant):
    """B = 1, forward + backward and forward only, every kind and every w: BASELINE's cfg1 / cfg2 / cfg3 shapes, ragged
    shapes (no dimension a multiple of the 16 x 16 x 4 tile), D = 1 and D = 3."""
    key = f"{'x'.join(map(str, shape))}/{variant}"
    for kind in KINDS:
        for w in WS:
            E = inputs64(shape, kind, seed=sum(shape) + len(kind))
            ref = orc.closed_form(E, w, b_for(w), variant=variant, dtype=np.float64)
            what = f"{shape} {kind} w={w} {variant}"
            o = run_f64(GF, E, w, b_for(w), variant)
            gate(o, {k: np.asarray(v)[None] for k, v in ref.items()}, E[None], w, what, key)
            f = run_f64(GF, E, w, b_for(w), variant, need_grad=False)
            gate(f, {k: np.asarray(v)[None] for k, v in ref.items()}, E[None], w, what + " fwd-only", key)
            assert np.array_equal(f["loss"], o["loss"]) and np.array_equal(f["per"], o["per"])
    report(key)


@pytest.mark.parametrize("cfg", ["cfg4", "cfg5"])
def test_accuracy_large_baseline_shapes(GF, cfg):
    """BASELINE's cfg4 (256, 10, 256) and cfg5 (1024, 10, 768), one batch each."""
    shape, cases = {"cfg4": ((256, 10, 256), [("unit", "softmax"), ("clustered", "contrast"), ("raw", "softmax")]),
                    "cfg5": ((1024, 10, 768), [("clustered", "softmax")])}[cfg]
    for kind, variant in cases:
        E = inputs64(shape, kind, seed=5)
        ref = orc.closed_form(E, 10.0, -5.0, variant=variant, dtype=np.float64)
        o = run_f64(GF, E, 10.0, -5.0, variant)
        gate(o, {k: np.asarray(v)[None] for k, v in ref.items()}, E[None], 10.0, f"{cfg} {kind} {variant}", cfg)
    report(cfg)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("stack", [(3, 64, 10, 256), (3, 7, 3, 36), (GRID + 9, 5, 2, 12), (2 * GRID + 1, 4, 5, 16)],
                         ids=lambda s: "x".join(map(str, s)))
def test_accuracy_stacks(GF, stack, variant):
    """B = 3 and B beyond the grid (the grid-stride loop and the reuse of a workgroup's workspace slice)."""
    key = f"B{'x'.join(map(str, stack))}/{variant}"
    for kind, w in (("unit", 10.0), ("raw", -3.0), ("clustered", 200.0)):
        E = inputs64(stack, kind, seed=stack[0])
        ref = orc.closed_form(E, w, b_for(w), variant=variant, dtype=np.float64)
        o = run_f64(GF, E, w, b_for(w), variant)
        gate(o, ref, E, w, f"{stack} {kind} w={w} {variant}", key)
        f = run_f64(GF, E, w, b_for(w), variant, need_grad=False)
        assert np.array_equal(f["loss"], o["loss"]) and np.array_equal(f["per"], o["per"])
    report(key)


def test_module_and_functional_route(GF):
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    shape = (16, 4, 64)
    nm = shape[0] * shape[1]
    E = inputs64(shape, "unit", seed=8)
    ref = orc.closed_form(E, 10.0, -5.0, dtype=np.float64)
    ulp32 = 1.2e-7

    def check_module(scale):
        mod = GE2ELoss(HParams(DEV))
        e = torch.as_tensor(E, device=DEV).requires_grad_()
        loss = mod(e)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        (loss if scale == 1.0 else scale * loss).backward()
        assert e.grad.dtype == torch.float64 and mod.w.grad.dtype == torch.float32 and mod.b.grad.dtype == torch.float32
        assert abs(loss.item() - ref["loss"]) <= REL * abs(ref["loss"]) + ABS * nm
        dE = e.grad.cpu().numpy()
        assert np.linalg.norm(dE - scale * ref["dE"]) <= REL * scale * np.linalg.norm(ref["dE"]) + ABS * scale * 10.0 * np.sqrt(nm)
        # the parameters are fp32: their gradients are the fp64 values rounded to fp32
        assert abs(mod.w.grad.item() - scale * ref["dw"]) <= ulp32 * abs(scale * ref["dw"]) + REL * nm
        assert abs(mod.b.grad.item() - scale * ref["db"]) <= ulp32 * abs(scale * ref["db"]) + REL * nm * scale
        return loss.detach().clone(), e.grad.clone()

    l1, g1 = check_module(1.0)
    l2, g2 = check_module(2.0)                                   # an upstream gradient scales, in float64
    assert torch.equal(l1, l2) and torch.equal(2.0 * g1, g2)

    # float64 w / b (the gradcheck case): float64 gradients for them too
    e = torch.as_tensor(E, device=DEV).requires_grad_()
    w64 = torch.tensor(10.0, device=DEV, dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor(-5.0, device=DEV, dtype=torch.float64, requires_grad=True)
    GF.ge2e_loss(e, w64, b64).backward()
    assert w64.grad.dtype == torch.float64 and abs(w64.grad.item() - ref["dw"]) <= REL * abs(ref["dw"]) + ABS * nm
    assert b64.grad.dtype == torch.float64 and abs(b64.grad.item() - ref["db"]) <= REL * nm
    assert torch.equal(e.grad, g1)

    # an explicit impl names an fp32 kernel: the cast route, unchanged -- float64 tensors with fp32-grade numbers
    w32 = torch.tensor(10.0, device=DEV, requires_grad=True)
    b32 = torch.tensor(-5.0, device=DEV, requires_grad=True)
    e = torch.as_tensor(E, device=DEV).requires_grad_()
    lg = GF.ge2e_loss(e, w32, b32, impl="generic")
    lg.backward()
    assert lg.dtype == torch.float64 and e.grad.dtype == torch.float64
    err = np.linalg.norm(e.grad.cpu().numpy() - ref["dE"]) / np.linalg.norm(ref["dE"])
    assert 1e-10 < err < 1e-4, err
    with pytest.raises(ValueError, match="float32 kernel"):
        GF.loss_fwd_bwd(torch.as_tensor(E, device=DEV), w64.detach(), b64.detach(), impl="generic")

    # float16 input behaves as before: computed in fp32 behind casts, float16 out
    mod = GE2ELoss(HParams(DEV))
    e16 = torch.as_tensor(E, device=DEV).half().requires_grad_()
    l16 = mod(e16)
    l16.backward()
    assert l16.dtype == torch.float16 and e16.grad.dtype == torch.float16 and mod.w.grad.dtype == torch.float32
    assert abs(l16.item() - ref["loss"]) <= 2e-2 * abs(ref["loss"])

    # graph=True admits fp32 only: a float64 input stays on the eager node, same bits, nothing captured
    modg = GE2ELoss(HParams(DEV), graph=True)
    for _ in range(3):
        e = torch.as_tensor(E, device=DEV).requires_grad_()
        modg.zero_grad(set_to_none=True)
        lossg = modg(e)
        lossg.backward()
        assert lossg.dtype == torch.float64 and torch.equal(lossg.detach(), l1) and torch.equal(e.grad, g1)
    assert len(modg._steps) == 0

    # a (B,N,M,D) stack through the module
    Es = inputs64((3,) + shape, "raw", seed=9)
    refs = orc.closed_form(Es, 10.0, -5.0, dtype=np.float64)
    mod = GE2ELoss(HParams(DEV))
    e = torch.as_tensor(Es, device=DEV).requires_grad_()
    losses = mod(e)
    assert losses.shape == (3,) and losses.dtype == torch.float64
    (losses * torch.tensor([1.0, 2.0, -0.5], device=DEV, dtype=torch.float64)).sum().backward()
    want = refs["dE"] * np.array([1.0, 2.0, -0.5])[:, None, None, None]
    assert np.linalg.norm(e.grad.cpu().numpy() - want) <= REL * np.linalg.norm(want) + ABS * 10.0 * np.sqrt(3 * nm) / 0.5


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(3, 3, 8), (4, 5, 16), (5, 2, 12), (2, 3, 3, 8)], ids=lambda s: "x".join(map(str, s)))
def test_gradcheck(GF, shape, variant):
    """torch.autograd.gradcheck with torch's default tolerances: needs float64 all the way through (the same function
    computed in fp32 behind casts fails it)."""
    e = torch.as_tensor(orc.synth_embeddings(shape, "unit", seed=3).astype(np.float64), device=DEV).requires_grad_()
    w = torch.tensor(10.0, device=DEV, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(-5.0, device=DEV, dtype=torch.float64, requires_grad=True)
    if len(shape) == 3:
        fn = lambda e, w, b: GF.ge2e_loss(e, w, b, variant=variant)  # noqa: E731
    else:
        fn = lambda e, w, b: GF.ge2e_loss(e, w, b, variant=variant).sum()  # noqa: E731
    assert torch.autograd.gradcheck(fn, (e, w, b))


def test_determinism_and_position_independence(GF):
    """Two runs give the same bits; a batch gives the same bits alone and at positions 0, 1 and last of a stack larger than
    the grid."""
    for variant in VARIANTS:
        shape = (7, 3, 36)
        B = GRID + 5
        E = inputs64((B,) + shape, "raw", seed=13)
        one = E[17].copy()
        for pos in (0, 1, B - 1):
            E[pos] = one
        a = run_f64(GF, E, 10.0, -5.0, variant)
        b = run_f64(GF, E, 10.0, -5.0, variant)
        s = run_f64(GF, one, 10.0, -5.0, variant)
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{variant} {k}: two runs differ"
            for pos in (0, 1, 17, B - 1):
                assert np.array_equal(a[k][pos], s[k][0]), f"{variant} {k}: position {pos} differs from the batch alone"
    E = inputs64((64, 10, 256), "unit", seed=14)
    a, b = run_f64(GF, E, 10.0, -5.0), run_f64(GF, E, 10.0, -5.0)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_access_outside_the_buffers(GF, variant):
    """E, dE and per live inside larger NaN-filled buffers at a ragged shape: the guards stay NaN (nothing written outside),
    the outputs have no NaN (no guard read into a result)."""
    B, N, M, D = 2, 7, 3, 37
    G = 64                                                       # guard elements either side (keeps 16-byte alignment)
    E = inputs64((B, N, M, D), "raw", seed=21)
    ref = orc.closed_form(E, 10.0, -5.0, variant=variant, dtype=np.float64)
    nE, nP = B * N * M * D, B * N * M

    def guarded(n):
        return torch.full((n + 2 * G,), float("nan"), device=DEV, dtype=torch.float64)

    bufE, bufD, bufP = guarded(nE), guarded(nE), guarded(nP)
    bufE[G:G + nE] = torch.as_tensor(E, device=DEV).reshape(-1)
    e = bufE[G:G + nE].view(B, N, M, D)
    sc = torch.full((3, B), float("nan"), device=DEV, dtype=torch.float64)
    out = GF.LossOutputs(loss=sc[0], per=bufP[G:G + nP].view(B, N, M), dE=bufD[G:G + nE].view(B, N, M, D), dw=sc[1], db=sc[2])
    w = torch.tensor(10.0, device=DEV, dtype=torch.float64)
    b = torch.tensor(-5.0, device=DEV, dtype=torch.float64)
    GF.loss_fwd_bwd(e, w, b, variant=variant, out=out)
    torch.cuda.synchronize()
    for buf, n in ((bufE, nE), (bufD, nE), (bufP, nP)):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all()), "guard overwritten"
    assert torch.equal(bufE[G:G + nE].view(B, N, M, D).cpu(), torch.as_tensor(E))
    o = {k: getattr(out, k).cpu().numpy() for k in ("loss", "per", "dE", "dw", "db")}
    assert all(np.isfinite(v).all() for v in o.values())
    gate(o, ref, E, 10.0, f"guarded {variant}", "guarded")
