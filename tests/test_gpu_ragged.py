"""GPU: the ragged loss (ge2e_loss_fwd_bwd_ragged, functional.ge2e_loss_ragged, GE2ELoss(...)(e, counts=...)).

Reference: tests/ragged_ref.py (torch autograd in float64 on per-speaker slices) and the golden vectors -- never the kernel.
The C-ABI tests call through ctypes on the guarded buffers of tests/guarded.py: inputs between NaN / sentinel guards,
outputs NaN-poisoned, the workspace exactly ge2e_workspace_bytes_ragged bytes between guard bands, filled with 0xFF bytes
in one run and 0x00 in another (the two must agree bit for bit), every guard intact afterwards.

Gate: rowlist_harness.check_rows -- the exact-fp32 row of dense_harness.TOL (loss 5e-6, dE 1e-5, dw 2e-5) through the formulas
of dense_harness.check_dense(..., strict=False), restated with nm = R because per is [R]:
    |loss - ref| <= 5e-6 |ref| + 3e-7 sum|per| + 1e-6 + 2e-7 R;    per: rtol 1e-4, atol 2e-5
    dE: rel-Frobenius <= 1e-5 (or max-abs <= 1e-8 for a vanishing gradient) and max-abs <= 4e-5 max(1, max|dE|)
    |dw - ref| <= 2e-5 |ref| + 1e-5 + 1e-7 R;    |db - ref| <= 1e-4 + 3e-7 R           (strict: without the R terms)
Inputs: unit rows centre[speaker] + 0.5 noise, seeded; w = 10, b = -5.  `-s` prints every figure before it is asserted.
"""
import numpy as np
import pytest
import torch

from capi import GF, lib  # noqa: F401
from conftest import golden_names, load_golden
from rowlist_cases import EDGE, case
from rowlist_harness import BIAS, DEV, VARIANTS, W, WT, batch_of, check_rows, offsets_of, same_bits
from rowlist_harness import run_ragged as run

pytestmark = pytest.mark.gpu


# ---- 1. edge shapes ----------------------------------------------------------------------------------------------------------
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
    check_rows(batch_of(full, 0), ref, f"{name}/{variant}")
    check_rows(batch_of(fwd, 0), ref, f"{name}/{variant}/fwd")


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
        check_rows(batch_of(a, i), cases[i][1], f"B3 batch {i} {counts[i]} {variant}")
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
        check_rows(batch_of(o, i), cases[i][1], f"B515 batch {i} {variant}", quiet=i % 103 != 0)
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
    check_rows(o, ref, name, strict=True)
    if (N, M, D) == (64, 10, 256):
        dev = torch.device(DEV)
        gen = GF.loss_fwd_bwd(torch.as_tensor(g["E"], device=dev), torch.tensor(float(g["w"]), device=dev),
                              torch.tensor(float(g["b"]), device=dev), impl="generic", need_per=True)
        torch.cuda.synchronize()
        gref = {"loss": gen.loss[0].item(), "per": gen.per[0].cpu().numpy().reshape(R), "dE": gen.dE[0].cpu().numpy().reshape(R, D),
                "dw": gen.dw[0].item(), "db": gen.db[0].item()}
        check_rows(o, gref, name + " vs generic", strict=True, factor=2.0)


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
    check_rows({"loss": 3 * loss.item(), "per": 3 * raw.per[0].cpu().numpy(), "dE": e.grad.cpu().numpy(), "dw": w.grad.item(),
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
        check_rows({"loss": g[i] * losses[i].item(), "per": g[i] * r["per"], "dE": es.grad[i].cpu().numpy(), "dw": g[i] * r["dw"],
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
    check_rows({"loss": lr.item(), "per": refd["per"], "dE": gr.cpu().numpy(), "dw": gw.item(), "db": gb.item()}, dense,
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
