"""GPU: the ragged loss from speaker labels (ge2e_label_index, ge2e_loss_fwd_bwd_labeled, functional.ge2e_loss_labeled,
GE2ELoss(...)(e, labels=...)): rows in any order, sorted on the device.

References, never the code under test: numpy for the index kernel (argsort(kind="stable"), bincount, cumsum: exact integer
equality); for the loss tests/ragged_ref.py (torch autograd in float64) on the rows sorted by numpy's stable argsort, per and
dE scattered back to the caller's order, and the golden vectors.  The C-ABI tests call through ctypes on the guarded buffers
of tests/guarded.py: inputs between NaN / sentinel guards, outputs poisoned, the workspace exactly
ge2e_workspace_bytes_labeled (ge2e_label_index_workspace_bytes) bytes between guard bands, filled with 0xFF bytes in one run
and 0x00 in another (the two must agree bit for bit), every guard intact afterwards.

Gate: rowlist_harness.check_rows, unchanged (the exact-fp32 row of dense_harness.TOL through the formulas of that module's
docstring): the arithmetic is the same kernel's.  Inputs: ragged_ref.ragged_inputs, seeded; w = 10, b = -5.

How the shuffled cases are made: the LABELS of the sorted layout are permuted (seeded) and the rows are placed so that the
stable sort of those labels brings back the sorted batch of rowlist_cases.case -- any interleaving of the speakers, one fp64
reference per batch shared with tests/test_gpu_ragged.py.  (That the order IS the stable one is the index tests' business,
where it is held to numpy exactly; the golden test shuffles rows with a plain permutation.)  `-s` prints every figure
before it is asserted.
"""
import numpy as np
import pytest
import torch

from capi import GF, lib  # noqa: F401
from conftest import golden_names, load_golden
from rowlist_cases import EDGE, case
from rowlist_harness import BIAS, DEV, VARIANTS, W, batch_of, check_rows, offsets_of, run_index, run_ragged, same_bits
from rowlist_harness import run_labeled as run

pytestmark = pytest.mark.gpu


# ---- references ----------------------------------------------------------------------------------------------------------------
def index_ref(labels, N):
    """numpy: offsets (B, N+1) and the stable order (B, R) of labels (B, R) in [0, N)."""
    labels = np.asarray(labels)
    off = np.stack([np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))]) for row in labels]).astype(np.int32)
    order = np.stack([np.argsort(row, kind="stable") for row in labels]).astype(np.int32)
    return off, order


def shuffled(counts, D, seed, variant, sort=False):
    """One batch in shuffled row order: (E (R, D), labels (R,), order (R,), sorted E, its fp64 reference).  E[order] is the
    sorted batch of rowlist_cases.case(counts, D, seed, variant) bit for bit.  `sort`: the labels stay sorted."""
    Es, ref = case(counts, D, seed, variant)
    lab = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    if not sort:
        lab = lab[np.random.default_rng(seed + 77).permutation(len(lab))]
    order = np.argsort(lab, kind="stable")
    E = np.empty_like(Es)
    E[order] = Es
    return E, lab, order, Es, ref


def scattered(ref, order):
    """The reference of the sorted batch in the caller's row order."""
    out = dict(ref)
    for k in ("per", "dE"):
        v = np.empty_like(ref[k])
        v[order] = ref[k]
        out[k] = v
    return out


# ---- 1. the index kernel: exact integer equality with numpy ----------------------------------------------------------------------
def _index_cases():
    rng = np.random.default_rng(11)
    runs = np.concatenate([np.zeros(700), np.arange(900) % 3, np.full(300, 2), rng.integers(0, 3, 350), np.ones(250)])
    return {
        "all_equal": (1, np.zeros((1, 5))),
        "descending_pairs": (6, np.repeat(np.arange(5, -1, -1), 2)[None]),
        "already_sorted": (5, np.repeat(np.arange(5), [2, 3, 4, 2, 6])[None]),
        "N67_R300": (67, rng.integers(0, 67, (1, 300))),
        "N3_R2500_runs_across_chunks": (3, runs[None]),
        "N1100_R2200": (1100, rng.permutation(np.repeat(np.arange(1100), 2))[None]),    # counters in the workspace
        "B3": (4, rng.integers(0, 4, (3, 40))),
        "B515_past_the_grid": (2, rng.integers(0, 2, (515, 5))),
        "B3_N1100": (1100, np.stack([rng.permutation(np.repeat(np.arange(1100), 2)) for _ in range(3)])),
    }


INDEX_CASES = _index_cases()


@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_label_index_is_numpys_stable_argsort(lib, name):
    N, labels = INDEX_CASES[name]
    labels = labels.astype(np.int32)
    B, R = labels.shape
    assert labels.min() >= 0 and labels.max() < N
    off_ref, order_ref = index_ref(labels, N)
    off, order = run_index(lib, labels, N, 0xFF)
    print(f"{name}: B {B} N {N} R {R}: offsets differ at {int((off != off_ref).sum())}, order at {int((order != order_ref).sum())}")
    assert np.array_equal(off, off_ref), f"{name}: offsets"
    assert np.array_equal(order, order_ref), f"{name}: order is not the stable argsort"
    off2, order2 = run_index(lib, labels, N, 0x00)
    assert np.array_equal(off, off2) and np.array_equal(order, order2), f"{name}: two launches differ"
    if B > 1:     # the batch at index i sits at index B-1-i of the flipped stack
        offf, orderf = run_index(lib, labels[::-1], N, 0xFF)
        assert np.array_equal(offf[::-1], off) and np.array_equal(orderf[::-1], order), f"{name}: a batch depends on its position"


def test_label_index_clamps(lib):
    labels = np.array([[3, -5, 9, 0, 2, 7, -1, 1, 3, 2147483647, -2147483648, 1]], dtype=np.int32)
    off, order = run_index(lib, labels, 4)
    off_ref, order_ref = index_ref(np.clip(labels, 0, 3), 4)
    assert np.array_equal(off, off_ref) and np.array_equal(order, order_ref)


# ---- 2. the loss at the ragged kernel's edge shapes, rows shuffled -----------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes_shuffled(lib, name, variant):
    counts, D = EDGE[name]
    N = len(counts)
    E, lab, order, _, ref = shuffled(counts, D, 1000 + N + D, variant)
    ref = scattered(ref, order)
    full = run(lib, E[None], lab[None], N, variant, True, 0xFF)
    zero = run(lib, E[None], lab[None], N, variant, True, 0x00)
    fwd = run(lib, E[None], lab[None], N, variant, False, 0xFF)
    for k in full:
        assert same_bits(full[k], zero[k]), f"{name}/{variant}: {k} depends on what the workspace held before the call"
    assert same_bits(fwd["loss"], full["loss"]) and same_bits(fwd["per"], full["per"]), f"{name}/{variant}: forward-only differs"
    check_rows(batch_of(full, 0), ref, f"{name}/{variant}")
    check_rows(batch_of(fwd, 0), ref, f"{name}/{variant}/fwd")


# ---- 3. the same bits as the ragged entry on gathered rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(EDGE))
def test_same_bits_as_the_ragged_entry(lib, name, variant):
    counts, D = EDGE[name]
    N = len(counts)
    off = offsets_of(counts)[None]
    for sort in (False, True):
        E, lab, order, Es, _ = shuffled(counts, D, 1000 + N + D, variant, sort=sort)
        assert same_bits(E[order], Es) and (not sort or same_bits(E, Es))
        got = run(lib, E[None], lab[None], N, variant, True, 0xFF)
        want = run_ragged(lib, E[order][None], off, variant, True, 0xFF)
        what = f"{name}/{variant}/{'sorted labels' if sort else 'shuffled'}"
        for k in ("loss", "dw", "db"):
            assert same_bits(got[k], want[k]), f"{what}: {k}"
        for k in ("per", "dE"):     # the ragged call's outputs scattered back (sorted labels: order is the identity)
            back = np.empty_like(want[k][0])
            back[order] = want[k][0]
            assert same_bits(got[k][0], back), f"{what}: {k}"


# ---- 4. B > 1, and more batches than workgroups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_batches_with_their_own_shuffles(lib, variant):
    counts = ([2, 2, 2, 34], [10, 10, 10, 10], [17, 3, 18, 2])
    cases = [shuffled(c, 64, 2000 + i, variant) for i, c in enumerate(counts)]
    E, lab = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    assert not np.array_equal(lab[0], lab[1])
    a = run(lib, E, lab, 4, variant, True, 0xFF)
    again = run(lib, E, lab, 4, variant, True, 0x00)
    flipped = run(lib, E[::-1], lab[::-1], 4, variant, True, 0xFF)
    for i in range(3):
        check_rows(batch_of(a, i), scattered(cases[i][4], cases[i][2]), f"B3 batch {i} {counts[i]} {variant}")
    for k in a:
        assert same_bits(a[k], again[k]), f"{variant} {k}: two launches differ"
        for i in range(3):   # the batch at index 0 sits at index 2 of the flipped stack, and the other way round
            assert same_bits(a[k][i], flipped[k][2 - i]), f"{variant} {k}: batch {i} depends on its position in the launch"


@pytest.mark.parametrize("variant", VARIANTS)
def test_past_the_grid(lib, variant):
    B, D = 515, 4
    pats = ([2, 4], [3, 3], [4, 2])
    cases = [shuffled(pats[i % 3], D, 3000 + i, variant) for i in range(B)]
    E, lab = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    o = run(lib, E, lab, 2, variant, True, 0xFF)
    for i in range(B):
        check_rows(batch_of(o, i), scattered(cases[i][4], cases[i][2]), f"B515 batch {i} {variant}", quiet=i % 103 != 0)
    fwd = run(lib, E, lab, 2, variant, False, 0x00)
    assert same_bits(fwd["loss"], o["loss"]) and same_bits(fwd["per"], o["per"])


# ---- 5. pinned to the reference project's own numbers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_golden_vectors_shuffled(lib, name):
    g = load_golden(name)
    N, M, D = g["E"].shape
    R = N * M
    perm = np.random.default_rng(R + D).permutation(R)
    E = np.ascontiguousarray(g["E"].reshape(R, D)[perm], dtype=np.float32)[None]
    lab = np.repeat(np.arange(N), M)[perm].astype(np.int32)[None]
    ref = {"loss": g["loss64"], "per": g["per64"].reshape(R)[perm], "dE": g.get("dE64", g["dE"]).reshape(R, D)[perm],
           "dw": g["dw64"], "db": g["db64"]}
    o = batch_of(run(lib, E, lab, N, "softmax", True, 0xFF, w=float(g["w"]), b=float(g["b"])), 0)
    if "degenerate" in name:
        # 1e8-scale gradients on the clamped rows: compare relative to the largest entry (as test_golden_vectors does)
        print(f"{name}: dE max-abs {np.abs(o['dE'] - ref['dE']).max():.3e} of max {np.abs(ref['dE']).max():.3e}")
        assert np.abs(o["dE"] - ref["dE"]).max() <= 1e-5 * np.abs(ref["dE"]).max()
        assert np.allclose(o["loss"], ref["loss"], rtol=1e-5)
        return
    check_rows(o, ref, name, strict=True)


# ---- 6. the clamp: labels that break the contract stay inside the buffers --------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_labels_outside_the_contract(lib, variant):
    counts, D = [2, 3, 4], 5
    N = len(counts)
    E, lab, _, _, _ = shuffled(counts, D, 1000 + N + D, variant)
    wild = lab.copy()
    wild[np.flatnonzero(lab == 0)[0]] = -5
    wild[np.flatnonzero(lab == N - 1)[:2]] = N + 3
    assert np.array_equal(np.clip(wild, 0, N - 1), lab) and not np.array_equal(wild, lab)
    a = run(lib, E[None], wild[None], N, variant)
    c = run(lib, E[None], np.clip(wild, 0, N - 1)[None], N, variant)
    for k in a:
        assert same_bits(a[k], c[k]), f"{variant} {k}: labels outside [0, N) are not read as the clipped ones"
    # one speaker left with a single row (it divides by count - 1 = 0): the call is made, every guard is intact and the
    # inputs are unmodified (asserted in run); the numbers may be anything
    lone = lab.copy()
    lone[np.flatnonzero(lab == 0)[0]] = 1
    assert np.bincount(lone, minlength=N).tolist() == [1, 4, 4]
    o = run(lib, E[None], lone[None], N, variant, finite=False)
    print(f"{variant}: a speaker with one row gives loss {o['loss']}")


# ---- 7. the Python surface --------------------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    dev = torch.device(DEV)
    counts = [2, 17, 3, 65, 2]
    D, R, N = 20, 89, 5
    E, lab, order, _, ref = shuffled(counts, D, 1000 + N + D, "softmax")
    ref = scattered(ref, order)
    ids = np.array([7, -3, 42, 1000000007, 0])                # arbitrary ids: dense label k stands for the k-th smallest
    host = np.sort(ids)[lab].tolist()
    assert GF.dense_labels(host)[0].tolist() == lab.tolist()

    def leaves():
        return (torch.as_tensor(E, device=dev).requires_grad_(True), torch.tensor(W, device=dev, requires_grad=True),
                torch.tensor(BIAS, device=dev, requires_grad=True))

    # host labels with arbitrary ids and device labels (int32, int64): the same launch
    e, w, b = leaves()
    loss = GF.ge2e_loss_labeled(e, host, w, b)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (3 * loss).backward()
    for dtype in (torch.int32, torch.int64):
        e2, w2, b2 = leaves()
        loss2 = GF.ge2e_loss_labeled(e2, torch.as_tensor(lab, device=dev).to(dtype), w2, b2, num_speakers=N)
        (3 * loss2).backward()
        assert torch.equal(loss, loss2) and torch.equal(e.grad, e2.grad) and torch.equal(w.grad, w2.grad) and torch.equal(b.grad, b2.grad)
    # a repeated host table is not uploaded again
    e3, w3, b3 = leaves()
    n_up = len(GF._label_uploads)
    assert torch.equal(GF.ge2e_loss_labeled(e3, torch.tensor(host), w3, b3), loss) and len(GF._label_uploads) == n_up
    raw = GF.loss_fwd_bwd_labeled(e.detach(), host, w.detach(), b.detach(), need_per=True)
    assert raw.per.shape == (1, R) and raw.dE.shape == (1, R, D) and torch.equal(raw.loss[0], loss.detach())
    # (3 * loss).backward() against 3 x the fp64 reference; e.grad in the caller's row order
    three = {k: 3 * ref[k] for k in ("loss", "per", "dE", "dw", "db")}
    check_rows({"loss": 3 * loss.item(), "per": 3 * raw.per[0].cpu().numpy(), "dE": e.grad.cpu().numpy(), "dw": w.grad.item(),
                "db": b.grad.item()}, three, "3 * ge2e_loss_labeled")
    # ... and it is the ragged function on the rows the caller sorts, with the gradient scattered back
    es = torch.as_tensor(E[order], device=dev).requires_grad_(True)
    ls = GF.ge2e_loss_ragged(es, counts, w.detach(), b.detach())
    (3 * ls).backward()
    back = torch.empty_like(es.grad)
    back[torch.as_tensor(order, device=dev)] = es.grad
    assert torch.equal(ls.detach(), loss.detach()) and torch.equal(back, e.grad)

    # label_index: what the loss reads
    off_d, order_d = GF.label_index(torch.as_tensor(lab, device=dev), N)
    assert off_d.dtype == order_d.dtype == torch.int32 and off_d.is_cuda and order_d.is_cuda
    assert off_d.cpu().tolist() == offsets_of(counts).tolist() and np.array_equal(order_d.cpu().numpy(), order)
    off_b, order_b = GF.label_index(torch.as_tensor(np.stack([lab, lab[::-1].copy()]), device=dev).long(), N)
    assert off_b.shape == (2, N + 1) and order_b.shape == (2, R) and torch.equal(order_b[0], order_d)
    assert np.array_equal(order_b[1].cpu().numpy(), np.argsort(lab[::-1], kind="stable"))

    # the module: GE2ELoss(hp)(e, labels=l) is the functional call, eager and with graph=True (eager too: nothing captured)
    for graph in (False, True):
        mod = GE2ELoss(HParams(DEV), graph=graph)
        for _ in range(3 if graph else 1):
            em = torch.as_tensor(E, device=dev).requires_grad_(True)
            mod.zero_grad(set_to_none=True)
            lm = mod(em, labels=host)
            (3 * lm).backward()
            assert torch.equal(lm.detach(), loss.detach()) and torch.equal(em.grad, e.grad)
            assert torch.equal(mod.w.grad, w.grad) and torch.equal(mod.b.grad, b.grad)
        assert len(mod._steps) == 0
    mod = GE2ELoss(HParams(DEV))
    lm = mod(torch.as_tensor(E, device=dev), labels=torch.as_tensor(lab, device=dev), num_speakers=N)
    assert torch.equal(lm.detach(), loss.detach())

    # a (B, R, D) stack with per-batch labels and a vector of incoming gradients
    cs = ([2, 2, 2, 34], [10, 10, 10, 10], [17, 3, 18, 2])
    cases = [shuffled(c, 64, 2000 + i, "softmax") for i, c in enumerate(cs)]
    es = torch.as_tensor(np.stack([c[0] for c in cases]), device=dev).requires_grad_(True)
    losses = mod(es, labels=np.stack([c[1] for c in cases]) * 10 - 7)
    assert losses.shape == (3,)
    g = [1.0, 2.0, -0.5]
    (losses * torch.tensor(g, device=dev)).sum().backward()
    for i in range(3):
        r = scattered(cases[i][4], cases[i][2])
        check_rows({"loss": g[i] * losses[i].item(), "per": g[i] * r["per"], "dE": es.grad[i].cpu().numpy(), "dw": g[i] * r["dw"],
                    "db": g[i] * r["db"]}, {k: g[i] * r[k] for k in ("loss", "per", "dE", "dw", "db")}, f"stack batch {i}")

    # dtypes: bf16 in, bf16 out (computed in fp32 behind differentiable casts); fp64 is not silently cast down
    eb = torch.as_tensor(E, device=dev).bfloat16().requires_grad_(True)
    mod = GE2ELoss(HParams(DEV))
    lb = mod(eb, labels=host)
    lb.backward()
    assert lb.dtype == torch.bfloat16 and eb.grad.dtype == torch.bfloat16 and mod.w.grad.dtype == torch.float32
    l32 = GF.ge2e_loss_labeled(eb.detach().float(), host, w.detach(), b.detach())
    assert torch.equal(lb.detach(), l32.to(torch.bfloat16)) and bool(torch.isfinite(eb.grad).all())
    with pytest.raises(NotImplementedError, match="float64"):
        mod(torch.as_tensor(E, device=dev).double(), labels=host)
    with pytest.raises(NotImplementedError, match="float64"):
        GF.ge2e_loss_labeled(torch.as_tensor(E, device=dev).double(), host, w.detach(), b.detach())
    # what is refused before anything is launched
    ef = torch.as_tensor(E, device=dev)
    with pytest.raises(ValueError, match="not both"):
        mod(ef, counts=counts, labels=host)
    with pytest.raises(ValueError, match="num_speakers"):
        mod(ef, labels=torch.as_tensor(lab, device=dev))
    with pytest.raises(ValueError, match="distinct speakers"):
        mod(ef, labels=host, num_speakers=N + 1)
    with pytest.raises(ValueError, match="at least 2"):
        mod(ef, labels=[123] + host[1:])
    with pytest.raises(ValueError, match="integers"):
        mod(ef, labels=[float(x) for x in host])
    with pytest.raises(TypeError, match="int32 or torch.int64"):
        mod(ef, labels=torch.as_tensor(lab, device=dev).float(), num_speakers=N)
    with pytest.raises(RuntimeError):
        GF.ge2e_loss_labeled(torch.as_tensor(E), host, w.detach(), b.detach())        # embeddings on the host
