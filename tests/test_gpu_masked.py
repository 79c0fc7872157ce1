"""GPU: the masked labelled loss (ge2e_label_index_masked, ge2e_loss_fwd_bwd_labeled_masked, functional.label_index_masked,
functional.ge2e_loss_labeled(masked=True), GE2ELoss(...)(e, labels=..., masked=True)): labels of any content, the rows and
speakers that count decided on the device.

References, never the code under test: tests/masked_ref.py -- numpy for the index kernel (exact integer equality of offsets,
order, speakers and active), tests/ragged_ref.py (torch autograd in float64) on the rows that count for the loss, zeros on
every other row.  The C-ABI tests call through ctypes on the guarded buffers of tests/guarded.py: inputs between NaN /
sentinel guards, outputs poisoned, the workspace exactly ge2e_workspace_bytes_labeled_masked
(ge2e_label_index_masked_workspace_bytes) bytes between guard bands, filled with 0xFF bytes in one run and 0x00 in another
(the two must agree bit for bit), every guard intact afterwards, inputs unmodified.

Gate: rowlist_harness.check_rows, unchanged: the arithmetic is the same kernel's.  A batch in which nothing counts is held to
exact zeros.  Inputs: unit rows centre[label] + 0.5 noise, seeded (rows that are ignored get a centre of their own);
w = 10, b = -5.  Every seeded random draw is checked on the numpy reference, before anything is launched, to hold at least
2 active speakers, a lone speaker, an absent speaker and an ignored row.  `-s` prints every figure before it is asserted.
"""
import numpy as np
import pytest
import torch

import masked_ref as mr
from capi import GF, lib  # noqa: F401
from rowlist_cases import INDEX_CASES, LOSS_CASES, RANDOM_INDEX_CASES, draw, inputs, loss_case, mixed_draw
from rowlist_harness import (BIAS, DEV, KEYS, VARIANTS, W, batch_of, check_masked, ragged_on_compacted, run_index, run_labeled,
                             same_bits)
from rowlist_harness import run_masked as run

pytestmark = pytest.mark.gpu


# ---- 1. the index kernel: exact integer equality with numpy ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_label_index_masked_is_the_numpy_reference(lib, name):
    N, labels = INDEX_CASES[name]
    labels = np.ascontiguousarray(labels).astype(np.int32)
    B, R = labels.shape
    ref = mr.index_ref_batched(labels, N)
    if name == "B3_own_nact_one_empty":
        assert sorted(ref["active"][:, 0].tolist()) == [0, 1, 3]
    if name == "N600_across_the_scan_rounds":
        assert ref["speakers"][0, :7].tolist() == [0, 255, 256, 511, 512, 599, -1]
    for row in ref["order"]:
        assert np.array_equal(np.sort(row), np.arange(R))
    # the seeded random draws hold every kind of row (B515: rows of 7, the stack as a whole does)
    kinds = [mixed_draw(dict(mr.index_ref(row, N), labels=row), N) for row in labels]
    for i in RANDOM_INDEX_CASES.get(name, ()):
        assert kinds[i], f"{name}: the draw of batch {i} does not hold every kind of row"
    if name == "B515_past_the_grid":
        hist = np.stack([np.bincount(row[(row >= 0) & (row < N)], minlength=N) for row in labels])
        assert (ref["active"][:, 0] >= 2).any() and (hist == 1).any() and (hist == 0).any() and (labels < 0).any() and (labels >= N).any()
    got = run_index(lib, labels, N, 0xFF, masked=True)
    print(f"{name}: B {B} N {N} R {R} active {ref['active'][:4].tolist()}: " +
          ", ".join(f"{k} differs at {int((got[k] != ref[k]).sum())}" for k in ref))
    for k in ref:
        assert np.array_equal(got[k], ref[k]), f"{name}: {k}"
    again = run_index(lib, labels, N, 0x00, masked=True)
    for k in ref:
        assert np.array_equal(got[k], again[k]), f"{name}: {k}: two launches differ"
    if B > 1:     # the batch at index i sits at index B-1-i of the flipped stack
        flipped = run_index(lib, labels[::-1], N, 0xFF, masked=True)
        for k in ref:
            assert np.array_equal(flipped[k][::-1], got[k]), f"{name}: {k}: a batch depends on its position"


# ---- 2. the loss against fp64, the rows that do not count, and the bits of the ragged entry ---------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_loss_cases(lib, name, variant):
    E, labels, N, ref = loss_case(name, variant)
    idx = ref["index"]
    what = f"{name}/{variant}"
    print(f"{what}: N {N} R {len(labels)} D {E.shape[1]} active {idx['active'].tolist()}")
    full = run(lib, E[None], labels[None], N, variant, True, 0xFF)
    zero = run(lib, E[None], labels[None], N, variant, True, 0x00)
    for k in full:
        assert same_bits(full[k], zero[k]), f"{what}: {k} depends on what the workspace held before the call"
    check_masked(batch_of(full, 0), ref, what)
    # forward only, without per, without active: the same bits of what is left
    fwd = run(lib, E[None], labels[None], N, variant, False, 0xFF)
    assert same_bits(fwd["loss"], full["loss"]) and same_bits(fwd["per"], full["per"]), f"{what}: forward-only differs"
    check_masked(batch_of(fwd, 0), ref, what + "/fwd")
    noper = run(lib, E[None], labels[None], N, variant, True, 0xFF, want_per=False, want_active=False)
    assert set(noper) == {"loss", "dE", "dw", "db"}
    for k in noper:
        assert same_bits(noper[k], full[k]), f"{what}: {k} differs without per and active"
    # the rows that do not count are never read: NaN there, the same bits
    poisoned = E.copy()
    poisoned[~idx["active_row"]] = np.nan
    assert np.isnan(poisoned).any()
    nan = run(lib, poisoned[None], labels[None], N, variant, True, 0xFF)
    for k in full:
        assert same_bits(nan[k], full[k]), f"{what}: {k} depends on a row that does not count"
    # the ragged entry on the compacted batch: the same bits
    if idx["active"][0] >= 1:
        want = ragged_on_compacted(lib, E, ref, variant)
        for k in KEYS:
            assert same_bits(full[k], want[k]), f"{what}: {k} is not the ragged entry's on the compacted batch"


@pytest.mark.parametrize("variant", VARIANTS)
def test_same_bits_as_the_labeled_entry_when_every_row_counts(lib, variant):
    rng = np.random.default_rng(7)
    for counts, D in (([2, 17, 3, 65, 2], 20), ([2, 3, 4], 5), ([5], 12)):
        N = len(counts)
        labels = np.repeat(np.arange(N), counts)[rng.permutation(sum(counts))].astype(np.int32)
        E = inputs(labels, N, D, 5000 + D)
        got = run(lib, E[None], labels[None], N, variant)
        assert got["active"].tolist() == [[N, sum(counts)]]
        want = run_labeled(lib, E[None], labels[None], N, variant)
        for k in KEYS:
            assert same_bits(got[k], want[k]), f"{counts}/{variant}: {k}"


# ---- 3. B > 1: every batch its own extents, more batches than workgroups, position independence ------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_batches_with_their_own_extents(lib, variant):
    N, R, D = 9, 40, 24
    labels = np.ascontiguousarray(INDEX_CASES["B3_own_nact_one_empty"][1]).astype(np.int32)
    E = np.stack([inputs(labels[i], N, D, 6000 + i) for i in range(3)])
    refs = [mr.masked_loss(E[i], labels[i], N, W, BIAS, variant=variant) for i in range(3)]
    assert sorted(int(r["index"]["active"][0]) for r in refs) == [0, 1, 3]
    a = run(lib, E, labels, N, variant, True, 0xFF)
    again = run(lib, E, labels, N, variant, True, 0x00)
    flipped = run(lib, E[::-1], labels[::-1], N, variant, True, 0xFF)
    for i in range(3):
        check_masked(batch_of(a, i), refs[i], f"B3 batch {i} active {refs[i]['index']['active'].tolist()} {variant}")
    for k in a:
        assert same_bits(a[k], again[k]), f"{variant} {k}: two launches differ"
        for i in range(3):
            assert same_bits(a[k][i], flipped[k][2 - i]), f"{variant} {k}: batch {i} depends on its position in the launch"


def test_position_independence_in_a_stack_of_601(lib):
    """One batch at positions 0 and 600 of a stack of mixed batches (more batches than workgroups: one is a workgroup's
    first batch, the other a workgroup's second): the same bits at both."""
    B, N, R, D = 601, 6, 14, 4
    rng = np.random.default_rng(8)
    labels = rng.integers(-1, N + 1, (B, R)).astype(np.int32)
    labels[5] = N                                   # a batch in which nothing counts
    labels[0] = draw(N, R, 2, 2, 3, 41)
    labels[600] = labels[0]
    E = np.stack([inputs(labels[i], N, D, 7000 + i) for i in range(B)])
    E[600] = E[0]
    ref0 = mr.masked_loss(E[0], labels[0], N, W, BIAS)
    ref0["index"]["labels"] = labels[0]
    assert mixed_draw(ref0["index"], N)
    n_acts = {int(mr.index_ref(labels[i], N)["active"][0]) for i in range(B)}
    assert 0 in n_acts and len(n_acts) >= 3, n_acts
    o = run(lib, E, labels, N, "softmax", True, 0xFF)
    for k in o:
        assert np.array_equal(o[k][0].view(np.uint32), o[k][600].view(np.uint32)), f"{k}: position 0 and 600 differ"
    for i in (0, 5, 99, 300, 511, 512, 600):
        check_masked(batch_of(o, i), mr.masked_loss(E[i], labels[i], N, W, BIAS), f"B601 batch {i}")
    ind = run_index(lib, labels, N, masked=True)
    for k in ind:
        assert np.array_equal(ind[k][0], ind[k][600]), f"index {k}: position 0 and 600 differ"
    assert np.array_equal(ind["active"], o["active"])


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    dev = torch.device(DEV)
    E, labels, N, ref = loss_case("nact17_of_N40_D36", "softmax")
    idx = ref["index"]
    R, D = E.shape

    def leaves():
        return (torch.as_tensor(E, device=dev).requires_grad_(True), torch.tensor(W, device=dev, requires_grad=True),
                torch.tensor(BIAS, device=dev, requires_grad=True))

    half = {k: 0.5 * ref[k] for k in KEYS}
    half["index"] = idx
    # device labels, int32: (0.5 * loss).backward() against 0.5 x the reference; active against numpy
    e, w, b = leaves()
    lab32 = torch.as_tensor(labels, device=dev)
    loss, active = GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=N, masked=True, return_active=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert active.shape == (2,) and active.dtype == torch.int32 and active.is_cuda and not active.requires_grad
    assert active.tolist() == idx["active"].tolist()
    (0.5 * loss).backward()
    raw = GF.loss_fwd_bwd_labeled(e.detach(), lab32, w.detach(), b.detach(), num_speakers=N, need_per=True, masked=True)
    assert raw.per.shape == (1, R) and raw.dE.shape == (1, R, D) and raw.active.tolist() == [idx["active"].tolist()]
    assert torch.equal(raw.loss[0], loss.detach())
    check_masked({"loss": 0.5 * loss.item(), "per": 0.5 * raw.per[0].cpu().numpy(), "dE": e.grad.cpu().numpy(),
                  "dw": w.grad.item(), "db": b.grad.item()}, half, "0.5 * ge2e_loss_labeled(masked)")
    mean = loss.detach() / active[..., 1].clamp(min=1)                         # the mean over the rows that counted, no sync
    assert abs(mean.item() - ref["loss"] / idx["active"][1]) <= 1e-5 * abs(ref["loss"] / idx["active"][1])
    assert torch.equal(GF.ge2e_loss_labeled(e.detach(), lab32, w.detach(), b.detach(), num_speakers=N, masked=True), loss.detach())

    # int64 device labels: 2**32 + 3 is ignored, not wrapped onto speaker 3; so is anything else outside the bound
    lab64 = torch.as_tensor(labels.astype(np.int64), device=dev)
    out_rows = torch.as_tensor(np.flatnonzero((labels < 0) | (labels >= N)), device=dev)
    assert len(out_rows) >= 3
    lab64[out_rows[0]] = 2 ** 32 + 3
    lab64[out_rows[1]] = -2 ** 40
    lab64[out_rows[2]] = 2 ** 31 + int(idx["speakers"][0])
    e2, w2, b2 = leaves()
    loss2, active2 = GF.ge2e_loss_labeled(e2, lab64, w2, b2, num_speakers=N, masked=True, return_active=True)
    (0.5 * loss2).backward()
    assert torch.equal(loss2, loss) and torch.equal(active2, active) and torch.equal(e2.grad, e.grad)
    assert torch.equal(w2.grad, w.grad) and torch.equal(b2.grad, b.grad)

    # label_index_masked: what the loss reads
    got = GF.label_index_masked(lab64, N)
    for t, k in zip(got, ("offsets", "order", "speakers", "active")):
        assert t.dtype == torch.int32 and t.is_cuda and np.array_equal(t.cpu().numpy(), idx[k]), k
    got = GF.label_index_masked(torch.stack([lab32, lab32.flip(0)]), N)
    flipped = mr.index_ref(labels[::-1], N)
    assert got[1].shape == (2, R) and np.array_equal(got[1][1].cpu().numpy(), flipped["order"])
    assert got[3].tolist() == [idx["active"].tolist()] * 2

    # host labels: arbitrary ids, a lone speaker, negative ids on the rows to ignore
    ids = np.sort(np.random.default_rng(9).choice(10 ** 6, size=N, replace=False))
    host = np.where((labels >= 0) & (labels < N), ids[np.clip(labels, 0, N - 1)], -1 - np.arange(R)).tolist()
    e3, w3, b3 = leaves()
    loss3, active3 = GF.ge2e_loss_labeled(e3, host, w3, b3, masked=True, return_active=True)
    (0.5 * loss3).backward()
    assert torch.equal(loss3, loss) and torch.equal(active3, active) and torch.equal(e3.grad, e.grad)
    n_up = len(GF._label_uploads)
    assert torch.equal(GF.ge2e_loss_labeled(e3.detach(), host, w3.detach(), b3.detach(), masked=True), loss.detach())
    assert len(GF._label_uploads) == n_up                                       # a repeated host table is not uploaded again
    with pytest.raises(ValueError, match="at least 2"):                         # without masking the lone speaker is refused
        GF.ge2e_loss_labeled(e3.detach(), host, w3.detach(), b3.detach())
    with pytest.raises(ValueError, match="bound"):
        GF.ge2e_loss_labeled(e3.detach(), host, w3.detach(), b3.detach(), num_speakers=3, masked=True)

    # the module, eager and with graph=True (eager too: nothing captured)
    for graph in (False, True):
        mod = GE2ELoss(HParams(DEV), graph=graph)
        for _ in range(3 if graph else 1):
            em = torch.as_tensor(E, device=dev).requires_grad_(True)
            mod.zero_grad(set_to_none=True)
            lm, am = mod(em, labels=lab32, num_speakers=N, masked=True, return_active=True)
            (0.5 * lm).backward()
            assert torch.equal(lm.detach(), loss.detach()) and torch.equal(am, active) and torch.equal(em.grad, e.grad)
            assert torch.equal(mod.w.grad, w.grad) and torch.equal(mod.b.grad, b.grad)
        assert len(mod._steps) == 0
    mod = GE2ELoss(HParams(DEV))
    assert torch.equal(mod(torch.as_tensor(E, device=dev), labels=host, masked=True).detach(), loss.detach())

    # a (B, R, D) stack, one batch of it without anything that counts, and a vector of incoming gradients
    lab_b = np.ascontiguousarray(INDEX_CASES["B3_own_nact_one_empty"][1]).astype(np.int32)
    Eb = np.stack([inputs(lab_b[i], 9, 24, 6000 + i) for i in range(3)])
    es = torch.as_tensor(Eb, device=dev).requires_grad_(True)
    losses, act_b = mod(es, labels=torch.as_tensor(lab_b, device=dev), num_speakers=9, masked=True, return_active=True)
    assert losses.shape == (3,) and act_b.shape == (3, 2)
    g = [1.0, 2.0, -0.5]
    mod.zero_grad(set_to_none=True)
    (losses * torch.tensor(g, device=dev)).sum().backward()
    rs = [mr.masked_loss(Eb[i], lab_b[i], 9, W, BIAS) for i in range(3)]
    # w.grad / b.grad: the sum over the batches, each within the gate's own bound for dw / db
    for grad, k, tol in ((mod.w.grad, "dw", lambda v: 2e-5 * abs(v) + 1e-5 + 1e-7 * 40), (mod.b.grad, "db", lambda v: 1e-4 + 3e-7 * 40)):
        want, bnd = sum(g[i] * float(rs[i][k]) for i in range(3)), sum(abs(g[i]) * tol(float(rs[i][k])) for i in range(3))
        print(f"stack {k}: {abs(grad.item() - want):.3e} / {bnd:.3e}")
        assert abs(grad.item() - want) <= bnd, f"stack {k}: {grad.item()} vs {want}"
    for i in range(3):
        r = rs[i]
        scaled = {k: g[i] * r[k] for k in KEYS}
        scaled["index"] = r["index"]
        check_masked({"loss": g[i] * losses[i].item(), "per": g[i] * r["per"].astype(np.float32),
                      "dE": es.grad[i].cpu().numpy(), "dw": g[i] * r["dw"], "db": g[i] * r["db"],
                      "active": act_b[i].cpu().numpy()}, scaled, f"stack batch {i}", plus=False)

    # bf16 in, bf16 out; fp64 is not silently cast down; what is refused before anything is launched
    eb = torch.as_tensor(E, device=dev).bfloat16().requires_grad_(True)
    lb = mod(eb, labels=lab32, num_speakers=N, masked=True)
    lb.backward()
    assert lb.dtype == torch.bfloat16 and eb.grad.dtype == torch.bfloat16 and bool(torch.isfinite(eb.grad).all())
    assert not eb.grad[torch.as_tensor(~idx["active_row"], device=dev)].any()
    ef = torch.as_tensor(E, device=dev)
    with pytest.raises(NotImplementedError, match="float64"):
        mod(ef.double(), labels=lab32, num_speakers=N, masked=True)
    with pytest.raises(ValueError, match="num_speakers"):
        mod(ef, labels=lab32, masked=True)
    with pytest.raises(ValueError, match="labels"):
        mod(ef, masked=True)
    with pytest.raises(ValueError, match="return_active"):
        mod(ef, labels=lab32, num_speakers=N, return_active=True)


# ---- 5. one capture, replayed on other labels -----------------------------------------------------------------------------------
def test_graph_capture_replayed_with_other_labels(GF, lib):
    dev = torch.device(DEV)
    N, R, D = 12, 48, 20
    lab_a, lab_b = draw(N, R, 5, 6, 9, 2), draw(N, R, 3, 2, 20, 51)
    E = inputs(lab_a, N, D, 8000)
    refs = [mr.masked_loss(E, lab, N, W, BIAS) for lab in (lab_a, lab_b)]
    for lab, ref in zip((lab_a, lab_b), refs):
        ref["index"]["labels"] = lab
        assert mixed_draw(ref["index"], N)
    assert refs[0]["index"]["active"].tolist() != refs[1]["index"]["active"].tolist()
    e = torch.as_tensor(E, device=dev)[None].contiguous()
    lab = torch.zeros(1, R, dtype=torch.int32, device=dev)
    w, b = torch.tensor(W, device=dev), torch.tensor(BIAS, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    out = GF.LossOutputs(loss=nan(1), per=nan(1, R), dE=nan(1, R, D), dw=nan(1), db=nan(1),
                         active=torch.full((1, 2), -7, dtype=torch.int32, device=dev))
    ws = GF.alloc_workspace(lib.ge2e_workspace_bytes_labeled_masked(1, N, R, D, 0), dev, init=False)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        GF.loss_fwd_bwd_labeled(e, lab, w, b, num_speakers=N, masked=True, out=out, workspace=ws)      # (nothing counts yet)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        GF.loss_fwd_bwd_labeled(e, lab, w, b, num_speakers=N, masked=True, out=out, workspace=ws)
    for labels, ref in zip((lab_a, lab_b), refs):
        lab.copy_(torch.as_tensor(labels, device=dev)[None])
        for t in (out.loss, out.per, out.dE, out.dw, out.db):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        o = {k: getattr(out, k)[0].cpu().numpy() for k in KEYS + ("active",)}
        assert all(np.isfinite(o[k]).all() for k in KEYS)
        check_masked(o, ref, f"replay with active {ref['index']['active'].tolist()}")
