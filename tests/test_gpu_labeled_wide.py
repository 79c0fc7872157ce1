"""GPU: the labelled loss's wide route (ge2e_loss_fwd_bwd_labeled_wide, functional.loss_fwd_bwd_labeled(wide=True),
functional.ge2e_loss_labeled(wide=True), GE2ELoss(...)(e, labels=..., wide=True)): the masked labelled loss as a chain of
many-workgroup kernels.

Reference, never the code under test: tests/masked_ref.py -- numpy for the index tables, torch autograd in float64 for the
loss on the rows that count, zeros on every other row.  The C-ABI tests call through ctypes on the guarded buffers of
tests/guarded.py: inputs between NaN / sentinel guards, outputs poisoned, the workspace exactly
ge2e_workspace_bytes_labeled_wide bytes between guard bands, filled with 0xFF bytes in one run and 0x00 in another (the two
must agree bit for bit), every guard intact afterwards, inputs unmodified.

Gate: rowlist_harness.check_rows, unchanged.  The agreement with ge2e_loss_fwd_bwd_labeled_masked on the same inputs is held to
factor=2 (two fp32 results are compared); a batch in which nothing counts is held to exact zeros.  Inputs:
rowlist_cases.inputs (unit rows centre[label] + 0.5 noise, seeded), w = 10, b = -5.  Every seeded draw is checked on the
numpy reference, before anything is launched, to hold what its case is named for.  `-s` prints every figure before it is
asserted.
"""
import functools

import numpy as np
import pytest
import torch

from capi import GF, lib  # noqa: F401
from rowlist_cases import LOSS_CASES, draw, inputs, loss_case, mixed_draw, reference
from rowlist_harness import BIAS, DEV, KEYS, VARIANTS, W, batch_of, check_masked, check_rows, poisoned, run_masked, same_bits
from rowlist_harness import run_wide as run

pytestmark = pytest.mark.gpu


def whole_check(lib, E, labels, N, variant, ref, what, against_masked=True, noper=False):
    """What every case is held to.  One batch E (R, D), labels (R,): the call with a gradient against the fp64 reference and
    -- NaN / Inf on the rows that do not count -- with the same bits; forward only: the bits of loss and per; the parent's
    masked entry within factor=2; `noper`: the same bits without per and active."""
    idx = ref["index"]
    bad = poisoned(E, idx)
    full = run(lib, E[None], labels[None], N, variant, True, 0xFF)
    check_masked(batch_of(full, 0), ref, what)
    nan = run(lib, bad[None], labels[None], N, variant, True, 0x00)
    for k in full:
        assert same_bits(nan[k], full[k]), f"{what}: {k} depends on a row that does not count, or on the workspace"
    fwd = run(lib, bad[None], labels[None], N, variant, False, 0xFF)
    assert set(fwd) == {"loss", "per", "active"}
    for k in fwd:
        assert same_bits(fwd[k], full[k]), f"{what}: forward-only {k} differs"
    if noper:
        bare = run(lib, E[None], labels[None], N, variant, True, 0xFF, want_per=False, want_active=False)
        assert set(bare) == {"loss", "dE", "dw", "db"}
        for k in bare:
            assert same_bits(bare[k], full[k]), f"{what}: {k} differs without per and active"
        bare = run(lib, E[None], labels[None], N, variant, False, 0xFF, want_per=False, want_active=False)
        assert set(bare) == {"loss"} and same_bits(bare["loss"], full["loss"]), f"{what}: the loss alone differs"
    if against_masked:
        parent = run_masked(lib, E[None], labels[None], N, variant, True, 0xFF)
        assert np.array_equal(parent["active"], full["active"])
        if idx["active"][0] == 0:
            for k in KEYS:
                assert same_bits(parent[k], full[k]), f"{what}: {k} is not the masked entry's zero"
        else:
            check_rows({k: full[k][0] for k in KEYS}, {k: parent[k][0].astype(np.float64) for k in KEYS},
                       what + " vs the masked entry", factor=2)
    return full


# ---- 1. every case of the masked entry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_masked_cases(lib, name, variant):
    E, labels, N, ref = loss_case(name, variant)          # (the draw is checked there)
    what = f"{name}/{variant}"
    print(f"{what}: N {N} R {len(labels)} D {E.shape[1]} active {ref['index']['active'].tolist()}")
    whole_check(lib, E, labels, N, variant, ref, what, noper=True)


# ---- 2. the edges of the 64-row tiles -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_tile_case(r_act, variant):
    N, R, D = 12, 140, 16
    labels = draw(N, R, 7, 3, R - r_act - 3, 100 + r_act)
    E = inputs(labels, N, D, 9000 + r_act)
    ref = reference(E, labels, N, variant)
    assert ref["index"]["active"].tolist() == [7, r_act] and mixed_draw(ref["index"], N)
    return E, labels, N, ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("r_act", (63, 64, 65, 129))
def test_row_tile_edges(lib, r_act, variant):
    E, labels, N, ref = row_tile_case(r_act, variant)
    whole_check(lib, E, labels, N, variant, ref, f"r_act {r_act} in R 140/{variant}")


# ---- 3. the edges of the 16-speaker column tiles, and of the four the rows kernel keeps in flight --------------------------
@functools.lru_cache(maxsize=None)
def column_tile_case(n_act, variant):
    rng = np.random.default_rng(200 + n_act)
    N, D = n_act + 4, 8
    ids = rng.choice(N, size=n_act + 2, replace=False)
    counts = rng.integers(2, 4, n_act)
    labels = np.concatenate([np.repeat(ids[:n_act], counts), ids[n_act:], [-1, N, N + 7]])      # two lone speakers, three ignored rows
    labels = labels[rng.permutation(len(labels))].astype(np.int32)
    E = inputs(labels, N, D, 9100 + n_act)
    ref = reference(E, labels, N, variant)
    assert ref["index"]["active"].tolist() == [n_act, int(counts.sum())] and mixed_draw(ref["index"], N)
    assert set(counts.tolist()) == {2, 3}
    return E, labels, N, ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n_act", (15, 16, 17, 63, 64, 65, 70))
def test_column_tile_edges(lib, n_act, variant):
    E, labels, N, ref = column_tile_case(n_act, variant)
    whole_check(lib, E, labels, N, variant, ref, f"n_act {n_act}/{variant}")


# ---- 4. the embedding sizes: the rows kernel's instantiations, the D slabs, the unaligned stores ------------------------------
@functools.lru_cache(maxsize=None)
def embedding_case(D, variant):
    N, R = 9, 40
    labels = draw(N, R, 3, 2, 4, 31)
    E = inputs(labels, N, D, 9200 + D)
    ref = reference(E, labels, N, variant)
    assert mixed_draw(ref["index"], N) and ref["index"]["active"].tolist() == [3, 34]
    return E, labels, N, ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", (4, 64, 128, 256, 260, 37))
def test_embedding_sizes(lib, D, variant):
    E, labels, N, ref = embedding_case(D, variant)
    whole_check(lib, E, labels, N, variant, ref, f"D {D}/{variant}")


# ---- 5. a speaker that spans tiles next to speakers that share one ------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_speaker_that_spans_tiles(lib, variant):
    counts, D = (2, 70, 3, 2, 66, 2), 32
    N, R = len(counts), sum(counts)
    labels = np.repeat(np.arange(N), counts)[np.random.default_rng(5).permutation(R)].astype(np.int32)
    E = inputs(labels, N, D, 9300)
    ref = reference(E, labels, N, variant)
    idx = ref["index"]
    assert idx["active"].tolist() == [N, R] and idx["counts"].tolist() == list(counts)
    # speaker 1 covers positions 2 .. 71 and speaker 4 positions 77 .. 142: both cross a multiple of 64
    assert idx["offsets"][1] < 64 < idx["offsets"][2] and idx["offsets"][4] < 128 < idx["offsets"][5]
    whole_check(lib, E, labels, N, variant, ref, f"counts {counts}/{variant}", noper=True)


# ---- 6. a stack: launch to launch, position in the stack, what the workspace held ---------------------------------------------
def stack_check(lib, E, labels, N, variant, refs, what):
    B = len(E)
    a = run(lib, E, labels, N, variant, True, 0xFF)
    for i in range(B):
        check_masked(batch_of(a, i), refs[i], f"{what} batch {i} active {refs[i]['index']['active'].tolist()}", quiet=i > 2)
    again = run(lib, E, labels, N, variant, True, 0xFF)
    zero = run(lib, E, labels, N, variant, True, 0x00)
    flipped = run(lib, E[::-1], labels[::-1], N, variant, True, 0xFF)
    for k in a:
        assert same_bits(a[k], again[k]), f"{what} {k}: two launches differ"
        assert same_bits(a[k], zero[k]), f"{what} {k} depends on what the workspace held before the call"
        for i in range(B):
            assert same_bits(a[k][i], flipped[k][B - 1 - i]), f"{what} {k}: batch {i} depends on its position in the stack"
    fwd = run(lib, E, labels, N, variant, False, 0x00)
    for k in fwd:
        assert same_bits(fwd[k], a[k]), f"{what}: forward-only {k} differs"


@pytest.mark.parametrize("variant", VARIANTS)
def test_stack_of_37(lib, variant):
    B, N, R, D = 37, 12, 48, 20
    labels = np.stack([draw(N, R, 2 + i % 5, 1 + i % 4, 5 + i % 9, 300 + i) for i in range(B)])
    labels[11] = np.where(np.arange(R) % 2 == 0, np.arange(R) // 2 % N, -1 - np.arange(R))   # 24 valid rows: 12 speakers twice each
    labels[23] = np.concatenate([np.arange(N), np.full(R - N, N + 1)])                        # lone speakers only: nothing counts
    E = np.stack([inputs(labels[i], N, D, 9400 + i) for i in range(B)])
    refs = [reference(E[i], labels[i], N, variant) for i in range(B)]
    acts = [r["index"]["active"].tolist() for r in refs]
    assert acts[23] == [0, 0] and acts[11] == [12, 24] and len({tuple(a) for a in acts}) >= 10
    assert all(mixed_draw(refs[i]["index"], N) for i in range(B) if i not in (11, 23))
    stack_check(lib, E, labels, N, variant, refs, f"B37/{variant}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_stack_where_gc_is_cut_into_pieces(lib, variant):
    """R = 300: the K loop of GC is cut into three pieces (one for every 128 rows of R), one of them short or empty."""
    B, N, R, D = 3, 20, 300, 12
    labels = np.stack([draw(N, R, 9, 3, 20, 401), draw(N, R, 4, 2, 150, 402), draw(N, R, 11, 5, 36, 403)])
    E = np.stack([inputs(labels[i], N, D, 9500 + i) for i in range(B)])
    refs = [reference(E[i], labels[i], N, variant) for i in range(B)]
    assert [r["index"]["active"].tolist() for r in refs] == [[9, 277], [4, 148], [11, 259]]
    assert all(mixed_draw(r["index"], N) for r in refs)
    stack_check(lib, E, labels, N, variant, refs, f"B3 R300/{variant}")


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    dev = torch.device(DEV)
    E, labels, N, ref = loss_case("nact17_of_N40_D36", "softmax")
    idx = ref["index"]
    R, D = E.shape

    def leaves():
        return (torch.as_tensor(E, device=dev).requires_grad_(True), torch.tensor(W, device=dev, requires_grad=True),
                torch.tensor(BIAS, device=dev, requires_grad=True))

    def grads(e, w, b, loss, per):
        return {"loss": loss.item(), "per": per, "dE": e.grad.cpu().numpy(), "dw": w.grad.item(), "db": b.grad.item()}

    lab32 = torch.as_tensor(labels, device=dev)
    # ge2e_loss_labeled(wide=True): loss.backward() against the fp64 reference, active against numpy
    e, w, b = leaves()
    loss, active = GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=N, wide=True, return_active=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert active.shape == (2,) and active.dtype == torch.int32 and not active.requires_grad
    assert active.tolist() == idx["active"].tolist()
    loss.backward()
    raw = GF.loss_fwd_bwd_labeled(e.detach(), lab32, w.detach(), b.detach(), num_speakers=N, need_per=True, wide=True)
    assert raw.per.shape == (1, R) and raw.dE.shape == (1, R, D) and raw.active.tolist() == [idx["active"].tolist()]
    assert torch.equal(raw.loss[0], loss.detach()) and torch.equal(raw.dE[0], e.grad)
    got = grads(e, w, b, loss, raw.per[0].cpu().numpy())
    check_masked(dict(got, active=active.cpu().numpy()), ref, "ge2e_loss_labeled(wide=True)")
    assert torch.equal(GF.ge2e_loss_labeled(e.detach(), lab32, w.detach(), b.detach(), num_speakers=N, wide=True, masked=True),
                       loss.detach())

    # what masked=True gives, at factor 2
    em, wm, bm = leaves()
    lm, am = GF.ge2e_loss_labeled(em, lab32, wm, bm, num_speakers=N, masked=True, return_active=True)
    lm.backward()
    rawm = GF.loss_fwd_bwd_labeled(em.detach(), lab32, wm.detach(), bm.detach(), num_speakers=N, need_per=True, masked=True)
    masked = {k: np.asarray(v, dtype=np.float64) for k, v in grads(em, wm, bm, lm, rawm.per[0].cpu().numpy()).items()}
    assert torch.equal(am, active)
    check_rows(got, masked, "wide vs masked=True", factor=2)

    # the module, with return_active
    mod = GE2ELoss(HParams(DEV))
    e1 = torch.as_tensor(E, device=dev).requires_grad_(True)
    l1, a1 = mod(e1, labels=lab32, num_speakers=N, wide=True, return_active=True)
    l1.backward()
    assert torch.equal(l1.detach(), loss.detach()) and torch.equal(a1, active) and torch.equal(e1.grad, e.grad)
    assert torch.equal(mod.w.grad, w.grad) and torch.equal(mod.b.grad, b.grad)
    check_masked(dict(grads(e1, mod.w, mod.b, l1, got["per"]), active=a1.cpu().numpy()), ref, "GE2ELoss(wide=True)")

    # int64 device labels: 2**32 + 3 is ignored, not wrapped onto speaker 3
    lab64 = torch.as_tensor(labels.astype(np.int64), device=dev)
    out_rows = torch.as_tensor(np.flatnonzero((labels < 0) | (labels >= N)), device=dev)
    assert len(out_rows) >= 2
    lab64[out_rows[0]] = 2 ** 32 + 3
    lab64[out_rows[1]] = -2 ** 40
    e2, w2, b2 = leaves()
    l2, a2 = GF.ge2e_loss_labeled(e2, lab64, w2, b2, num_speakers=N, wide=True, return_active=True)
    l2.backward()
    assert torch.equal(a2, active) and torch.equal(l2, loss) and torch.equal(e2.grad, e.grad)
    check_rows(grads(e2, w2, b2, l2, got["per"]), masked, "int64 labels vs masked=True", factor=2)

    # host labels with arbitrary ids, a lone speaker, negative ids on the rows to ignore
    ids = np.sort(np.random.default_rng(9).choice(10 ** 6, size=N, replace=False))
    host = np.where((labels >= 0) & (labels < N), ids[np.clip(labels, 0, N - 1)], -1 - np.arange(R)).tolist()
    e3, w3, b3 = leaves()
    l3, a3 = GF.ge2e_loss_labeled(e3, host, w3, b3, wide=True, return_active=True)
    l3.backward()
    assert torch.equal(a3, active)
    check_rows(grads(e3, w3, b3, l3, got["per"]), masked, "host labels vs masked=True", factor=2)
    check_masked(dict(grads(e3, w3, b3, l3, got["per"]), active=a3.cpu().numpy()), ref, "host labels")
    with pytest.raises(ValueError, match="masked=False"):
        GF.ge2e_loss_labeled(e3.detach(), host, w3.detach(), b3.detach(), wide=True, masked=False)
    with pytest.raises(ValueError, match="labels"):
        mod(e3.detach(), wide=True)


# ---- 8. one capture, replayed on other labels -----------------------------------------------------------------------------------
def test_graph_capture_replayed_with_other_labels(GF, lib):
    dev = torch.device(DEV)
    N, R, D = 12, 48, 20
    lab_a, lab_b = draw(N, R, 5, 6, 9, 2), draw(N, R, 3, 2, 20, 51)
    lab_none = np.concatenate([np.arange(N), np.full(R - N, -1)]).astype(np.int32)
    E = inputs(lab_a, N, D, 8000)
    refs = [reference(E, lab, N, "softmax") for lab in (lab_a, lab_b, lab_none)]
    assert mixed_draw(refs[0]["index"], N) and mixed_draw(refs[1]["index"], N)
    acts = [r["index"]["active"].tolist() for r in refs]
    assert acts[0] != acts[1] and acts[0][0] != acts[1][0] and acts[2] == [0, 0]
    e = torch.as_tensor(E, device=dev)[None].contiguous()
    lab = torch.zeros(1, R, dtype=torch.int32, device=dev)
    w, b = torch.tensor(W, device=dev), torch.tensor(BIAS, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731

    def outputs():
        return GF.LossOutputs(loss=nan(1), per=nan(1, R), dE=nan(1, R, D), dw=nan(1), db=nan(1),
                              active=torch.full((1, 2), -7, dtype=torch.int32, device=dev))

    out = outputs()
    ws = GF.alloc_workspace(lib.ge2e_workspace_bytes_labeled_wide(1, N, R, D, 0), dev, init=False)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        GF.loss_fwd_bwd_labeled(e, lab, w, b, num_speakers=N, wide=True, out=out, workspace=ws)      # (one speaker of 48 rows)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        GF.loss_fwd_bwd_labeled(e, lab, w, b, num_speakers=N, wide=True, out=out, workspace=ws)
    for labels, ref in zip((lab_a, lab_b, lab_none, lab_a), refs + refs[:1]):
        lab.copy_(torch.as_tensor(labels, device=dev)[None])
        for t in (out.loss, out.per, out.dE, out.dw, out.db):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        o = {k: getattr(out, k)[0].cpu().numpy() for k in KEYS + ("active",)}
        what = f"replay with active {ref['index']['active'].tolist()}"
        assert all(np.isfinite(o[k]).all() for k in KEYS)
        check_masked(o, ref, what)
        eager = outputs()
        GF.loss_fwd_bwd_labeled(e, lab, w, b, num_speakers=N, wide=True, out=eager)
        torch.cuda.synchronize()
        for k in KEYS + ("active",):
            assert torch.equal(getattr(eager, k).view(torch.int32), getattr(out, k).view(torch.int32)), f"{what}: {k} is not the eager call's"
