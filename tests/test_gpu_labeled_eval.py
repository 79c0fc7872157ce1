"""GPU: labelled evaluation (ge2e_cos_sim_labeled, ge2e_eer_counts_labeled, functional.cos_sim_labeled /
eer_counts_labeled, evaluation.evaluate_labeled): cosines and EER counts for rows in any order, one label per row.

Reference, never the code under test: tests/labeled_eval_ref.py (numpy float64 on tests/masked_ref.index_ref).  The C-ABI
tests call through ctypes on the guarded buffers of tests/guarded.py: inputs between guards, outputs poisoned, the workspace
exactly ge2e_cos_sim_labeled_workspace_bytes between guard bands, filled with 0xFF bytes in one run and 0x00 in another (the
two must agree bit for bit), guards intact and inputs unmodified afterwards.

Gates: max|cos - ref| <= 3e-6 on the entries that count -- the project's bound for exact-fp32 cosines
(tests/test_gpu_helpers.py; the fp32 MFMA's documented error is 1.5e-7 x sum|a b|, and that sum is <= 1 for unit operands)
-- exact +0.0 everywhere else; col, speakers, active equal to the numpy index reference; counts exact.  Counts are compared
with the float64 reference only for inputs whose reference cosines keep at least 1.2e-5 (four times the gate) from every
threshold; each such test asserts that margin before anything is launched.  `-s` prints every figure before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

import labeled_eval_ref as ler
from capi import GF, lib  # noqa: F401
from conftest import golden_names, load_golden
from rowlist_cases import EDGE_CASES, INDEX_CASES, draw, edge_case, host_ids, inputs
from rowlist_cases import cos_reference as reference
from rowlist_harness import DEV, batch_of, run_counts, same_bits
from rowlist_harness import run_cos as run

pytestmark = pytest.mark.gpu

GATE = 3e-6
MARGIN = 4 * GATE
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "callers", "eer.npz"))
EER_CASES = sorted({k.split(".")[0] for k in Z.files})


def thresholds_of(kind):
    from speaker_embedding_ge2e_loss_amd.evaluation import THRESHOLDS
    if kind == "reference":
        return np.asarray(THRESHOLDS, dtype=np.float64)
    # "seeded33": 33 entries, one value twice.  The seed was chosen on the CPU for the float64 reference of MARGIN_CASES:
    # its cosines stay 3.8e-5 and 4.0e-5 away from every entry (test_fused_counts asserts >= 1.2e-5 before it launches)
    t = np.sort(np.random.default_rng(30).uniform(-0.2, 1.0, 32))
    return np.sort(np.concatenate([t, t[11:12]]))


def check(o, ref, what):
    """One batch against the reference: the gate of the module docstring."""
    for k in ("col", "speakers", "active"):
        if k in o:
            assert np.array_equal(o[k], ref[k]), f"{what}: {k}"
    if "cos" in o:
        n_act = int(ref["active"][0])
        counted = np.zeros(ref["cos"].shape, dtype=bool)
        counted[ref["col"] >= 0, :n_act] = True
        err = float(np.abs(o["cos"][counted] - ref["cos"][counted]).max()) if counted.any() else 0.0
        print(f"{what}: active {ref['active'].tolist()} max|cos - ref| {err:.2e} / {GATE:.0e}")
        assert err <= GATE, f"{what}: max|cos - ref| = {err:.3e}"
        rest = o["cos"][~counted]
        assert not rest.any() and not np.signbit(rest).any(), f"{what}: cos is not +0 where nothing counts"


def counts_of(cos, col, active, thr):
    """numpy's `>` on a call's own fp32 cos, per batch."""
    return np.stack([ler.counts_ref(cos[i], col[i], active[i][0], thr) for i in range(len(cos))])


# ---- 1. edge shapes, with the rows that do not count (3.) and the fused counts on the call's own cos ----------------------------
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_shapes(lib, name):
    E, labels, N, ref = edge_case(name)
    thr = thresholds_of("reference")
    full = run(lib, E[None], labels[None], N, thr, True, 0xFF)
    zero = run(lib, E[None], labels[None], N, thr, True, 0x00)
    for k in full:
        assert same_bits(full[k], zero[k]), f"{name}: {k} depends on what the workspace held before the call"
    check(batch_of(full, 0), ref, name)
    want = counts_of(full["cos"], full["col"], full["active"], thr)
    assert np.array_equal(full["counts"], want), f"{name}: the fused counts are not numpy's on the call's own cos"
    # cos alone, without the index outputs; counts alone: the same bits of what is left
    alone = run(lib, E[None], labels[None], N, None, True, 0xFF, want_index=False)
    assert set(alone) == {"cos"} and same_bits(alone["cos"], full["cos"]), f"{name}: cos differs without counts"
    nocos = run(lib, E[None], labels[None], N, thr, False, 0xFF)
    assert "cos" not in nocos and all(np.array_equal(nocos[k], full[k]) for k in nocos), f"{name}: without cos"
    # the rows that do not count are never read: NaN there, the same bits
    poisoned = E.copy()
    poisoned[ref["col"] < 0] = np.nan
    if (ref["col"] < 0).any():
        nan = run(lib, poisoned[None], labels[None], N, thr, True, 0xFF)
        for k in full:
            assert same_bits(nan[k], full[k]), f"{name}: {k} depends on a row that does not count"
    # ge2e_eer_counts_labeled on that cos: the same counts
    again = run_counts(lib, full["cos"], full["col"], full["active"], thr)
    assert np.array_equal(again, full["counts"]), f"{name}: ge2e_eer_counts_labeled differs from the fused counts"


# ---- 2. batches ----------------------------------------------------------------------------------------------------------------
def test_batches_with_their_own_labels(lib):
    N, D = 9, 24
    labels = np.ascontiguousarray(INDEX_CASES["B3_own_nact_one_empty"][1]).astype(np.int32)
    E = np.stack([inputs(labels[i], N, D, 6000 + i) for i in range(3)])
    refs = [reference(E[i], labels[i], N) for i in range(3)]
    assert sorted(int(r["active"][0]) for r in refs) == [0, 1, 3]
    thr = thresholds_of("seeded33")
    a = run(lib, E, labels, N, thr, True, 0xFF)
    again = run(lib, E, labels, N, thr, True, 0x00)
    flipped = run(lib, E[::-1], labels[::-1], N, thr, True, 0xFF)
    for i in range(3):
        check(batch_of(a, i), refs[i], f"B3 batch {i}")
    assert np.array_equal(a["counts"], counts_of(a["cos"], a["col"], a["active"], thr))
    for k in a:
        assert same_bits(a[k], again[k]), f"{k}: two launches differ"
        for i in range(3):
            assert same_bits(a[k][i], flipped[k][2 - i]), f"{k}: batch {i} depends on its position in the launch"


def test_stack_of_601(lib):
    B, N, R, D = 601, 4, 8, 8
    rng = np.random.default_rng(8)
    labels = rng.integers(-1, N + 1, (B, R)).astype(np.int32)
    labels[5] = N                                   # a batch in which nothing counts
    labels[600] = labels[0]
    E = np.stack([inputs(labels[i], N, D, 7000 + i) for i in range(B)])
    E[600] = E[0]
    thr = thresholds_of("reference")
    o = run(lib, E, labels, N, thr, True, 0xFF)
    n_acts = set()
    for i in range(B):
        ref = reference(E[i], labels[i], N)
        n_acts.add(int(ref["active"][0]))
        for k in ("col", "speakers", "active"):
            assert np.array_equal(o[k][i], ref[k]), f"B601 batch {i}: {k}"
        if i in (0, 5, 99, 300, 511, 512, 600):
            check(batch_of(o, i), ref, f"B601 batch {i}")
    assert 0 in n_acts and len(n_acts) >= 3, n_acts
    for k in o:
        assert same_bits(o[k][0], o[k][600]), f"{k}: position 0 and 600 differ"
    assert np.array_equal(o["counts"], counts_of(o["cos"], o["col"], o["active"], thr))


# ---- 4. order invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nact17_of_N40_D36", "nact67_of_2_rows_D36"])
def test_rows_permuted_with_every_speakers_order_kept(lib, name):
    E, labels, N, _ = edge_case(name)
    R = len(labels)
    rng = np.random.default_rng(44)
    new_labels = labels[rng.permutation(R)]
    src = np.empty(R, dtype=np.int64)               # new row i is old row src[i]: the rows of one label keep their order
    for v in np.unique(labels):
        src[np.flatnonzero(new_labels == v)] = np.flatnonzero(labels == v)
    assert np.array_equal(labels[src], new_labels) and not np.array_equal(src, np.arange(R))
    a = run(lib, E[None], labels[None], N, None, True)
    b = run(lib, E[src][None], new_labels[None], N, None, True)
    assert same_bits(b["cos"][0], a["cos"][0][src]), f"{name}: a row's bits depend on where the other rows stand"
    assert np.array_equal(b["col"][0], a["col"][0][src]) and np.array_equal(b["speakers"], a["speakers"])


# ---- 5. the fused counts against the float64 reference ------------------------------------------------------------------------
MARGIN_CASES = {
    # name: (labels, N, D, input seed, margin to the reference thresholds found on the CPU when the case was chosen)
    "N40_R75_D36": (draw(40, 75, 17, 4, 5, seed=2), 40, 36, 7002, 4.9e-5),
    "N1251_R80_D16": (draw(1251, 80, 23, 9, 6, seed=1), 1251, 16, 7001, 2.6e-5),
}


@pytest.mark.parametrize("table", ["reference", "seeded33"])
@pytest.mark.parametrize("name", list(MARGIN_CASES))
def test_fused_counts(lib, name, table):
    labels, N, D, seed, _ = MARGIN_CASES[name]
    E = inputs(labels, N, D, seed)
    ref = reference(E, labels, N)
    thr = thresholds_of(table)
    assert len(thr) == (50 if table == "reference" else 33) and (table == "reference" or (np.diff(thr) == 0).sum() == 1)
    m = ler.margin(ref["cos"], ref["col"], ref["active"][0], thr)
    want64 = ler.counts_ref(ref["cos"], ref["col"], ref["active"][0], thr)
    print(f"{name}/{table}: margin {m:.2e} (needs {MARGIN:.1e}); false accepts at the first threshold {want64[0, 0]}")
    assert m >= MARGIN, f"{name}/{table}: a reference cosine is {m:.2e} from a threshold"
    if name == "N1251_R80_D16" and table == "reference":
        assert want64[0, 0] > 0                                    # the false-accept column is exercised
    full = run(lib, E[None], labels[None], N, thr, True)
    check(batch_of(full, 0), ref, f"{name}/{table}")
    assert np.array_equal(full["counts"], counts_of(full["cos"], full["col"], full["active"], thr))
    assert np.array_equal(full["counts"], run_counts(lib, full["cos"], full["col"], full["active"], thr))
    nocos = run(lib, E[None], labels[None], N, thr, False)
    assert np.array_equal(nocos["counts"], full["counts"]), f"{name}/{table}: counts differ without cos"
    assert np.array_equal(full["counts"][0], want64), f"{name}/{table}: counts differ from the float64 reference's"


# ---- 6. ge2e_eer_counts_labeled on a sim of the test's own ----------------------------------------------------------------------
@pytest.mark.parametrize("T", [33, 1, 4096])
def test_eer_counts_labeled_alone(lib, T):
    B, N, R, n_act = 5, 7, 29, 5
    rng = np.random.default_rng(600 + T)
    if T == 33:
        thr = thresholds_of("seeded33")
    else:
        thr = np.sort(rng.choice(rng.uniform(-0.2, 1.0, max(1, T // 2)), size=T))     # (T = 4096: many repeated values)
    thr32 = thr.astype(np.float32)
    sim = rng.uniform(-0.3, 1.1, (B, R, N)).astype(np.float32)
    col = rng.integers(-1, n_act, (B, R)).astype(np.int32)
    col[3] = -1                                                    # a batch without a row that counts
    hit = rng.random(sim.shape)
    sim[hit < 0.15] = rng.choice(thr32, size=int((hit < 0.15).sum()))   # values equal to a threshold: `>` is strict
    sim[(hit >= 0.15) & (hit < 0.2)] = np.nan
    sim[(hit >= 0.2) & (hit < 0.25)] = np.inf
    wild = np.where(rng.random((B, R, N)) < 0.5, np.nan, np.inf).astype(np.float32)
    sim[:, :, n_act:] = wild[:, :, n_act:]                         # must not be counted: the columns >= n_act ...
    sim[col < 0] = wild[col < 0]                                   # ... and the rows with col = -1
    active = np.stack([[n_act, int((col[i] >= 0).sum())] for i in range(B)]).astype(np.int32)
    want = np.stack([ler.counts_ref(sim[i], col[i], n_act, thr) for i in range(B)])
    assert (want[3] == 0).all() and want[0, 0, 0] > 0 and want[0, 0, 1] > 0
    got = run_counts(lib, sim, col, active, thr)
    assert np.array_equal(got, want), f"T {T}: differs at {int((got != want).sum())} of {want.size}"
    assert np.array_equal(run_counts(lib, sim, col, active, thr), got)


# ---- 7. equal counts against the existing fixtures ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", EER_CASES)
def test_eer_fixtures(lib, GF, name):
    from speaker_embedding_ge2e_loss_amd.evaluation import THRESHOLDS
    Eg, S = Z[name + ".E"], Z[name + ".S"]
    N, M, D = Eg.shape
    R = N * M
    labels = np.repeat(np.arange(N), M).astype(np.int32)
    perm = np.random.default_rng(70).permutation(R)
    for what, rows in (("sorted", np.arange(R)), ("shuffled", perm)):
        o = run(lib, Eg.reshape(R, D)[rows][None], labels[rows][None], N, None, True)
        err = float(np.abs(o["cos"][0].astype(np.float64) - S.reshape(R, N)[rows]).max())
        print(f"{name}/{what}: max|cos - S| {err:.2e} / {GATE:.0e}")
        assert err <= GATE and np.array_equal(o["col"][0], labels[rows]) and o["active"].tolist() == [[N, R]]
        got = run_counts(lib, S.reshape(R, N)[rows][None], o["col"], o["active"], THRESHOLDS)
        assert np.array_equal(got[0], Z[name + ".counts"]), f"{name}/{what}: counts on the fixture's S"
    dense = GF.eer_counts(torch.as_tensor(S, device=DEV), THRESHOLDS).cpu().numpy()
    assert np.array_equal(got[0], dense), f"{name}: ge2e_eer_counts_labeled and ge2e_eer_counts differ on S"


@pytest.mark.parametrize("name", golden_names())
def test_golden_fixtures(lib, name):
    g = load_golden(name)
    N, M, D = g["E"].shape
    o = run(lib, g["E"].reshape(1, N * M, D), np.repeat(np.arange(N), M)[None], N, None, True)
    err = float(np.abs(o["cos"][0] - g["cos64"].reshape(N * M, N)).max())
    print(f"{name}: max|cos - cos64| {err:.2e} / {GATE:.0e}  (tests/test_gpu_parity.py holds every fixture's cosines to 3e-6)")
    assert err <= GATE and o["active"].tolist() == [[N, N * M]]


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    dev = torch.device(DEV)
    E, labels, N, ref = edge_case("nact17_of_N40_D36")
    R, D = E.shape
    thr = thresholds_of("reference")
    e = torch.as_tensor(E, device=dev)
    lab32 = torch.as_tensor(labels, device=dev)
    o = GF.cos_sim_labeled(e.clone().requires_grad_(True), lab32, num_speakers=N, thresholds=thr)
    assert o.cos.shape == (R, N) and o.col.shape == (R,) and o.speakers.shape == (N,) and o.active.shape == (2,)
    assert o.counts.shape == (50, 2) and o.counts.dtype == torch.int32 and not o.cos.requires_grad
    got = {k: getattr(o, k).cpu().numpy() for k in ("cos", "col", "speakers", "active")}
    check(got, ref, "cos_sim_labeled, int32 device labels")
    assert np.array_equal(o.counts.cpu().numpy(), ler.counts_ref(got["cos"], got["col"], got["active"][0], thr))
    # 3-D input; counts only
    o3 = GF.cos_sim_labeled(e[None], lab32[None], num_speakers=N, thresholds=thr, need_cos=False)
    assert o3.cos is None and o3.counts.shape == (1, 50, 2) and o3.col.shape == (1, R) and o3.active.shape == (1, 2)
    assert torch.equal(o3.counts[0], o.counts) and torch.equal(o3.col[0], o.col)
    # int64 device labels: 2**32 + 3 is ignored, not wrapped onto speaker 3; num_speakers is a bound
    lab64 = torch.as_tensor(labels.astype(np.int64), device=dev)
    out_rows = np.flatnonzero((labels < 0) | (labels >= N))
    assert len(out_rows) >= 2
    lab64[int(out_rows[0])] = 2 ** 32 + 3
    lab64[int(out_rows[1])] = -2 ** 40
    o64 = GF.cos_sim_labeled(e, lab64, num_speakers=N, thresholds=thr)
    assert torch.equal(o64.cos, o.cos) and torch.equal(o64.col, o.col) and torch.equal(o64.counts, o.counts)
    wide = GF.cos_sim_labeled(e, lab32, num_speakers=N + 9)
    assert wide.cos.shape == (R, N + 9) and wide.counts is None and torch.equal(wide.cos[:, :N], o.cos)
    assert not wide.cos[:, N:].any() and wide.speakers[N:].eq(-1).all() and torch.equal(wide.col, o.col)
    # host labels of arbitrary ids, negative ones on the rows to ignore: compacted by ascending id
    host = host_ids(labels, N, 9)
    oh = GF.cos_sim_labeled(e, host.tolist(), thresholds=thr)
    n_host = len(np.unique(host[host >= 0]))
    n_act = int(ref["active"][0])
    assert oh.cos.shape == (R, n_host) and torch.equal(oh.active, o.active) and torch.equal(oh.col, o.col)
    assert torch.equal(oh.cos[:, :n_act], o.cos[:, :n_act]) and torch.equal(oh.counts, o.counts)
    # eer_counts_labeled on w * cos + b
    sim = 0.9 * o.cos + 0.05
    c2 = GF.eer_counts_labeled(sim, o.col, o.active, thr)
    assert np.array_equal(c2.cpu().numpy(), ler.counts_ref(sim.cpu().numpy(), got["col"], n_act, thr))
    assert torch.equal(GF.eer_counts_labeled(sim[None], o.col[None], o.active[None], thr)[0], c2)
    with pytest.raises(ValueError, match="non-decreasing"):
        GF.eer_counts_labeled(sim, o.col, o.active, [0.6, 0.5])
    with pytest.raises(ValueError, match="non-decreasing"):
        GF.cos_sim_labeled(e, lab32, num_speakers=N, thresholds=[0.6, 0.5])
    with pytest.raises(ValueError, match="num_speakers"):
        GF.cos_sim_labeled(e, lab32)
    with pytest.raises(ValueError, match="nothing to compute"):
        GF.cos_sim_labeled(e, lab32, num_speakers=N, need_cos=False)
    with pytest.raises(TypeError, match="float32"):
        GF.cos_sim_labeled(e.double(), lab32, num_speakers=N)


def test_evaluate_labeled_on_two_batches_of_different_sizes(GF):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    thr = np.asarray(EV.THRESHOLDS)
    batches, want = [], []
    for name in MARGIN_CASES:
        labels, N, D, seed, _ = MARGIN_CASES[name]
        E = inputs(labels, N, D, seed)
        ref = reference(E, labels, N)
        m = ler.margin(ref["cos"], ref["col"], ref["active"][0], thr)
        assert m >= MARGIN, f"{name}: a reference cosine is {m:.2e} from a threshold"
        n_act, r_act = (int(v) for v in ref["active"])
        r = EV.eer_from_labeled_counts(ler.counts_ref(ref["cos"], ref["col"], n_act, thr), n_act, r_act)
        want.append(dict(r, n_act=n_act, r_act=r_act))
        batches.append((torch.as_tensor(E)[:, None, :], host_ids(labels, N, 10 + len(batches)).tolist()))
    assert batches[0][0].shape[0] != batches[1][0].shape[0]
    got = EV.evaluate_labeled(lambda x: x[:, 0, :], batches, device=DEV, verbose=False)
    print(got, want)
    assert got == want
    # device ids with a bound, one batch
    labels, N, D, seed, _ = MARGIN_CASES["N40_R75_D36"]
    dev_batch = [(batches[0][0], torch.as_tensor(labels, device=DEV))]
    assert EV.evaluate_labeled(lambda x: x[:, 0, :], dev_batch, num_speakers=N, device=DEV, verbose=False) == want[:1]


def test_graph_capture_replayed_with_other_labels(GF):
    dev = torch.device(DEV)
    N, R, D = 12, 48, 20
    lab_a, lab_b = draw(N, R, 5, 6, 9, 2), draw(N, R, 3, 2, 20, 51)
    E = inputs(lab_a, N, D, 8000)
    refs = [reference(E, lab, N) for lab in (lab_a, lab_b)]
    assert refs[0]["active"].tolist() != refs[1]["active"].tolist()
    e = torch.as_tensor(E, device=dev)[None].contiguous()
    lab = torch.zeros(1, R, dtype=torch.int32, device=dev)
    thr = torch.as_tensor(thresholds_of("seeded33"), dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        GF.cos_sim_labeled(e, lab, num_speakers=N, thresholds=thr)                       # (nothing counts yet)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = GF.cos_sim_labeled(e, lab, num_speakers=N, thresholds=thr)
    for labels, ref in zip((lab_a, lab_b), refs):
        lab.copy_(torch.as_tensor(labels, device=dev)[None])
        out.cos.fill_(float("nan"))
        out.counts.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        eager = GF.cos_sim_labeled(e, lab, num_speakers=N, thresholds=thr)
        for k in ("cos", "col", "speakers", "active", "counts"):
            assert torch.equal(getattr(out, k), getattr(eager, k)), f"replay differs from the eager call: {k}"
        check({k: getattr(out, k)[0].cpu().numpy() for k in ("cos", "col", "speakers", "active")}, ref,
              f"replay with active {ref['active'].tolist()}")
