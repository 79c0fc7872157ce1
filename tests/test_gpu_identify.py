"""GPU: speaker identification (ge2e_identify, ge2e_selftest_identify_slices, functional.identify,
evaluation.SpeakerBank.identify / evaluate_identification): the best k enrolled speakers of every trial row, the target's
rank and the histogram of ranks, over a bank axis that is split into slices.

References, never the code under test: tests/identify_ref.py (numpy) applied to two score matrices -- the fp32 matrix that
ge2e_verify_scores returns for the same inputs (exact: indices, ranks, histogram and score bits), and the float64
enroll_ref.scores_ref (the 3e-6 gate of tests/test_gpu_enroll.py on the scores; ranks on the rows that
tests/identify_cases.py calls decided, which tests/test_identify_cpu.py licenses).  The C-ABI tests call through ctypes on the
guarded buffers of tests/guarded.py: inputs between guards, outputs poisoned, the workspace exactly the advertised size
between guard bands, filled with 0xFF in one run and 0x00 in another.  `-s` prints every figure before it is asserted.
"""
import numpy as np
import pytest
import torch

import enroll_cases as ec
import enroll_ref as er
import identify_cases as ic
import identify_ref as ir
from capi import GF, lib  # noqa: F401
from guarded import Buf, IntBuf, Workspace, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = ec.GATE
EPS, EPS_COS = er.EPS, er.EPS_COS
NAMES = list(ec.VALUE_CASES)


# ---- the call on guarded buffers -------------------------------------------------------------------------------------------
def run_identify(lib, E, labels, models, cnt, k, slices=None, pattern=0xFF, want=("score", "rank", "hist")):
    """One ge2e_identify call (`slices`: ge2e_selftest_identify_slices with that many) -> dict of numpy outputs."""
    E, models, cnt = np.array(E, dtype=np.float32), np.array(models, dtype=np.float32), np.array(cnt, dtype=np.int32)
    (R, D), K = E.shape, len(cnt)
    what = f"identify K{K} R{R} D{D} k{k} slices {slices} fill {pattern:#04x} {'+'.join(want)}"
    e, m, c = Buf(E.shape, E), Buf(models.shape, models), IntBuf((K,), cnt)
    lab = IntBuf((R,), np.array(labels, dtype=np.int32)) if labels is not None else None
    outs = {"idx": IntBuf((R, k))}
    if "score" in want:
        outs["score"] = Buf((R, k))
    if "rank" in want and labels is not None:
        outs["rank"] = IntBuf((R,))
    if "hist" in want and labels is not None:
        outs["hist"] = IntBuf((k + 1,))
    nbytes = int(lib.ge2e_identify_workspace_bytes(K, R, D, k) if slices is None
                 else lib.ge2e_selftest_identify_workspace_bytes(K, R, D, k, slices))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    ptr = lambda b: b.ptr if b is not None else None  # noqa: E731
    args = (e.ptr, ptr(lab), m.ptr, c.ptr, K, R, D, k, EPS_COS, EPS, outs["idx"].ptr, ptr(outs.get("score")),
            ptr(outs.get("rank")), ptr(outs.get("hist")), ws.ptr, nbytes, None)
    code = lib.ge2e_identify(*args) if slices is None else lib.ge2e_selftest_identify_slices(*args, slices)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    res = {key: (b.get(f"{what} {key}", finite=False) if key == "score" else b.get(f"{what} {key}")) for key, b in outs.items()}
    ins = [e, m, c] + ([lab] if lab is not None else [])
    assert all(b.guards_intact() for b in ins), f"{what}: an input's guard"
    assert same_bits(e.get(what + " E", finite=False), E) and same_bits(m.get(what + " models", finite=False), models)
    return res


def verify_matrix(lib, E, labels, models, cnt):
    """The fp32 score matrix of ge2e_verify_scores, a kernel of the parent commit, for the same inputs."""
    E, models, cnt = np.array(E, dtype=np.float32), np.array(models, dtype=np.float32), np.array(cnt, dtype=np.int32)
    (R, D), K = E.shape, len(cnt)
    e, m, c, s = Buf(E.shape, E), Buf(models.shape, models), IntBuf((K,), cnt), Buf((R, K))
    lab = IntBuf((R,), np.array(labels, dtype=np.int32)) if labels is not None else None
    code = lib.ge2e_verify_scores(e.ptr, lab.ptr if lab else None, m.ptr, c.ptr, K, R, D, EPS_COS, EPS, None, 0, s.ptr, None, None,
                                  None)
    torch.cuda.synchronize()
    assert code == 0
    return s.get("verify_scores", finite=False)


_banks = {}


def bank_of(GF, lib, name):
    """-> cnt, models, matrix: the case's bank as the library fills it over the case's two calls, and the verify matrix of the
    case's trial rows against it: made once, read-only."""
    if name not in _banks:
        c = ec.case(name)
        dev = torch.device(DEV)
        sums = torch.zeros(c["K"], c["D"], device=dev)
        cnt = torch.zeros(c["K"], dtype=torch.int32, device=dev)
        for E, lab in c["calls"]:
            GF.enroll_accumulate(sums, cnt, torch.as_tensor(np.nan_to_num(E), device=dev), torch.as_tensor(np.array(lab), device=dev))
        models = GF.enroll_finalize(sums, cnt).cpu().numpy()
        cnt = cnt.cpu().numpy()
        assert np.array_equal(cnt, c["cnt"])
        matrix = verify_matrix(lib, c["E"], c["labels"], models, cnt)
        for a in (cnt, models, matrix):
            a.setflags(write=False)
        _banks[name] = cnt, models, matrix
    return _banks[name]


def check_exact(got, want, what):
    """idx, rank, hist equal and score bit-equal to topk_ref's of the library's own matrix (NaN for NaN where `nan_ok`)."""
    idx, score, rank, hist = want
    assert np.array_equal(got["idx"], idx), f"{what}: idx differs on rows {np.flatnonzero((got['idx'] != idx).any(1))[:8]}"
    if "score" in got:
        nan = np.isnan(score)
        assert np.array_equal(np.isnan(got["score"]), nan), f"{what}: NaN scores"
        assert same_bits(np.where(nan, np.float32(0), got["score"]), np.where(nan, np.float32(0), score)), f"{what}: score bits"
        assert (got["score"][idx < 0] == -np.inf).all(), f"{what}: score is not -inf where idx is -1"
    if "rank" in got:
        assert np.array_equal(got["rank"], rank), f"{what}: rank"
    if "hist" in got:
        assert np.array_equal(got["hist"], hist), f"{what}: hist {got['hist'].tolist()} against {hist.tolist()}"
        assert got["hist"].sum() == (rank >= 0).sum()


def same_outputs(a, b):
    return set(a) == set(b) and all(np.array_equal(a[key].view(np.int32), b[key].view(np.int32)) for key in a)


# ---- 1. exact, against the library's own score matrix ----------------------------------------------------------------------
@pytest.mark.parametrize("k", ic.TOPS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_against_the_verify_matrix_for_every_split(GF, lib, name, k):
    c = ec.case(name)
    cnt, models, matrix = bank_of(GF, lib, name)
    E = c["E"]
    for which, lab in ic.label_vectors(name).items():
        want = ir.topk_ref(matrix, lab, cnt, k)
        base = run_identify(lib, E, lab, models, cnt, k)
        check_exact(base, want, f"{name} k{k} {which}")
        assert not np.isnan(base["score"]).any(), f"{name}: NaN poison left in score"
        n_enrolled = int((cnt > 0).sum())
        scored = lab >= 0
        assert ((base["idx"][scored] >= 0).sum(1) == min(k, n_enrolled)).all() and (base["idx"][~scored] == -1).all()
        for slices in ic.slices_of(c["K"]):
            for pattern in (0xFF, 0x00):
                again = run_identify(lib, E, lab, models, cnt, k, slices=slices, pattern=pattern)
                assert same_outputs(again, base), f"{name} k{k} {which}: slices {slices}, fill {pattern:#04x} gives other bits"
    # the ignored rows are never read: other contents there, the same bits
    filled = E.copy()
    filled[c["labels"] < 0] = 0.25
    assert same_outputs(run_identify(lib, filled, c["labels"], models, cnt, k), run_identify(lib, E, c["labels"], models, cnt, k))


@pytest.mark.parametrize("name", ["K130_D36_R65", "K130_D256_R130", "K17_D7_R63"])
def test_rows_permuted(GF, lib, name):
    c = ec.case(name)
    cnt, models, _ = bank_of(GF, lib, name)
    lab = ic.random_labels(name)
    perm = np.random.default_rng(9).permutation(c["R"])
    for slices in (None, 2):
        a = run_identify(lib, c["E"], lab, models, cnt, 5, slices=slices)
        b = run_identify(lib, c["E"][perm], lab[perm], models, cnt, 5, slices=slices)
        assert np.array_equal(b["idx"], a["idx"][perm]) and same_bits(b["score"], a["score"][perm]), "a row's list depends on its place"
        assert np.array_equal(b["rank"], a["rank"][perm]) and np.array_equal(b["hist"], a["hist"])


# ---- 2. against float64, with no margin needed -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", ic.TOPS)
@pytest.mark.parametrize("name", NAMES)
def test_lists_against_float64(GF, lib, name, k):
    c = ec.case(name)
    cnt, models, _ = bank_of(GF, lib, name)
    ref = c["scores"]
    got = run_identify(lib, c["E"], c["labels"], models, cnt, k)
    enrolled = cnt > 0
    worst = [0.0, 0.0, 0.0]
    rows = np.flatnonzero(c["labels"] >= 0)
    for r in rows:                                                     # every scored row
        idx = got["idx"][r]
        n = int((idx >= 0).sum())
        assert n == min(k, int(enrolled.sum())) and (idx[:n] >= 0).all() and enrolled[idx[:n]].all() and len(set(idx[:n])) == n
        if not n:
            continue
        back = ref[r, idx[:n]]
        worst[0] = max(worst[0], float(np.abs(got["score"][r, :n] - back).max()))
        worst[1] = max(worst[1], float((back[1:] - back[:-1]).max()) if n > 1 else 0.0)
        rest = enrolled.copy()
        rest[idx[:n]] = False
        if rest.any():
            worst[2] = max(worst[2], float(ref[r, rest].max() - back[-1]))
    print(f"{name} k{k}: {len(rows)} rows; max|score - ref| {worst[0]:.2e} / {GATE:.0e}; largest rise along a list {worst[1]:.2e}, "
          f"largest excess of a speaker left out {worst[2]:.2e} / {2 * GATE:.0e}")
    assert worst[0] <= GATE, f"{name}: a returned score is {worst[0]:.3e} from the reference score of its index"
    assert worst[1] <= 2 * GATE, f"{name}: the reference scores of a list rise by {worst[1]:.3e}"
    assert worst[2] <= 2 * GATE, f"{name}: a speaker that was left out scores {worst[2]:.3e} above the last one returned"


# ---- 3. ranks against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ic.TOPS)
@pytest.mark.parametrize("name", NAMES)
def test_ranks_against_float64(GF, lib, name, k):
    c = ec.case(name)
    cnt, models, _ = bank_of(GF, lib, name)
    for which, lab in ic.label_vectors(name).items():
        n, of = ic.assert_cap(name, which)                              # (asserted on the CPU too, before anything is launched)
        dec = ic.undecided(name, which)[2]
        _, _, rank64, hist64 = ir.topk_ref(c["scores"], lab, c["cnt"], k)
        got = run_identify(lib, c["E"], lab, models, cnt, k)
        print(f"{name} k{k} {which}: {n} of {of} rows undecided; hist {got['hist'].tolist()}, float64 {hist64.tolist()}")
        assert np.array_equal(got["rank"][dec], rank64[dec]), f"{name} {which}: rank differs on a decided row"
        everything = np.ones(c["R"], dtype=bool)
        assert np.array_equal(got["hist"], ir.hist_of(got["rank"], everything, k)), f"{name} {which}: hist is not the histogram of rank"
        assert np.array_equal(ir.hist_of(got["rank"], dec, k), ir.hist_of(rank64, dec, k)), f"{name} {which}: hist on the decided rows"
        assert got["hist"].sum() == of


# ---- 4. ties and specials on a hand-made bank ------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt67", [1, 0])
def test_ties_and_specials(lib, cnt67):
    t = ic.tie_bank(cnt67)
    E, labels, models, cnt, K = t["E"], t["labels"], t["models"], t["cnt"], t["K"]
    matrix = verify_matrix(lib, E, labels, models, cnt)
    assert np.isnan(matrix[2, cnt > 0]).all() and not matrix[[3, 9]].any()
    tied = [3, 67, 129] if cnt67 else [3, 129]
    first = np.flatnonzero(cnt > 0)
    eps32 = np.float32(EPS)
    for k in ic.TOPS:
        want = ir.topk_ref(matrix, labels, cnt, k)
        for slices in (None, 1, 2, 3):
            got = run_identify(lib, E, labels, models, cnt, k, slices=slices)
            what = f"tie bank cnt67 {cnt67} k{k} slices {slices}"
            check_exact(got, want, what)
            n = min(k, len(tied))
            for r in (0, 4):                                           # the equal scores in index order, across 64 and 128
                assert got["idx"][r, :n].tolist() == tied[:n], f"{what}: row {r} {got['idx'][r, :3]}"
                assert len(set(got["score"][r, :n].view(np.uint32).tolist())) == 1
            assert got["idx"][1].tolist() == first[:k].tolist() and (got["score"][1] == eps32).all(), f"{what}: the zero row"
            assert got["idx"][2].tolist() == first[:k].tolist() and np.isnan(got["score"][2]).all(), f"{what}: the NaN row"
            assert (got["idx"][[3, 9]] == -1).all() and (got["score"][[3, 9]] == -np.inf).all() and (got["rank"][[3, 9]] == -1).all()
            assert got["rank"][5] == -1 and got["rank"][6] == -1 and got["rank"][8] == -1   # unenrolled, K, INT_MAX: no target
        # score = NULL, rank = NULL and hist = NULL in turn: the others keep their bits
        full = run_identify(lib, E, labels, models, cnt, k)
        for left_out in ("score", "rank", "hist"):
            part = run_identify(lib, E, labels, models, cnt, k, want=tuple(w for w in ("score", "rank", "hist") if w != left_out))
            assert set(part) == set(full) - {left_out}
            assert all(np.array_equal(part[key].view(np.int32), full[key].view(np.int32)) for key in part), f"without {left_out}"
        # no labels: every row is scored (the NaN rows 3 and 9 too), nobody has a target
        plain = run_identify(lib, E, None, models, cnt, k, slices=2)
        assert set(plain) == {"idx", "score"}
        scored = labels >= 0
        assert np.array_equal(plain["idx"][scored], full["idx"][scored])
        assert np.array_equal(plain["idx"][~scored], np.tile(first[:k], ((~scored).sum(), 1))) and np.isnan(plain["score"][~scored]).all()
        fin = scored & ~np.isnan(E).any(1)
        assert same_bits(plain["score"][fin], full["score"][fin])


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------
def test_python_surface(GF, lib):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    dev = torch.device(DEV)
    name = "K130_D36_R65"
    c = ec.case(name)
    K, D, R = c["K"], c["D"], c["R"]
    cnt_np, models_np, matrix = bank_of(GF, lib, name)
    lab = ic.random_labels(name)
    cnt, models = torch.as_tensor(np.array(cnt_np), device=dev), torch.as_tensor(np.array(models_np), device=dev)
    e = torch.as_tensor(np.nan_to_num(c["E"]), device=dev)
    for k in (1, 5):
        want = ir.topk_ref(matrix, lab, cnt_np, k)
        l64 = torch.as_tensor(lab.astype(np.int64), device=dev)
        l64[l64 < 0] = -2 ** 40
        o = GF.identify(e, models, cnt, k=k, labels=l64)                             # int64 device labels
        assert o.indices.shape == (R, k) and o.indices.dtype == torch.int32 and o.scores.shape == (R, k)
        assert o.rank.shape == (R,) and o.hist.shape == (k + 1,) and o.hist.dtype == torch.int32
        got = dict(idx=o.indices.cpu().numpy(), score=o.scores.cpu().numpy(), rank=o.rank.cpu().numpy(), hist=o.hist.cpu().numpy())
        check_exact(got, want, f"functional.identify k{k}")
        o2 = GF.identify(e, models, cnt, k=k, labels=lab.tolist(), need_scores=False)  # host ids, no scores
        assert o2.scores is None and torch.equal(o2.indices, o.indices) and torch.equal(o2.rank, o.rank) and torch.equal(o2.hist, o.hist)
        o3 = GF.identify(e, models, cnt, k=k)                                         # no labels: no rank, no hist
        scored = torch.as_tensor(lab >= 0, device=dev)
        assert o3.rank is None and o3.hist is None and torch.equal(o3.indices[scored], o.indices[scored])
        assert bool((o3.indices[~scored] >= 0).all())
        ws = torch.empty(int(lib.ge2e_identify_workspace_bytes(K, R, D, k)) + 256, dtype=torch.uint8, device=dev)
        ws = ws[(-ws.data_ptr()) % 256:]
        o4 = GF.identify(e, models, cnt, k=k, labels=l64, workspace=ws)               # the caller's workspace
        assert torch.equal(o4.indices, o.indices) and torch.equal(o4.scores, o.scores)
    with pytest.raises(ValueError, match="k must be"):
        GF.identify(e, models, cnt, k=33)
    with pytest.raises(ValueError, match="k must be"):
        GF.identify(e, models, cnt, k=0)
    with pytest.raises(TypeError):
        GF.identify(e, models, cnt.long(), k=1)
    with pytest.raises(ValueError):
        GF.identify(e[:, :-1].contiguous(), models, cnt, k=1)
    # SpeakerBank.identify on a bank of its own
    bank = EV.SpeakerBank(K, D, dev)
    for E1, l1 in c["calls"]:
        bank.enroll(torch.as_tensor(np.nan_to_num(E1), device=dev), l1.tolist())
    b = bank.identify(e, k=5, ids=torch.as_tensor(np.array(lab), device=dev))
    want = ir.topk_ref(matrix, lab, cnt_np, 5)
    check_exact(dict(idx=b.indices.cpu().numpy(), score=b.scores.cpu().numpy(), rank=b.rank.cpu().numpy(), hist=b.hist.cpu().numpy()),
                want, "SpeakerBank.identify")
    top1 = bank.identify(e)
    assert top1.indices.shape == (R, 1) and top1.rank is None and torch.equal(top1.indices[:, 0][scored], b.indices[:, 0][scored])


def test_evaluate_identification_on_batches_of_different_sizes(GF):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    name = "K17_D7_R63"
    c = ec.case(name)
    K, k = c["K"], 5
    lab = ic.random_labels(name)
    n, of, _ = ic.undecided(name, "random")
    assert n == 0, "the float64 histogram is the expectation only where every row is decided"
    trial_E = np.nan_to_num(c["E"])
    enroll = [(torch.as_tensor(np.nan_to_num(E))[:, None, :], l.tolist()) for E, l in c["calls"]]
    trials = [(torch.as_tensor(trial_E[:23])[:, None, :], torch.as_tensor(np.array(lab[:23]), device=DEV)),
              (torch.as_tensor(trial_E[23:])[:, None, :], lab[23:].tolist())]
    _, _, _, hist64 = ir.topk_ref(c["scores"], lab, c["cnt"], k)
    got = EV.evaluate_identification(lambda x: x[:, 0, :], enroll, trials, K, k=k, device=DEV, verbose=False)
    print(got, hist64.tolist())
    assert got["hist"] == hist64.tolist() and got["n_tgt"] == of == int(hist64.sum())
    assert got["rates"] == EV.identification_rates(hist64) and len(got["rates"]) == k
    assert 0 < got["rates"][0] < got["rates"][-1] < 1
    with pytest.raises(ValueError, match="empty"):
        EV.evaluate_identification(lambda x: x, [], trials, K, device=DEV, verbose=False)


def test_graph_capture_replayed_on_other_rows_and_labels(GF):
    dev = torch.device(DEV)
    name = "K17_D7_R63"
    c = ec.case(name)
    K, D, R, k = c["K"], c["D"], c["R"], 5
    E1, lab1 = c["calls"][0]
    e1 = torch.as_tensor(np.nan_to_num(E1), device=dev)
    l1 = torch.as_tensor(np.array(lab1), device=dev)
    rng = np.random.default_rng(78)
    perm = rng.permutation(R)
    rows_a, lab_a = np.nan_to_num(c["E"]), np.array(c["labels"])
    rows_b, lab_b = rows_a[perm] * np.float32(1.5), np.array(ic.random_labels(name))[perm]
    et = torch.zeros(R, D, device=dev)
    tl = torch.full((R,), -1, dtype=torch.int32, device=dev)
    sums = torch.zeros(K, D, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)

    def chain():
        sums.zero_()
        cnt.zero_()
        GF.enroll_accumulate(sums, cnt, e1, l1)
        models = GF.enroll_finalize(sums, cnt)
        return GF.identify(et, models, cnt, k=k, labels=tl)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = chain()
    for rows, labs in ((rows_a, lab_a), (rows_b, lab_b)):
        et.copy_(torch.as_tensor(rows, device=dev))
        tl.copy_(torch.as_tensor(labs, device=dev))
        out.indices.fill_(-7)
        out.scores.fill_(float("nan"))
        out.rank.fill_(-7)
        out.hist.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = {key: getattr(out, key).cpu().numpy().copy() for key in ("indices", "scores", "rank", "hist")}
        eager = chain()
        torch.cuda.synchronize()
        for key in got:
            assert np.array_equal(got[key].view(np.int32), getattr(eager, key).cpu().numpy().view(np.int32)), f"replay differs: {key}"
        assert got["hist"].sum() == (got["rank"] >= 0).sum() > 0 and (got["indices"][labs < 0] == -1).all()
    assert not np.array_equal(lab_a, lab_b)
