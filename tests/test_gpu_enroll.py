"""GPU: enrolment and verification (ge2e_enroll_accumulate, ge2e_enroll_finalize, ge2e_verify_scores, functional.enroll_* /
verify_scores, evaluation.SpeakerBank / evaluate_enrolled): a speaker bank filled from labelled rows in any order, and
held-out trial rows scored against it.

Reference, never the code under test: tests/enroll_ref.py (numpy float64) on the inputs of tests/enroll_cases.py, which
tests/test_enroll_cpu.py licenses.  The C-ABI tests call through ctypes on the guarded buffers of tests/guarded.py: inputs
between guards, outputs poisoned, the workspace exactly ge2e_enroll_workspace_bytes between guard bands, filled with 0xFF
bytes in one run and 0x00 in another (the two must agree bit for bit), guards intact and inputs unmodified afterwards.

Gates: max|score - ref| <= 3e-6 on the entries that count -- the project's bound for exact-fp32 cosines
(tests/test_gpu_labeled_eval.py, tests/test_gpu_helpers.py) -- and exact +0.0 everywhere else; per element of sums
|sums - ref| <= (m - 1) 2^-24 sum_i |e_i[d]|, the first-order bound of any fixed-order fp32 summation of the speaker's m
rows; cnt and trials exact; counts exact against numpy's fp32 `>` on the call's own scores, and against the float64
reference's where every counted reference score keeps at least 1.2e-5 (four gates) from every threshold, which each such
test asserts before anything is launched.  `-s` prints every figure before it is asserted.
"""
import numpy as np
import pytest
import torch

import enroll_cases as ec
import enroll_ref as er
from capi import GF, lib  # noqa: F401
from guarded import Buf, IntBuf, Workspace, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE, MARGIN = ec.GATE, ec.MARGIN
EPS, EPS_COS = er.EPS, er.EPS_COS


# ---- the calls on guarded buffers ------------------------------------------------------------------------------------------
def run_accumulate(lib, E, labels, sums, cnt, pattern=0xFF):
    """One ge2e_enroll_accumulate call: the bank (sums (K, D) float32, cnt (K,) int32) -> the bank after the call."""
    E, labels, cnt = np.array(E, dtype=np.float32), np.array(labels, dtype=np.int32), np.array(cnt, dtype=np.int32)   # (copies)
    (R, D), K = E.shape, len(cnt)
    what = f"enroll_accumulate K{K} R{R} D{D} fill {pattern:#04x}"
    e, lab = Buf(E.shape, E), IntBuf(labels.shape, labels)
    s, c = Buf((K, D), np.array(sums, dtype=np.float32)), IntBuf((K,), cnt)
    nbytes = int(lib.ge2e_enroll_workspace_bytes(K, R, D))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    code = lib.ge2e_enroll_accumulate(e.ptr, lab.ptr, K, R, D, s.ptr, c.ptr, ws.ptr, nbytes, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    out = s.get(what + " sums", finite=False), c.get(what + " cnt", written=False)
    assert e.guards_intact() and lab.guards_intact(), f"{what}: an input's guard"
    assert same_bits(e.get(what + " E", finite=False), E), f"{what}: E was modified"
    assert np.array_equal(lab.get(what + " labels", written=False), labels), f"{what}: the labels were modified"
    return out


def run_finalize(lib, sums, cnt):
    sums, cnt = np.array(sums, dtype=np.float32), np.array(cnt, dtype=np.int32)
    K, D = sums.shape
    what = f"enroll_finalize K{K} D{D}"
    s, c, m = Buf((K, D), sums), IntBuf((K,), cnt), Buf((K, D))
    code = lib.ge2e_enroll_finalize(s.ptr, c.ptr, K, D, EPS_COS, m.ptr, None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    out = m.get(what + " models")                                   # every element written, and finite
    assert s.guards_intact() and c.guards_intact(), f"{what}: an input's guard"
    assert same_bits(s.get(what + " sums", finite=False), sums) and np.array_equal(c.get(what, written=False), cnt)
    return out


def run_verify(lib, E, labels, models, cnt, thr=None, want_scores=True, want_trials=True, form=None, offset=0, finite=True):
    """One ge2e_verify_scores call (`form`: ge2e_selftest_verify_form with that form) -> dict of numpy outputs.  `offset`:
    scores start that many floats past a 16-byte boundary."""
    E, models, cnt = np.array(E, dtype=np.float32), np.array(models, dtype=np.float32), np.array(cnt, dtype=np.int32)
    (R, D), K = E.shape, len(cnt)
    T = 0 if thr is None else len(thr)
    what = f"verify_scores K{K} R{R} D{D} T{T} {'scores' if want_scores else 'no scores'} form {form}"
    e, m, c = Buf(E.shape, E), Buf(models.shape, models), IntBuf((K,), cnt)
    lab = IntBuf((R,), np.array(labels, dtype=np.int32)) if labels is not None else None
    th = Buf((T,), np.asarray(thr, dtype=np.float64).astype(np.float32)) if T else None
    outs = {}
    if want_scores:
        outs["scores"] = Buf((R, K), offset=offset)
    if T:
        outs["counts"] = IntBuf((T, 2))
    if want_trials and labels is not None:
        outs["trials"] = IntBuf((2,))
    ptr = lambda b: b.ptr if b is not None else None  # noqa: E731
    args = (e.ptr, ptr(lab), m.ptr, c.ptr, K, R, D, EPS_COS, EPS, ptr(th), T, ptr(outs.get("scores")), ptr(outs.get("counts")),
            ptr(outs.get("trials")), None)
    code = lib.ge2e_verify_scores(*args) if form is None else lib.ge2e_selftest_verify_form(*args, form)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    res = {k: (v.get(f"{what} {k}", finite=finite) if k == "scores" else v.get(f"{what} {k}")) for k, v in outs.items()}
    ins = [e, m, c] + [b for b in (lab, th) if b is not None]
    assert all(b.guards_intact() for b in ins), f"{what}: an input's guard"
    assert same_bits(e.get(what + " E", finite=False), E) and same_bits(m.get(what + " models", finite=False), models)
    return res


_banks = {}


def bank_of(lib, name):
    """The case's bank as the library fills it over the case's two calls, and its models: made once."""
    if name not in _banks:
        c = ec.case(name)
        sums, cnt = np.zeros((c["K"], c["D"]), dtype=np.float32), np.zeros(c["K"], dtype=np.int32)
        for E, lab in c["calls"]:
            sums, cnt = run_accumulate(lib, E, lab, sums, cnt)
        models = run_finalize(lib, sums, cnt)
        for a in (sums, cnt, models):
            a.setflags(write=False)
        _banks[name] = sums, cnt, models
    return _banks[name]


def check_scores(scores, c, what):
    """The gate of the module docstring for one score matrix against the case's reference."""
    imp, tgt = er.counted(c["labels"], c["cnt"], len(scores))
    on = imp | tgt
    err = float(np.abs(scores[on] - c["scores"][on]).max()) if on.any() else 0.0
    print(f"{what}: {int(on.sum())} entries count, max|score - ref| {err:.2e} / {GATE:.0e}")
    assert err <= GATE, f"{what}: max|score - ref| = {err:.3e}"
    rest = scores[~on]
    assert not rest.any() and not np.signbit(rest).any(), f"{what}: scores are not +0 where nothing counts"


# ---- 1. enrolment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.VALUE_CASES))
def test_enroll_values(lib, name):
    c = ec.case(name)
    K, D = c["K"], c["D"]
    banks = {}
    for pattern in (0xFF, 0x00):
        sums, cnt = np.zeros((K, D), dtype=np.float32), np.zeros(K, dtype=np.int32)
        for E, lab in c["calls"]:
            sums, cnt = run_accumulate(lib, E, lab, sums, cnt, pattern)
        banks[pattern] = sums, cnt
    sums, cnt = banks[0xFF]
    assert same_bits(sums, banks[0x00][0]) and np.array_equal(cnt, banks[0x00][1]), f"{name}: the bank depends on the workspace"
    assert np.array_equal(cnt, c["cnt"]), f"{name}: cnt"
    err = np.abs(sums.astype(np.float64) - c["sums"])
    share = float((err[c["sums_bound"] > 0] / c["sums_bound"][c["sums_bound"] > 0]).max()) if (c["sums_bound"] > 0).any() else 0.0
    print(f"{name}: max|sums - ref| {float(err.max()):.2e}, worst share of the bound {share:.3f}")
    assert (err <= c["sums_bound"]).all(), f"{name}: sums"
    assert same_bits(sums, bank_of(lib, name)[0]), f"{name}: a second pair of launches gives other bits"
    models = bank_of(lib, name)[2]
    off = cnt <= 0
    assert not models[off].any() and not np.signbit(models[off]).any(), f"{name}: models of speakers that are not enrolled"
    merr = float(np.abs(models - c["models"]).max())
    print(f"{name}: max|models - ref| {merr:.2e}")
    assert merr <= GATE and np.abs(np.linalg.norm(models[~off].astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_enroll_leaves_untouched_speakers_bits_alone(lib):
    K, D = 9, 20
    rng = np.random.default_rng(3)
    labels = np.array([3, 3, -1, 7, 9, ec.I32_MIN, 3, 0], dtype=np.int32)
    E = rng.standard_normal((len(labels), D)).astype(np.float32)
    E[[2, 4, 5]] = np.nan
    sums = rng.standard_normal((K, D)).astype(np.float32)
    cnt = np.array([2, 0, 0, 4, 0, 0, -3, 1, 0], dtype=np.int32)
    untouched = [1, 2, 4, 5, 6, 8]
    sums.view(np.uint32)[untouched] = 0x7FC12345 + np.arange(D, dtype=np.uint32)      # a NaN pattern of the test's own
    want, wcnt = er.accumulate_ref(sums, cnt, E, labels)
    got, gcnt = run_accumulate(lib, E, labels, sums, cnt)
    assert np.array_equal(gcnt, wcnt) and gcnt.tolist() == [3, 0, 0, 7, 0, 0, -3, 2, 0]
    assert same_bits(got[untouched], sums[untouched]), "a speaker without a row in the call was written"
    # (at most three additions per element, each within 2^-24 of a partial sum that the terms' magnitudes bound)
    bound = 3 * 2.0 ** -24 * (np.abs(sums[[0, 3, 7]]) + np.abs(E[[7, 0, 3]]) + np.abs(E[[7, 1, 3]]) + np.abs(E[[7, 6, 3]]))
    assert (np.abs(got[[0, 3, 7]] - want[[0, 3, 7]]) <= bound).all()
    models = run_finalize(lib, got, gcnt)                            # cnt <= 0: +0, and the NaN sums are never read
    assert not models[untouched].any() and not np.signbit(models[untouched]).any()
    assert np.abs(models - er.finalize_ref(want, wcnt)).max() <= GATE


@pytest.mark.parametrize("K,R,D", [(1030, 40, 8), (5000, 3, 5), (2500, 2100, 4)])
def test_enroll_many_speakers(lib, K, R, D):
    """Above 1024 speakers the index kernel's counters leave LDS for the workspace; K far above R; more rows than a chunk."""
    rng = np.random.default_rng(K)
    labels = rng.integers(0, K, R).astype(np.int32)
    labels[R // 2] = K
    labels[0] = K - 1
    E = rng.standard_normal((R, D)).astype(np.float32)
    E[R // 2] = np.nan
    zero = np.zeros((K, D), dtype=np.float32), np.zeros(K, dtype=np.int32)
    a = run_accumulate(lib, E, labels, *zero, pattern=0xFF)
    b = run_accumulate(lib, E, labels, *zero, pattern=0x00)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    want, wcnt = er.accumulate_ref(*zero, E, labels)
    assert np.array_equal(a[1], wcnt) and a[1].sum() == R - 1 and a[1][K - 1] >= 1
    assert (np.abs(a[0] - want) <= er.sums_bound([(E, labels)], K, D)).all()


@pytest.mark.parametrize("name", ["K17_D7_R63", "K130_D36_R65"])
def test_enroll_rows_permuted_with_every_speakers_order_kept(lib, name):
    c = ec.case(name)
    E, labels = c["calls"][0]
    R = len(labels)
    new_labels = labels[np.random.default_rng(44).permutation(R)]
    src = np.empty(R, dtype=np.int64)               # new row i is old row src[i]: the rows of one label keep their order
    for v in np.unique(labels):
        src[np.flatnonzero(new_labels == v)] = np.flatnonzero(labels == v)
    assert np.array_equal(labels[src], new_labels) and not np.array_equal(src, np.arange(R))
    zero = np.zeros((c["K"], c["D"]), dtype=np.float32), np.zeros(c["K"], dtype=np.int32)
    a = run_accumulate(lib, E, labels, *zero)
    b = run_accumulate(lib, E[src], new_labels, *zero)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{name}: sums depend on where the other speakers' rows stand"


# ---- 2. verification ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.VALUE_CASES))
def test_verify_values(lib, name):
    c = ec.case(name)
    thr = ec.reference_thresholds()
    m = er.margin(c["scores"], c["labels"], c["cnt"], thr)
    want64, trials64 = er.counts_ref(c["scores"], c["labels"], c["cnt"], thr)
    print(f"{name}: margin {m:.2e} (needs {MARGIN:.1e}); trials {trials64.tolist()}; accepts at the first threshold {want64[0].tolist()}")
    assert m >= MARGIN, f"{name}: a reference score is {m:.2e} from a threshold"
    _, cnt, models = bank_of(lib, name)
    E, labels = c["E"], c["labels"]
    full = run_verify(lib, E, labels, models, cnt, thr)
    check_scores(full["scores"], c, name)
    own, trials = er.counts_ref(full["scores"], labels, cnt, thr)
    assert np.array_equal(full["counts"], own), f"{name}: the counts are not numpy's on the call's own scores"
    assert np.array_equal(full["trials"], trials) and np.array_equal(trials, trials64), f"{name}: trials"
    assert np.array_equal(full["counts"], want64), f"{name}: counts differ from the float64 reference's"
    # a second launch, and both forms of the rows kernel: the same bits
    for form in (None, 1, 2):
        again = run_verify(lib, E, labels, models, cnt, thr, form=form)
        for k in full:
            assert same_bits(again[k].view(np.float32), full[k].view(np.float32)), f"{name}: {k} differs, form {form}"
    # scores = NULL: the same counts; counts and trials left out: the same scores
    nos = run_verify(lib, E, labels, models, cnt, thr, want_scores=False)
    assert set(nos) == {"counts", "trials"} and all(np.array_equal(nos[k], full[k]) for k in nos), f"{name}: without scores"
    alone = run_verify(lib, E, labels, models, cnt, None, want_trials=False)
    assert set(alone) == {"scores"} and same_bits(alone["scores"], full["scores"]), f"{name}: scores alone"
    # the ignored rows are never read: other contents there, the same bits
    scored, _, _ = er.classes(labels, cnt, len(E))
    filled = E.copy()
    filled[~scored] = 0.25
    other = run_verify(lib, filled, labels, models, cnt, thr)
    for k in full:
        assert same_bits(other[k].view(np.float32), full[k].view(np.float32)), f"{name}: {k} depends on an ignored row"
    # labels = NULL: every row is scored, the rows scored before keep their bits
    plain = run_verify(lib, filled, None, models, cnt)
    assert set(plain) == {"scores"} and same_bits(plain["scores"][scored], full["scores"][scored]), f"{name}: labels = NULL"
    if (~scored).any():
        assert plain["scores"][~scored][:, cnt > 0].all() and not plain["scores"][:, cnt <= 0].any()


def test_verify_scores_off_a_16_byte_boundary(lib):
    name = "K16_D256_R17"
    c = ec.case(name)
    _, cnt, models = bank_of(lib, name)
    a = run_verify(lib, c["E"], c["labels"], models, cnt)
    b = run_verify(lib, c["E"], c["labels"], models, cnt, offset=1)
    assert same_bits(a["scores"], b["scores"])


def test_verify_rows_permuted(lib):
    name = "K130_D36_R65"
    c = ec.case(name)
    _, cnt, models = bank_of(lib, name)
    perm = np.random.default_rng(9).permutation(c["R"])
    a = run_verify(lib, c["E"], c["labels"], models, cnt, ec.reference_thresholds())
    b = run_verify(lib, c["E"][perm], c["labels"][perm], models, cnt, ec.reference_thresholds())
    assert same_bits(b["scores"], a["scores"][perm]), "a row's scores depend on where it stands"
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["trials"], b["trials"])


@pytest.mark.parametrize("T", [1, 50, 2730, 2731, 4096])
def test_verify_threshold_tables(lib, T):
    """T = 50: the reference's table.  Up to T = 2730 the staged form of the rows kernel has room for its model tiles beside
    the histograms, above that it streams like the product call.  Values equal to a threshold, NaN and Inf among the scores:
    the models hold them."""
    name = "K17_D7_R63"
    c = ec.case(name)
    _, cnt, models = bank_of(lib, name)
    models = models.copy()
    enrolled = np.flatnonzero(cnt > 0)
    models[enrolled[1]] = np.nan
    models[enrolled[2]] = 0
    models[enrolled[2], 0] = np.inf                                    # Inf and -Inf scores
    thr = ec.thresholds_of(T)
    o = run_verify(lib, c["E"], c["labels"], models, cnt, thr, finite=False)
    again = run_verify(lib, c["E"], c["labels"], models, cnt, thr, want_scores=False)
    staged = run_verify(lib, c["E"], c["labels"], models, cnt, thr, form=1, finite=False)
    assert all(same_bits(staged[k].view(np.float32), o[k].view(np.float32)) for k in o), f"T {T}: the staged form differs"
    want, trials = er.counts_ref(o["scores"], c["labels"], cnt, thr)
    assert np.isnan(o["scores"]).any() and np.isinf(o["scores"]).any() and want[0].sum() > 0
    assert np.array_equal(o["counts"], want), f"T {T}: differs at {int((o['counts'] != want).sum())} of {want.size}"
    assert np.array_equal(o["trials"], trials) and np.array_equal(again["counts"], want)
    # thresholds that ARE scores: `>` is strict
    if T >= 50:
        s = o["scores"][np.isfinite(o["scores"]) & (o["scores"] != 0)]
        thr2 = np.sort(np.concatenate([thr[: T - 20], s[:: max(1, len(s) // 20)][:20].astype(np.float64)]))
        assert len(thr2) == T
        o2 = run_verify(lib, c["E"], c["labels"], models, cnt, thr2, want_scores=False)
        assert np.array_equal(o2["counts"], er.counts_ref(o["scores"], c["labels"], cnt, thr2)[0])


def test_verify_wild_labels_and_cnt(lib):
    """No target: labels K, INT_MAX and speakers with cnt <= 0 (negative counts too) -- impostors against everybody; an
    unenrolled column is +0 whatever its model holds."""
    K, R, D = 21, 40, 12
    rng = np.random.default_rng(12)
    cnt = rng.integers(-2, 4, K).astype(np.int32)
    cnt[:3] = [1, 0, -5]
    models = rng.standard_normal((K, D)).astype(np.float32)
    models[cnt <= 0] = np.nan
    labels = rng.integers(-3, K + 3, R).astype(np.int32)
    labels[:6] = [0, 1, 2, K, ec.I32_MAX, ec.I32_MIN]
    E = rng.standard_normal((R, D)).astype(np.float32)
    E[labels < 0] = np.nan
    thr = ec.thresholds_of(33)
    o = run_verify(lib, E, labels, models, cnt, thr)
    ref = er.scores_ref(E, labels, np.nan_to_num(models), cnt)
    # (the models are not unit vectors here: the fp32 contraction's error grows with sum|a b| <= |e-hat| |model|)
    assert np.abs(o["scores"] - ref).max() <= GATE * np.linalg.norm(np.nan_to_num(models).astype(np.float64), axis=1).max()
    imp, tgt = er.counted(labels, cnt, R)
    rest = o["scores"][~(imp | tgt)]
    assert not rest.any() and not np.signbit(rest).any()
    want, trials = er.counts_ref(o["scores"], labels, cnt, thr)
    assert np.array_equal(o["counts"], want) and np.array_equal(o["trials"], trials)
    assert not tgt[1].any() and not tgt[2].any() and imp[1].sum() == (cnt > 0).sum() and tgt[0, 0]


# ---- 3. the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface(GF):
    dev = torch.device(DEV)
    name = "K130_D36_R65"
    c = ec.case(name)
    K, D = c["K"], c["D"]
    sums = torch.zeros(K, D, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)
    (E1, l1), (E2, l2) = ((np.array(E), np.array(lab)) for E, lab in c["calls"])      # (copies: the case's arrays are read-only)
    GF.enroll_accumulate(sums, cnt, torch.as_tensor(E1, device=dev), torch.as_tensor(l1, device=dev))            # int32 device ids
    l2_64 = torch.as_tensor(l2.astype(np.int64), device=dev)
    l2_64[l2_64 < 0] = -2 ** 40
    l2_64[l2_64 == K] = 2 ** 32 + 3                                   # not wrapped onto speaker 3
    GF.enroll_accumulate(sums, cnt, torch.as_tensor(E2, device=dev), l2_64)
    assert np.array_equal(cnt.cpu().numpy(), c["cnt"])
    assert (np.abs(sums.cpu().numpy() - c["sums"]) <= c["sums_bound"]).all()
    host = torch.zeros_like(sums), torch.zeros_like(cnt)
    GF.enroll_accumulate(*host, torch.as_tensor(E1, device=dev), l1.tolist())                                  # host ids, as they are
    GF.enroll_accumulate(*host, torch.as_tensor(E2, device=dev), l2.tolist())
    assert torch.equal(host[1], cnt) and same_bits(host[0].cpu().numpy(), sums.cpu().numpy())
    models = GF.enroll_finalize(sums, cnt)
    assert models.shape == (K, D) and np.abs(models.cpu().numpy() - c["models"]).max() <= GATE
    thr = ec.reference_thresholds()
    e = torch.as_tensor(np.nan_to_num(c["E"]), device=dev)
    lab = torch.as_tensor(np.array(c["labels"]), device=dev)
    o = GF.verify_scores(e, models, cnt, labels=lab, thresholds=thr)
    assert o.scores.shape == (c["R"], K) and o.counts.shape == (50, 2) and o.trials.shape == (2,) and o.counts.dtype == torch.int32
    check_scores(o.scores.cpu().numpy(), c, "verify_scores")
    want, trials = er.counts_ref(c["scores"], c["labels"], c["cnt"], thr)
    assert np.array_equal(o.counts.cpu().numpy(), want) and np.array_equal(o.trials.cpu().numpy(), trials)
    o2 = GF.verify_scores(e, models, cnt, labels=c["labels"].tolist(), thresholds=thr, need_scores=False)
    assert o2.scores is None and torch.equal(o2.counts, o.counts) and torch.equal(o2.trials, o.trials)
    o3 = GF.verify_scores(e, models, cnt)
    scored = torch.as_tensor(c["labels"] >= 0, device=dev)
    assert o3.counts is None and o3.trials is None and torch.equal(o3.scores[scored], o.scores[scored])
    o4 = GF.verify_scores(e, models, cnt, labels=lab)
    assert o4.counts is None and torch.equal(o4.trials, o.trials) and torch.equal(o4.scores, o.scores)
    with pytest.raises(ValueError, match="need labels"):
        GF.verify_scores(e, models, cnt, thresholds=thr)
    with pytest.raises(ValueError, match="nothing to compute"):
        GF.verify_scores(e, models, cnt, labels=lab, need_scores=False)
    with pytest.raises(ValueError, match="non-decreasing"):
        GF.verify_scores(e, models, cnt, labels=lab, thresholds=[0.6, 0.5])
    with pytest.raises(TypeError):
        GF.enroll_accumulate(sums, cnt.long(), e, lab)
    with pytest.raises(ValueError):
        GF.enroll_accumulate(sums, cnt, e[:, :-1].contiguous(), lab)
    with pytest.raises(TypeError, match="integers"):
        GF.enroll_accumulate(sums, cnt, e, [0.5] * c["R"])


def test_speaker_bank_and_evaluate_enrolled_on_batches_of_different_sizes(GF):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    dev = torch.device(DEV)
    c = ec.case("K17_D7_R63")                                        # (false accepts at the low thresholds)
    K, D, R = c["K"], c["D"], c["R"]
    thr = ec.reference_thresholds()
    m = er.margin(c["scores"], c["labels"], c["cnt"], thr)
    assert m >= MARGIN, f"a reference score is {m:.2e} from a threshold"
    trial_E = np.nan_to_num(c["E"])
    enroll = [(torch.as_tensor(np.nan_to_num(E))[:, None, :], lab.tolist()) for E, lab in c["calls"]]
    trials = [(torch.as_tensor(trial_E[:23])[:, None, :], torch.as_tensor(np.array(c["labels"][:23]), device=dev)),
              (torch.as_tensor(trial_E[23:])[:, None, :], c["labels"][23:].tolist())]
    assert enroll[0][0].shape[0] != enroll[1][0].shape[0] and trials[0][0].shape[0] != trials[1][0].shape[0]
    counts, (n_imp, n_tgt) = er.counts_ref(c["scores"], c["labels"], c["cnt"], thr)     # numpy on the concatenated sets
    want = dict(EV.eer_from_trial_counts(counts, n_imp, n_tgt), n_imp=int(n_imp), n_tgt=int(n_tgt))
    got = EV.evaluate_enrolled(lambda x: x[:, 0, :], enroll, trials, K, device=DEV, verbose=False)
    print(got, want)
    assert got == want and n_imp > 0 and n_tgt > 0 and counts[0, 0] > 0 and 0 < got["EER"] < 0.5
    bank = EV.SpeakerBank(K, D, dev)
    bank.enroll(enroll[0][0][:, 0].to(dev), enroll[0][1])
    first = bank.models()
    assert bank.models() is first                                     # finalised lazily, once
    bank.enroll(enroll[1][0][:, 0].to(dev), enroll[1][1])
    assert bank.models() is not first and np.array_equal(bank.cnt.cpu().numpy(), c["cnt"])
    e = torch.as_tensor(trial_E, device=dev)
    v = bank.verify(e, torch.as_tensor(np.array(c["labels"]), device=dev))
    check_scores(v.scores.cpu().numpy(), c, "SpeakerBank.verify")
    assert np.array_equal(v.counts.cpu().numpy(), counts) and v.trials.tolist() == [n_imp, n_tgt]
    scored = torch.as_tensor(c["labels"] >= 0, device=dev)
    s = bank.score(e)
    assert s.shape == (R, K) and torch.equal(s[scored], v.scores[scored])


def test_graph_capture_replayed_with_other_labels(GF):
    dev = torch.device(DEV)
    c = ec.case("K17_D7_R63")
    K, D, R = c["K"], c["D"], c["R"]
    E1, lab_a = c["calls"][0]
    E1 = np.nan_to_num(E1)
    rng = np.random.default_rng(77)
    lab_b = lab_a[rng.permutation(len(lab_a))]
    trial_E = np.nan_to_num(c["E"])
    tl_a, tl_b = c["labels"], c["labels"][rng.permutation(R)]
    thr64 = ec.thresholds_of(33)
    e1, et = torch.as_tensor(E1, device=dev), torch.as_tensor(trial_E, device=dev)
    lab = torch.full((len(lab_a),), -1, dtype=torch.int32, device=dev)
    tl = torch.full((R,), -1, dtype=torch.int32, device=dev)
    thr = torch.as_tensor(thr64, dtype=torch.float32, device=dev)
    sums = torch.zeros(K, D, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)

    def chain():
        sums.zero_()
        cnt.zero_()
        GF.enroll_accumulate(sums, cnt, e1, lab)
        models = GF.enroll_finalize(sums, cnt)
        return models, GF.verify_scores(et, models, cnt, labels=tl, thresholds=thr)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain()                                                       # (nobody is enrolled yet)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        models, out = chain()
    for la, ta in ((lab_a, tl_a), (lab_b, tl_b)):
        lab.copy_(torch.as_tensor(np.array(la), device=dev))
        tl.copy_(torch.as_tensor(np.array(ta), device=dev))
        out.scores.fill_(float("nan"))
        out.counts.fill_(-7)
        out.trials.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: getattr(out, k).cpu().numpy() for k in ("scores", "counts", "trials")}
        got_cnt = cnt.cpu().numpy()
        em, eo = chain()
        torch.cuda.synchronize()
        assert torch.equal(em, models)
        for k in got:
            assert np.array_equal(got[k], getattr(eo, k).cpu().numpy()), f"replay differs from the eager chain: {k}"
        rs, rc = er.accumulate_ref(np.zeros((K, D)), np.zeros(K, dtype=np.int64), E1, la)
        ref = er.scores_ref(trial_E, ta, er.finalize_ref(rs, rc), rc)
        assert np.array_equal(got_cnt, rc)
        imp, tgt = er.counted(ta, rc, R)
        on = imp | tgt
        err = float(np.abs(got["scores"][on] - ref[on]).max())
        print(f"replay: {int(on.sum())} entries count, max|score - ref| {err:.2e} / {GATE:.0e}")
        assert err <= GATE and not got["scores"][~on].any()
        want, trials = er.counts_ref(got["scores"], ta, rc, thr64)
        assert np.array_equal(got["counts"], want) and np.array_equal(got["trials"], trials)
    assert not np.array_equal(lab_a, lab_b)
