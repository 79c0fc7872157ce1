"""CPU: the host side of enrolment and verification -- ge2e_enroll_workspace_bytes / ge2e_enroll_accumulate /
ge2e_enroll_finalize / ge2e_verify_scores and evaluation.eer_from_trial_counts: declared, exported and bound, a sane
workspace size, every error code and the order of the checks.  tests/enroll_ref.py, the reference of the GPU tests, is
held to tests/labeled_eval_ref.py where the two must agree, and the inputs of tests/enroll_cases.py are licensed for the
GPU gate: with the sums accumulated sequentially in fp32 their scores stay within half the gate of the float64 reference,
and every counted reference score keeps four gates from every reference threshold."""
import ctypes
import re

import numpy as np
import pytest

import enroll_cases as ec
import enroll_ref as er
import labeled_eval_ref as ler
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from rowlist_cases import inputs
from speaker_embedding_ge2e_loss_amd import _lib, build
from speaker_embedding_ge2e_loss_amd import evaluation as EV

SYMS = ("ge2e_enroll_workspace_bytes", "ge2e_enroll_accumulate", "ge2e_enroll_finalize", "ge2e_verify_scores")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -6
I, F, P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_enroll_workspace_bytes"] == (ctypes.c_size_t, [I] * 3)
    assert _lib.PROTOTYPES["ge2e_enroll_accumulate"] == (I, [P, P, I, I, I, P, P, P, ctypes.c_size_t, P])
    assert _lib.PROTOTYPES["ge2e_enroll_finalize"] == (I, [P, P, I, I, F, P, P])
    assert _lib.PROTOTYPES["ge2e_verify_scores"] == (I, [P, P, P, P, I, I, I, F, F, P, I, P, P, P, P])
    assert hasattr(EV, "SpeakerBank") and hasattr(EV, "evaluate_enrolled")


def bound(K, R):
    """offsets [K+1], order [R], speakers [K], active [2], and above 1024 speakers K counters: five parts, each rounded up
    to 256 bytes."""
    return 4 * ((K + 1) + R + K + 2 + (K if K > 1024 else 0)) + 5 * 255


def test_workspace_bytes(lib):
    f = lib.ge2e_enroll_workspace_bytes
    for base in ((7, 2100, 36), (1020, 40, 8)):
        for axis in range(2):                                          # monotone in K and in R
            prev = 0
            for step in (0, 1, 2, 5, 30, 700, 3000):
                shape = list(base)
                shape[axis] += step
                cur = f(*shape)
                assert cur > 0 and cur % 256 == 0 and prev <= cur <= bound(*shape[:2]), (shape, cur, prev)
                assert cur >= 4 * (2 * shape[0] + shape[1] + 3)
                prev = cur
    assert f(7, 40, 1) == f(7, 40, 4096)                               # no plane of the workspace has a D
    assert f(1025, 40, 8) - f(1024, 40, 8) >= 4 * 1025                 # the counters leave LDS above 1024 speakers
    for shape in ((1, 1, 1), (5000, 3, 5), (1030, 40, 8), (1251, 16384, 256), (100000, 70, 64)):
        assert 0 < f(*shape) <= bound(*shape[:2]) and f(*shape) % 256 == 0, shape
    for bad in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8), (4, -4, 8), (4, 4, -8)):
        assert f(*bad) == 0, bad


def test_enroll_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_enroll_accumulate
    ok = dict(E=16, labels=16, K=4, R=20, D=8, sums=32, cnt=16, ws=256, ws_bytes=1 << 40, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("E", "labels", "sums", "cnt"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("K", "R", "D"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -3}) == ERR_SHAPE, k
    need = lib.ge2e_enroll_workspace_bytes(4, 20, 8)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws=None, ws_bytes=0) == ERR_WORKSPACE
    assert call(ws=264) == ERR_WORKSPACE
    assert call(E=24) == ERR_ALIGN and call(E=20) == ERR_ALIGN and call(sums=40) == ERR_ALIGN
    # the order: NULL, shape, workspace, alignment
    assert call(cnt=None, K=0) == ERR_NULL and call(labels=None, ws=None, E=24) == ERR_NULL
    assert call(R=0, ws=None) == ERR_SHAPE and call(D=0, ws=None, sums=40) == ERR_SHAPE
    assert call(ws=None, E=24) == ERR_WORKSPACE and call(ws_bytes=need - 1, sums=40) == ERR_WORKSPACE

    g = lib.ge2e_enroll_finalize
    okf = dict(sums=16, cnt=16, K=4, D=8, eps_cos=1e-8, models=16, stream=None)

    def callf(**kw):
        a = dict(okf, **kw)
        return g(*[a[k] for k in okf])

    for k in ("sums", "cnt", "models"):
        assert callf(**{k: None}) == ERR_NULL, k
    for k in ("K", "D"):
        assert callf(**{k: 0}) == ERR_SHAPE and callf(**{k: -1}) == ERR_SHAPE, k
    assert callf(models=None, K=0) == ERR_NULL


def test_verify_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_verify_scores
    ok = dict(E=16, labels=16, models=16, cnt=16, K=4, R=20, D=8, eps_cos=1e-8, eps=1e-6, thr=16, T=50, scores=16, counts=16,
              trials=16, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("E", "models", "cnt"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(scores=None, counts=None) == ERR_NULL                           # nothing asked for
    assert call(scores=None, counts=None, trials=None, thr=None, T=0) == ERR_NULL
    assert call(labels=None) == ERR_NULL                                        # counts and trials need labels
    assert call(labels=None, counts=None, thr=None, T=0) == ERR_NULL            # ... trials alone too
    assert call(labels=None, trials=None) == ERR_NULL
    for k in ("K", "R", "D"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    assert call(T=-1) == ERR_SHAPE and call(T=4097) == ERR_SHAPE and call(T=4097, counts=None) == ERR_SHAPE
    assert call(thr=None) == ERR_SHAPE and call(T=0) == ERR_SHAPE               # counts without thresholds / with T = 0
    assert call(K=65536, R=32768) == ERR_SHAPE                                  # R K = 2^31 with counts
    assert call(K=65536, R=32768, counts=None, thr=None, T=0) == ERR_SHAPE      # ... with trials alone
    assert call(E=24) == ERR_ALIGN and call(models=20) == ERR_ALIGN
    # the order: NULL, shape, alignment
    assert call(cnt=None, R=0) == ERR_NULL and call(scores=None, counts=None, T=4097) == ERR_NULL
    assert call(labels=None, K=0, E=24) == ERR_NULL
    assert call(R=0, E=24) == ERR_SHAPE and call(T=4097, models=20) == ERR_SHAPE


def test_eer_from_trial_counts_by_hand():
    thr = [0.5, 0.6, 0.7, 0.8]
    counts = [[8, 10], [4, 9], [1, 6], [0, 2]]
    # FAR = fa / 16: 0.5, 0.25, 0.0625, 0;  FRR = (10 - ta) / 10: 0, 0.1, 0.4, 0.8;  |FAR - FRR|: 0.5, 0.15, 0.3375, 0.8
    r = EV.eer_from_trial_counts(counts, 16, 10, thr)
    assert r == {"EER": (0.25 + 0.1) / 2, "thres": 0.6, "FAR": 0.25, "FRR": (10 - 9) / 10}
    # a zero denominator gives 0
    assert EV.eer_from_trial_counts(counts, 0, 10, thr) == {"EER": 0.0, "thres": 0.5, "FAR": 0, "FRR": 0.0}
    r = EV.eer_from_trial_counts(counts, 16, 0, thr)
    assert r["FRR"] == 0 and r["FAR"] == 0 and r["thres"] == 0.8
    assert EV.eer_from_trial_counts([[0, 0]] * 50, 0, 0) == {"EER": 0.0, "thres": EV.THRESHOLDS[0], "FAR": 0, "FRR": 0}
    # the labelled sweep at its own denominators
    assert EV.eer_from_trial_counts(counts, 5 * 3, 5, thr) == EV.eer_from_labeled_counts(counts, 4, 5, thr)


def test_counts_ref_at_the_edges():
    scores = np.array([[0.7, 0.2, 9.0], [0.6, np.inf, 9.0], [9.0, 9.0, 9.0], [np.nan, 0.65, 9.0], [0.9, 0.55, 9.0]],
                      dtype=np.float32)
    labels, cnt = [0, 1, -1, 0, 7], [2, 1, 0]            # row 2 ignored, row 4 an unknown speaker, speaker 2 not enrolled
    counts, trials = er.counts_ref(scores, labels, cnt, [0.5, 0.6, 0.6, 0.7])
    assert trials.tolist() == [5, 3]                     # NaN is tallied where it would have been binned
    assert counts.tolist() == [[4, 2], [2, 2], [2, 2], [1, 1]]
    imp, tgt = er.counted(labels, cnt, 5)
    assert not imp[2].any() and not tgt[2].any() and not imp[:, 2].any() and imp[4].tolist() == [True, True, False]


def test_enroll_ref_is_labeled_eval_ref_on_the_other_speakers_columns():
    for (N, R, D), seed in (((6, 30, 12), 1), ((9, 40, 33), 2)):
        labels = np.random.default_rng(seed).permutation(np.arange(R) % N).astype(np.int32)
        E = inputs(labels, N, D, seed)
        cos, col, speakers, active = ler.cos_ref(E, labels, N)
        assert active.tolist() == [N, R] and speakers.tolist() == list(range(N))
        sums, cnt = er.accumulate_ref(np.zeros((N, D)), np.zeros(N, dtype=np.int64), E, labels)
        scores = er.scores_ref(E, labels, er.finalize_ref(sums, cnt), cnt)
        other = col[:, None] != np.arange(N)[None, :]
        assert np.abs(scores - cos)[other].max() <= 1e-12
        assert np.abs(scores - cos)[~other].min() > 1e-4          # the own column: a model that holds the row itself
        # the counts of the two references on one matrix, at the trial classes those labels give
        thr = ec.reference_thresholds()
        c, trials = er.counts_ref(cos, labels, cnt, thr)
        assert np.array_equal(c, ler.counts_ref(cos, col, N, thr)) and trials.tolist() == [R * (N - 1), R]


def test_accumulate_ref_leaves_untouched_speakers_alone():
    sums = np.full((4, 3), np.nan)
    sums[1] = 1.0
    E = np.array([[1, 2, 3], [np.nan] * 3, [10, 20, 30], [np.nan] * 3], dtype=np.float32)
    out, cnt = er.accumulate_ref(sums, [0, 5, 0, 0], E, [1, -1, 1, 4])
    assert cnt.tolist() == [0, 7, 0, 0] and out[1].tolist() == [12.0, 23.0, 34.0]
    assert np.isnan(out[[0, 2, 3]]).all()
    m = er.finalize_ref(out, cnt)
    assert not m[[0, 2, 3]].any() and abs(np.linalg.norm(m[1]) - 1) < 1e-15


@pytest.mark.parametrize("name", list(ec.VALUE_CASES))
def test_value_inputs_are_licensed_for_the_gpu_gate(name):
    c = ec.case(name)
    K, D = c["K"], c["D"]
    per = np.zeros(K, dtype=np.int64)
    per_call = [np.bincount(lab[er.valid_rows(lab, K)], minlength=K) for _, lab in c["calls"]]
    per = per_call[0] + per_call[1]
    assert per.max() <= 70 and np.array_equal(per, c["cnt"])
    if K >= 8:   # one call holds speakers of 1, 2, 64 and 65 rows, and absent ones; one speaker is never enrolled
        assert {0, 1, 2, 64, 65} <= set(per_call[0].tolist()) and (per == 0).any() and ((per_call[0] == 0) & (per > 0)).any()
    # the sums as a kernel may form them: fp32, a speaker's rows one after the other
    s32, cnt = np.zeros((K, D), dtype=np.float32), np.zeros(K, dtype=np.int64)
    for E, lab in c["calls"]:
        s32, cnt = er.accumulate_ref(s32, cnt, E, lab, dtype=np.float32)
    assert s32.dtype == np.float32 and (np.abs(s32 - c["sums"]) <= c["sums_bound"]).all()
    scores32 = er.scores_ref(c["E"], c["labels"], er.finalize_ref(s32, cnt), cnt)
    err = float(np.abs(scores32 - c["scores"]).max())
    print(f"{name}: scores from fp32 sequential sums differ by {err:.2e} (half the gate: {ec.GATE / 2:.1e})")
    assert err <= ec.GATE / 2
    m = er.margin(c["scores"], c["labels"], c["cnt"], ec.reference_thresholds())
    print(f"{name}: margin to the reference thresholds {m:.2e} (needs {ec.MARGIN:.1e})")
    assert m >= ec.MARGIN
    # the classes of trial rows the case is there for
    scored, target, enrolled = er.classes(c["labels"], c["cnt"], c["R"])
    if c["R"] >= 8:
        assert (~scored).sum() >= 2 and (scored & (target < 0)).sum() >= 3 and (target >= 0).sum() >= 3
        assert np.isnan(c["E"][~scored]).all() and np.isfinite(c["E"][scored]).all()
