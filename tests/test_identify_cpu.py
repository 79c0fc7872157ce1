"""CPU: the host side of identification -- ge2e_identify_workspace_bytes / ge2e_identify and their selftest forms,
evaluation.identification_rates: declared, exported and bound, the workspace size, every error code and the order of the
checks (fake pointers: every call fails a check, nothing is launched).  tests/identify_ref.py, the reference of the GPU
tests, is held to hand-made matrices, and the inputs of tests/identify_cases.py are licensed for the GPU test of ranks
against float64: at most 5 % of a label vector's rows with a target are undecided."""
import ctypes
import re

import numpy as np
import pytest

import enroll_cases as ec
import enroll_ref as er
import identify_cases as ic
import identify_ref as ir
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build
from speaker_embedding_ge2e_loss_amd import evaluation as EV
from speaker_embedding_ge2e_loss_amd import functional as GF

SYMS = ("ge2e_identify_workspace_bytes", "ge2e_identify", "ge2e_selftest_identify_workspace_bytes",
        "ge2e_selftest_identify_slices")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -6
I, F, P, Z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
NAN, INF = np.nan, np.inf


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert "#define GE2E_IDENTIFY_MAX_TOP 32" in text and GF.IDENTIFY_MAX_TOP == 32
    ident = [P, P, P, P, I, I, I, I, F, F, P, P, P, P, P, Z, P]
    assert _lib.PROTOTYPES["ge2e_identify_workspace_bytes"] == (Z, [I] * 4)
    assert _lib.PROTOTYPES["ge2e_identify"] == (I, ident)
    assert _lib.PROTOTYPES["ge2e_selftest_identify_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.PROTOTYPES["ge2e_selftest_identify_slices"] == (I, ident + [I])
    assert GF._ENTRIES["identify"].entry == "ge2e_identify" and GF._ENTRIES["identify"].tag == ("identify",)
    assert hasattr(EV.SpeakerBank, "identify") and hasattr(EV, "evaluate_identification")


def slices_of(K, R, want=0, W=512):
    """The split as the header states it: S = clamp(ceil(W / tiles), 1, ceil(K / 64)), slices of ceil(G / S) groups, and
    only those that start inside the bank."""
    G, tiles = -(-K // 64), -(-R // 64)
    S = min(max(want if want > 0 else -(-W // tiles), 1), G)
    length = -(-G // S)
    return -(-G // length)


def test_workspace_bytes(lib):
    f, g = lib.ge2e_identify_workspace_bytes, lib.ge2e_selftest_identify_workspace_bytes
    for K, R, D, k in ((1, 1, 1, 1), (130, 65, 36, 5), (1251, 16384, 256, 5), (262144, 4096, 256, 5), (262144, 16, 256, 32),
                       (100, 70000, 64, 32), (65, 1, 7, 1)):
        got = f(K, R, D, k)
        S = slices_of(K, R)
        assert got > 0 and got % 256 == 0 and S * R * k * 8 <= got < S * R * k * 8 + 256, (K, R, D, k, got, S)
        assert got == g(K, R, D, k, 0) and f(K, R, 1, k) == f(K, R, 4096, k)      # the partial lists have no D
        for want in (1, 2, 3, 7, -(-K // 64), 10 ** 6):
            S = slices_of(K, R, want)
            assert S <= max(1, -(-K // 64)) and S * R * k * 8 <= g(K, R, D, k, want) < S * R * k * 8 + 256, (K, R, k, want)
        assert g(K, R, D, k, -4) == got                                           # nothing below 1 is forced
    assert slices_of(262144, 16) == 512 and slices_of(262144, 4096) == 8 and slices_of(1251, 16384) == 2
    assert slices_of(5 * 64, 1, 4) == 3                                           # five groups in slices of two: three slices
    for bad in ((0, 4, 8, 1), (4, 0, 8, 1), (4, 4, 0, 1), (-1, 4, 8, 1), (4, -4, 8, 1), (4, 4, -8, 1), (4, 4, 8, 0),
                (4, 4, 8, 33), (4, 4, 8, -1)):
        assert f(*bad) == 0 and g(*bad, 2) == 0, bad


@pytest.mark.parametrize("entry", ["ge2e_identify", "ge2e_selftest_identify_slices"])
def test_argument_validation_returns_codes_without_gpu(lib, entry):
    f = getattr(lib, entry)
    ok = dict(E=16, labels=16, models=16, cnt=16, K=130, R=20, D=8, k_top=5, eps_cos=1e-8, eps=1e-6, idx=16, score=16, rank=16,
              hist=16, ws=256, ws_bytes=1 << 40, stream=None)
    forced = entry.endswith("slices")

    def call(**kw):
        a = dict(ok, **kw)
        return f(*([a[k] for k in ok] + ([2] if forced else [])))

    for k in ("E", "models", "cnt", "idx"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(labels=None) == ERR_NULL                                        # rank and hist need labels
    assert call(labels=None, rank=None) == ERR_NULL and call(labels=None, hist=None) == ERR_NULL
    for k in ("K", "R", "D", "k_top"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    assert call(k_top=33) == ERR_SHAPE
    need = (lib.ge2e_selftest_identify_workspace_bytes(130, 20, 8, 5, 2) if forced
            else lib.ge2e_identify_workspace_bytes(130, 20, 8, 5))
    assert need > 0
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws=None, ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(ws=264) == ERR_WORKSPACE and call(ws=128) == ERR_WORKSPACE
    assert call(E=24) == ERR_ALIGN and call(E=20) == ERR_ALIGN and call(models=40) == ERR_ALIGN
    # the order: NULL, shape, workspace, alignment
    assert call(idx=None, K=0) == ERR_NULL and call(labels=None, k_top=33) == ERR_NULL and call(cnt=None, ws=None, E=24) == ERR_NULL
    assert call(R=0, ws=None) == ERR_SHAPE and call(k_top=33, ws=None, models=40) == ERR_SHAPE and call(D=0, E=24) == ERR_SHAPE
    assert call(ws=None, E=24) == ERR_WORKSPACE and call(ws_bytes=need - 1, models=40) == ERR_WORKSPACE


# ---- the reference on hand-made 3 x 5 matrices -----------------------------------------------------------------------------
def test_topk_ref_ties_and_zeros():
    scores = np.array([[0.5, 0.9, 0.5, 0.9, 0.1],
                       [0.0, -0.0, 0.3, -0.0, 0.0],
                       [-1.0, -INF, -1.0, INF, -2.0]], dtype=np.float32)
    cnt = [1, 1, 1, 1, 1]
    idx, score, rank, hist = ir.topk_ref(scores, [2, 4, 1], cnt, 5)
    assert idx.tolist() == [[1, 3, 0, 2, 4], [2, 0, 1, 3, 4], [3, 0, 2, 4, 1]]       # equal scores, -0 and +0: index order
    assert rank.tolist() == [3, 4, 4] and hist.tolist() == [0, 0, 0, 1, 2, 0]
    assert score.dtype == np.float32 and score[0].tolist() == [np.float32(v) for v in (0.9, 0.9, 0.5, 0.5, 0.1)]
    assert np.signbit(score[1]).tolist() == [False, False, True, True, False]          # the matrix's own bits come back
    idx, score, rank, hist = ir.topk_ref(scores, None, cnt, 2)                         # no labels: no target anywhere
    assert idx.tolist() == [[1, 3], [2, 0], [3, 0]] and rank.tolist() == [-1] * 3 and hist.tolist() == [0, 0, 0]


def test_topk_ref_nan_unenrolled_ignored_unknown_and_outside():
    scores = np.array([[0.2, NAN, 0.7, 9.0, -INF],
                       [NAN, NAN, NAN, 9.0, NAN],
                       [0.1, 0.2, 0.3, 9.0, 0.4]], dtype=np.float64)
    cnt = [2, 1, 1, 0, 3]                                # speaker 3 is not enrolled: never a candidate, whatever its score
    # k above the enrolled count: -1 / -inf tails; a NaN stands behind -inf; NaNs among themselves in index order
    idx, score, rank, hist = ir.topk_ref(scores, [1, 4, 0], cnt, 5)
    assert idx.tolist() == [[2, 0, 4, 1, -1], [0, 1, 2, 4, -1], [4, 2, 1, 0, -1]]
    assert score[0, :3].tolist() == [0.7, 0.2, -INF] and np.isnan(score[0, 3]) and score[0, 4] == -INF
    assert np.isnan(score[1, :4]).all() and score[1, 4] == -INF
    assert rank.tolist() == [3, 3, 3] and hist.tolist() == [0, 0, 0, 3, 0, 0] and hist.sum() == 3
    # an ignored row (all -1, never looked at), an unknown target (3: not enrolled; 5 and INT_MAX: outside the bank), and a
    # target outside the list
    for unknown in (3, 5, ec.I32_MAX):
        idx, score, rank, hist = ir.topk_ref(scores, [-1, unknown, 0], cnt, 2)
        assert idx.tolist() == [[-1, -1], [0, 1], [4, 2]] and (score[0] == -INF).all()
        assert rank.tolist() == [-1, -1, 2] and hist.tolist() == [0, 0, 1]
    idx, _, rank, hist = ir.topk_ref(scores, [ec.I32_MIN, 2, 2], cnt, 1)
    assert idx.tolist() == [[-1], [0], [4]] and rank.tolist() == [-1, 1, 1] and hist.tolist() == [0, 2]
    # nobody enrolled: every list is empty and no row has a target
    idx, score, rank, hist = ir.topk_ref(scores, [0, 1, 2], [0] * 5, 3)
    assert (idx == -1).all() and (score == -INF).all() and rank.tolist() == [-1] * 3 and not hist.any()


def test_decided_and_hist_of():
    scores = np.array([[0.5, 0.5 + 1e-6, 0.9], [0.5, 0.6, 0.9], [0.1, 0.2, 0.3]])
    dec = ir.decided(scores, [0, 0, -1], [1, 1, 1], ec.MARGIN)
    assert dec.tolist() == [False, True, False]
    assert ir.decided(scores, [0, 0, 1], [1, 0, 1], ec.MARGIN).tolist() == [True, True, False]   # the close one is not enrolled
    assert ir.hist_of([2, 0, -1, 2, 3], np.array([True, True, True, False, True]), 3).tolist() == [1, 0, 1, 1]


def test_identification_rates():
    assert EV.identification_rates([6, 2, 0, 2]) == [0.6, 0.8, 0.8]
    assert EV.identification_rates(np.array([0, 0, 0])) == [0, 0]
    assert EV.identification_rates([3, 0]) == [1.0]
    import torch
    assert EV.identification_rates(torch.tensor([1, 1, 2], dtype=torch.int64)) == [0.25, 0.5]


# ---- the licence of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.VALUE_CASES))
def test_cases_are_licensed_for_the_rank_test(name):
    c = ec.case(name)
    K, R = c["K"], c["R"]
    enrolled = c["cnt"] > 0
    for which, lab in ic.label_vectors(name).items():
        n, of = ic.assert_cap(name, which)
        print(f"{name} / {which}: {n} of {of} rows with a target are undecided")
        scored, target, _ = er.classes(lab, c["cnt"], R)
        assert np.array_equal(scored, c["labels"] >= 0)
        if which == "random":
            assert (target[scored] >= 0).all() and enrolled[target[scored]].all()     # every scored row: an enrolled target
    # the ranks of the random targets spread over the list and beyond it
    if R >= 60 and enrolled.sum() > 5:
        _, _, rank, hist = ir.topk_ref(c["scores"], ic.random_labels(name), c["cnt"], 5)
        print(f"{name}: ranks of the random targets {hist.tolist()}")
        assert hist[5] > 0 and hist[:5].sum() > 0 and hist.sum() == (rank >= 0).sum(), hist
    assert 32 > enrolled.sum() or K >= 67                                             # k = 32: tails on the small banks
    assert ic.slices_of(K)[0] == 0 and ic.slices_of(K)[-1] in (3, -(-K // 64))


def test_tie_bank():
    for cnt67 in (1, 0):
        t = ic.tie_bank(cnt67)
        m = t["models"].view(np.uint32)
        assert np.array_equal(m[3], m[67]) and np.array_equal(m[3], m[129]) and t["cnt"][67] == cnt67 and t["cnt"][5] == 0
        scores = er.scores_ref(np.nan_to_num(t["E"]), t["labels"], t["models"], t["cnt"])
        idx, _, rank, _ = ir.topk_ref(scores, t["labels"], t["cnt"], 5)
        want = [3, 67, 129] if cnt67 else [3, 129]
        assert idx[0, :len(want)].tolist() == want and idx[4, :len(want)].tolist() == want
        assert idx[1].tolist() == [0, 1, 2, 3, 4]                                       # the zero row: every score is eps
        assert rank[0] == len(want) - 1 and rank[4] == (1 if cnt67 else -1) and rank[5] == -1 and rank[6] == -1
        assert (idx[[3, 9]] == -1).all() and np.isnan(t["E"][[2, 3, 9]]).all()
