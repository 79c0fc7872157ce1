"""CPU: the host side of score normalisation -- ge2e_cohort_stats, ge2e_verify_scores_normed and the selftest forms of the
former: declared, exported and bound, the workspace size, every error code and the order of the checks (fake pointers: every
call fails a check, nothing is launched).  tests/snorm_ref.py, the reference of the GPU tests, is held to hand-made
matrices, the Python surface raises as it says, and the inputs of tests/snorm_cases.py are licensed for the GPU test's
comparison with float64 through the normalisation."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import enroll_cases as ec
import snorm_cases as sc
import snorm_ref as sr
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build
from speaker_embedding_ge2e_loss_amd import evaluation as EV
from speaker_embedding_ge2e_loss_amd import functional as GF

SYMS = ("ge2e_cohort_stats_workspace_bytes", "ge2e_cohort_stats", "ge2e_verify_scores_normed",
        "ge2e_selftest_cohort_stats_workspace_bytes", "ge2e_selftest_cohort_stats_chunk")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -6
I, F, P, Z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
NAN, INF = np.nan, np.inf
MIB = 1 << 20


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert "#define GE2E_COHORT_MAX 65536" in text and GF.COHORT_MAX == 65536
    stats = [P, P, I, P, P, I, I, I, I, F, F, F, P, P, Z, P]
    assert _lib.PROTOTYPES["ge2e_cohort_stats_workspace_bytes"] == (Z, [I] * 4)
    assert _lib.PROTOTYPES["ge2e_cohort_stats"] == (I, stats)
    assert _lib.PROTOTYPES["ge2e_selftest_cohort_stats_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.PROTOTYPES["ge2e_selftest_cohort_stats_chunk"] == (I, stats + [I])
    verify = _lib.PROTOTYPES["ge2e_verify_scores"][1]
    assert _lib.PROTOTYPES["ge2e_verify_scores_normed"] == (I, verify[:9] + [P, P] + verify[9:])
    assert GF._ENTRIES["cohort"].entry == "ge2e_cohort_stats" and GF._ENTRIES["cohort"].tag == ("cohort",)
    assert GF._ENTRIES["cohort"].size_query == "ge2e_cohort_stats_workspace_bytes"


def chunk_rows_of(C, want=0, budget=32 * MIB):
    """The chunk as the header states it: floor(32 MiB / (4 C)) rounded down to 64 rows, at least 64; a forced chunk is
    rounded up to 64 rows."""
    if want > 0:
        return -(-want // 64) * 64
    return max(budget // (4 * C) // 64 * 64, 64)


def test_workspace_bytes(lib):
    f, g = lib.ge2e_cohort_stats_workspace_bytes, lib.ge2e_selftest_cohort_stats_workspace_bytes
    for C, R, D, n in ((1, 1, 1, 1), (300, 65, 36, 5), (5994, 16384, 256, 300), (5994, 1251, 256, 300), (65536, 4096, 256, 300),
                       (65536, 100, 7, 1), (17, 10 ** 6, 64, 400), (4097, 70000, 260, 64)):
        got = f(C, R, D, n)
        rows = min(chunk_rows_of(C), -(-R // 64) * 64)
        assert got > 0 and got % 256 == 0 and rows * C * 4 <= got < rows * C * 4 + 256, (C, R, D, n, got)
        assert got <= 32 * MIB + 256, (C, R, got)
        assert got == g(C, R, D, n, 0) == g(C, R, D, n, -3) and f(C, R, 1, n) == f(C, R, 4096, n) == f(C, R, D, 1)
        # independent of R beyond the chunk
        beyond = chunk_rows_of(C)
        assert f(C, beyond, D, n) == f(C, beyond + 1, D, n) == f(C, 2 ** 31 - 1, D, n)
        for want in (1, 64, 65, 200):
            rows = min(chunk_rows_of(C, want), -(-R // 64) * 64)
            assert rows * C * 4 <= g(C, R, D, n, want) < rows * C * 4 + 256, (C, R, want)
    assert chunk_rows_of(5994) == 1344 and chunk_rows_of(65536) == 128 and chunk_rows_of(1) == 8 * MIB
    for bad in ((0, 4, 8, 1), (4, 0, 8, 1), (4, 4, 0, 1), (4, 4, 8, 0), (-1, 4, 8, 1), (4, -4, 8, 1), (4, 4, -8, 1), (4, 4, 8, -1),
                (65537, 4, 8, 1), (2 ** 31 - 1, 4, 8, 1)):
        assert f(*bad) == 0 and g(*bad, 64) == 0, bad


@pytest.mark.parametrize("entry", ["ge2e_cohort_stats", "ge2e_selftest_cohort_stats_chunk"])
def test_cohort_stats_validation_returns_codes_without_gpu(lib, entry):
    f = getattr(lib, entry)
    ok = dict(X=16, sel=16, sel_min=0, cohort=16, ccnt=16, C=130, R=200, D=8, n_top=5, eps_cos=1e-8, eps=1e-6, eps_std=1e-5,
              stats=16, ws=256, ws_bytes=1 << 40, stream=None)
    forced = entry.endswith("chunk")

    def call(**kw):
        a = dict(ok, **kw)
        return f(*([a[k] for k in ok] + ([64] if forced else [])))

    for k in ("X", "cohort", "ccnt", "stats"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("C", "R", "D", "n_top"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    assert call(C=65537) == ERR_SHAPE
    need = (lib.ge2e_selftest_cohort_stats_workspace_bytes(130, 200, 8, 5, 64) if forced
            else lib.ge2e_cohort_stats_workspace_bytes(130, 200, 8, 5))
    assert need == (64 if forced else 256) * 130 * 4
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws=None, ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(ws=264) == ERR_WORKSPACE and call(ws=128) == ERR_WORKSPACE
    assert call(X=24) == ERR_ALIGN and call(X=20) == ERR_ALIGN and call(cohort=40) == ERR_ALIGN
    # the order: NULL, shape, workspace, alignment
    assert call(stats=None, C=0) == ERR_NULL and call(ccnt=None, ws=None, X=24) == ERR_NULL
    assert call(R=0, ws=None) == ERR_SHAPE and call(C=65537, ws=None, cohort=40) == ERR_SHAPE and call(n_top=0, X=24) == ERR_SHAPE
    assert call(ws=None, X=24) == ERR_WORKSPACE and call(ws_bytes=need - 1, cohort=40) == ERR_WORKSPACE


def test_verify_scores_normed_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_verify_scores_normed
    ok = dict(E=16, labels=16, models=16, cnt=16, K=130, R=20, D=8, eps_cos=1e-8, eps=1e-6, row_stats=16, model_stats=16, thr=16,
              T=50, scores=16, counts=16, trials=16, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("E", "models", "cnt", "row_stats", "model_stats"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(scores=None, counts=None) == ERR_NULL
    assert call(labels=None) == ERR_NULL and call(labels=None, counts=None) == ERR_NULL     # counts or trials without labels
    for k in ("K", "R", "D"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    assert call(T=-1) == ERR_SHAPE and call(T=4097) == ERR_SHAPE and call(T=0) == ERR_SHAPE and call(thr=None) == ERR_SHAPE
    assert call(K=65536, R=65536) == ERR_SHAPE                                                # counts past 2^31 - 1 trials
    assert call(E=24) == ERR_ALIGN and call(models=40) == ERR_ALIGN
    # the order: NULL, shape, alignment
    assert call(row_stats=None, K=0) == ERR_NULL and call(model_stats=None, E=24) == ERR_NULL
    assert call(D=0, E=24) == ERR_SHAPE and call(T=4097, models=40) == ERR_SHAPE


# ---- the reference on hand-made matrices -----------------------------------------------------------------------------------
def test_cohort_stats_ref_ties_zeros_and_nan():
    scores = np.array([[0.5, 0.9, 0.5, 0.9, 0.1, 7.0],
                       [0.0, -0.0, 0.3, -0.0, 0.0, 7.0],
                       [NAN, 0.25, NAN, 0.75, -INF, 7.0],
                       [1.0, 2.0, 3.0, 4.0, 5.0, NAN]], dtype=np.float32)
    member = [True] * 5 + [False]                         # column 5 is no member, whatever it scores
    s = sr.cohort_stats_ref(scores, member, 3)
    assert s[0].tolist() == pytest.approx([(0.9 + 0.9 + 0.5) / 3, np.std([0.9, 0.9, 0.5])], rel=1e-7)   # one of the two 0.5
    assert sr.cut_through_tie(scores, member, 3).tolist() == [True, True, False, False]
    assert s[1].tolist() == pytest.approx([0.1, np.std([0.3, 0, 0])], rel=1e-7)                          # -0 and +0 alike
    assert s[2, 0] == -INF and np.isnan(s[2, 1])                                                       # 0.75, 0.25, -inf
    assert s[3].tolist() == pytest.approx([4.0, np.std([5, 4, 3])])
    s = sr.cohort_stats_ref(scores, member, 2)
    assert s[0].tolist() == [pytest.approx(0.9, rel=1e-7), sr.EPS_STD] and s[2].tolist() == pytest.approx([0.5, 0.25])
    s = sr.cohort_stats_ref(scores, member, 4)             # NaN last: taken only when the numbers run out
    assert np.isnan(s[2]).all() and s[0].tolist() == pytest.approx([0.7, 0.2], rel=1e-6)
    for n in (5, 6, 50):                                   # n above the member count: the whole cohort
        s = sr.cohort_stats_ref(scores, member, n)
        assert s[3].tolist() == pytest.approx([3.0, np.sqrt(2.0)]) and np.isnan(s[2]).all()
        assert s[1].tolist() == pytest.approx([0.06, 0.12], rel=1e-6)
    assert sr.cohort_stats_ref(scores, member, 1)[:, 0].tolist()[:2] == [pytest.approx(0.9, rel=1e-7), pytest.approx(0.3, rel=1e-7)]
    assert (sr.cohort_stats_ref(scores, member, 1)[[0, 1, 3], 1] == sr.EPS_STD).all()


def test_cohort_stats_ref_no_members_and_unscored_rows():
    scores = np.array([[0.5, 0.9], [NAN, NAN], [0.1, 0.2]])
    assert sr.cohort_stats_ref(scores, [False, False], 3).tolist() == [[0, 1]] * 3
    s = sr.cohort_stats_ref(scores, [True, True], 2, scored=[True, False, True])
    assert s[1].tolist() == [0, 1] and s[0].tolist() == pytest.approx([0.7, 0.2]) and s[2].tolist() == pytest.approx([0.15, 0.05])
    assert np.signbit(s[1]).tolist() == [False, False]


def test_normed_f32_with_unit_tables_returns_its_input_bits():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (9, 14)).astype(np.float32)
    v[0, :4] = [0.0, -0.0, 1e-38, -1e-45]
    scored = np.arange(9) != 4
    enrolled = np.arange(14) % 5 != 2
    unit_r, unit_k = np.tile(np.float32([0, 1]), (9, 1)), np.tile(np.float32([0, 1]), (14, 1))
    unit_r[4] = NAN                                        # the statistics of what is not scored are never looked at
    unit_k[~enrolled] = NAN
    out = sr.normed_f32(v, unit_r, unit_k, scored, enrolled)
    want = np.where(scored[:, None] & enrolled[None, :], v, np.float32(0))
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # and a hand-made value: 0.5 ((0.75 - 0.25) / 0.5 + (0.75 - 0.5) / 0.125) = 1.5
    one = sr.normed_f32(np.float32([[0.75]]), np.float32([[0.5, 0.125]]), np.float32([[0.25, 0.5]]), [True], [True])
    assert one.tolist() == [[1.5]]
    assert sr.normed_f64([[0.75]], [[0.5, 0.125]], [[0.25, 0.5]], [True], [True]).tolist() == [[1.5]]
    b = sr.normed_bound([[0.75]], [[0.5, 0.125]], [[0.25, 0.5]], [True], [True], 3e-6)
    assert 0.5 * (3 * 3e-6 / 0.5 + 3 * 3e-6 / 0.125) < b[0, 0] < 2e-4


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_python_surface_exists_and_raises_as_stated():
    assert callable(GF.cohort_stats) and callable(GF.verify_scores_normed)
    sig = inspect.signature(GF.cohort_stats).parameters
    assert sig["n_top"].default == 300 and sig["select"].default is None and sig["select_min"].default == 0
    assert sig["eps_std"].default == 1e-5 and sig["workspace"].default is None
    assert inspect.signature(GF.verify_scores_normed).parameters["need_scores"].default is True
    sig = inspect.signature(EV.SpeakerBank.set_cohort).parameters
    assert sig["n_top"].default == 300 and sig["eps_std"].default == 1e-5
    assert inspect.signature(EV.SpeakerBank.score).parameters["normalize"].default is False
    assert inspect.signature(EV.SpeakerBank.verify).parameters["normalize"].default is False
    sig = inspect.signature(EV.evaluate_enrolled).parameters
    assert sig["cohort"].default is None and sig["n_top"].default == 300
    bank, other = EV.SpeakerBank(4, 8, "cpu"), EV.SpeakerBank(6, 8, "cpu")
    import torch
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="cohort"):
        bank.score(x, normalize=True)
    with pytest.raises(ValueError, match="cohort"):
        bank.verify(x, [0, 1, 2], normalize=True)
    with pytest.raises(TypeError):
        bank.set_cohort("a cohort")
    with pytest.raises(ValueError, match="dimension"):
        bank.set_cohort(EV.SpeakerBank(6, 9, "cpu"))
    with pytest.raises(ValueError, match="n_top"):
        bank.set_cohort(other, n_top=0)
    bank.set_cohort(other, n_top=7)
    assert bank._cohort[:2] == (other, 7) and bank._model_stats is None
    bank._model_stats = "stale"
    bank.set_cohort(other)                                  # set_cohort invalidates the model-side statistics
    assert bank._model_stats is None and bank._cohort[1:] == (300, 1e-5)
    # with a cohort the default table, one of cosines, is refused before anything is computed
    with pytest.raises(ValueError, match="thresholds"):
        EV.evaluate_enrolled(lambda m: m, [], [], 4, device="cpu", cohort=other)


# ---- the licence of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.VALUE_CASES))
def test_cases_are_licensed_for_the_comparison_through_the_normalisation(name):
    s, c = sc.case(name), ec.case(name)
    C = s["C"]
    assert C in (1, 15, 17, 67, 130, 300) and s["cohort"].shape == (C, c["D"])
    assert np.array_equal(s["member"], np.arange(C) % 8 != 4) and np.isnan(s["cohort"][~s["member"]]).all()
    assert np.isfinite(s["cohort"][s["member"]]).all() and (s["ccnt"][~s["member"]] <= 0).all()
    m = int(s["member"].sum())
    assert set(sc.n_tops(name)) == {1, 2, 5, 64, m, m + 10}
    for n_top in sc.n_tops(name):
        rows, models = sc.stats_ref(name, n_top)
        assert (rows[c["labels"] < 0] == [0, 1]).all() and (models[c["cnt"] <= 0] == [0, 1]).all()
        assert np.isfinite(rows).all() and np.isfinite(models).all()
        if sc.licensed(name, n_top):
            lo = sc.assert_licence(name, n_top)
            print(f"{name} n_top {n_top}: the smallest reference spread is {lo:.3e}")
        else:
            assert sc.taken(name, n_top) < 5
            if sc.taken(name, n_top) == 1:                  # one score: the spread is the floor
                assert (rows[c["labels"] >= 0, 1] == sc.EPS_STD).all() and (models[c["cnt"] > 0, 1] == sc.EPS_STD).all()
    assert {sc.COHORTS[n][0] for n in ec.VALUE_CASES} == {1, 15, 17, 67, 130, 300}
    assert any(sc.licensed(n, t) for n in ec.VALUE_CASES for t in sc.n_tops(n))


def test_hand_made_cohorts():
    t = sc.tie_cohort()
    m = t["cohort"].view(np.uint32)
    assert all(np.array_equal(m[3], m[at]) and t["member"][at] for at in sc.TIE_AT)
    import enroll_ref as er
    scores = er.scores_ref(t["E"], t["labels"], t["cohort"], t["ccnt"])
    near = np.arange(sc.TIE_ROWS)
    assert (scores[near].argmax(1) == 3).all() and (scores[near, 3] == scores[near, 67]).all()
    for n_top in (1, 2):                                    # three equal best scores, one or two of them taken
        assert sr.cut_through_tie(scores, t["member"], n_top)[near].all()
        assert (sr.cohort_stats_ref(scores, t["member"], n_top)[near, 1] == sc.EPS_STD).all()
    assert not sr.cut_through_tie(scores, t["member"], 3)[near].any()
    i = sc.inf_cohort()
    assert np.isinf(i["cohort"][2, 0]) and not i["E"][i["labels"] >= 0, 0].any() and i["member"][2] and i["finite"] == 14 == int(i["member"].sum()) - 1
    e = sc.empty_cohort()
    assert not e["member"].any() and np.isnan(e["cohort"]).all()
