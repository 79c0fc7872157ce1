"""Cohorts for the banks and trial sets of tests/enroll_cases.py (a plain helper module, no fixtures, no GPU):
tests/test_snorm_cpu.py licenses them, tests/test_gpu_snorm.py runs them.  Every array is made once and read-only.

Each case of enroll_cases.VALUE_CASES is paired with a cohort of its dimension; the cohort sizes cross the 16-column tile
(15, 17), the group of four accumulators (67), two of them (130) and the 256 columns one pass of the select kernel's
threads takes (300); C = 1 is the cohort of one.  Cohort speaker c is a member iff c % 8 != 4; its count is 1 .. 3, a
non-member's 0 or -1 and a non-member's model row is NaN.  Members are unit vectors round centres of their own (a cohort
is a disjoint set of speakers).  The seeds were chosen on the CPU so that, wherever at least five scores are taken, the
float64 spread of every scored row and every enrolled model is at least MIN_STD (tests/test_snorm_cpu.py asserts it, the
GPU test asserts it again before it launches).
"""
import functools

import numpy as np

import enroll_cases as ec
import enroll_ref as er
import snorm_ref as sr

MIN_STD = 1e-3
EPS_STD = sr.EPS_STD
# name: (C, seed)
COHORTS = {
    "K1_D36_R1": (1, 101),
    "K15_D100_R16": (15, 102),
    "K16_D256_R17": (17, 103),
    "K17_D7_R63": (67, 104),
    "K67_D260_R64": (130, 105),
    "K130_D36_R65": (300, 106),
    "K130_D256_R130": (300, 108),
    "K16_D100_R130": (67, 108),
}


def members_of(C):
    return np.arange(C) % 8 != 4


def make_cohort(C, D, seed):
    """-> cohort (C, D) float32 with NaN rows for the non-members, ccnt (C,) int32."""
    rng = np.random.default_rng(seed)
    member = members_of(C)
    centre = rng.standard_normal((C, D))
    cohort = ec.unit_rows(rng, centre, np.arange(C))
    cohort[~member] = np.nan
    ccnt = np.where(member, 1 + np.arange(C) % 3, -(np.arange(C) % 2)).astype(np.int32)
    return cohort, ccnt


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: C, cohort, ccnt, member, and the float64 references scores_rows (R, C) of the case's trial rows and
    scores_models (K, C) of the case's reference models against the cohort."""
    C, seed = COHORTS[name]
    c = ec.case(name)
    cohort, ccnt = make_cohort(C, c["D"], seed)
    return ec.frozen(dict(C=C, cohort=cohort, ccnt=ccnt, member=ccnt > 0,
                          scores_rows=er.scores_ref(c["E"], c["labels"], cohort, ccnt),
                          scores_models=er.scores_ref(c["models"], np.where(c["cnt"] > 0, 0, -1), cohort, ccnt)))


def n_tops(name):
    """1, 2, 5, 64, the member count and ten above it."""
    m = int(case(name)["member"].sum())
    return sorted({1, 2, 5, 64, m, m + 10})


def taken(name, n_top):
    return min(n_top, int(case(name)["member"].sum()))


@functools.lru_cache(maxsize=None)
def stats_ref(name, n_top):
    """-> (row stats (R, 2), model stats (K, 2)) in float64."""
    c, s = ec.case(name), case(name)
    rows = sr.cohort_stats_ref(s["scores_rows"], s["member"], n_top, c["labels"] >= 0)
    models = sr.cohort_stats_ref(s["scores_models"], s["member"], n_top, c["cnt"] > 0)
    rows.setflags(write=False)
    models.setflags(write=False)
    return rows, models


def licensed(name, n_top):
    """The (case, n_top) that are compared with float64 through the normalisation: at least five scores are taken.  With one
    the spread is eps_std and the normalised score is the raw one magnified 1e5 times, rounding and all; with two it is
    half the gap between a row's two best scores, which falls below MIN_STD on some of 130 rows for almost any seed.
    Those are held bit for bit against the float32 restatement only."""
    return taken(name, n_top) >= 5


def assert_licence(name, n_top):
    """The smallest reference spread on either side, asserted >= MIN_STD."""
    c = ec.case(name)
    rows, models = stats_ref(name, n_top)
    lo = min(float(rows[c["labels"] >= 0, 1].min()), float(models[c["cnt"] > 0, 1].min()))
    assert lo >= MIN_STD, f"{name} n_top {n_top}: a reference spread of {lo:.3e} is below {MIN_STD:.0e}"
    return lo


# ---- hand-made cohorts for the case K130_D36_R65 (D = 36) -------------------------------------------------------------------
TIE_CASE = "K130_D36_R65"
TIE_AT = (3, 67, 129)
TIE_ROWS = 10


@functools.lru_cache(maxsize=None)
def tie_cohort():
    """C = 130: bit-equal models at 3, 67 and 129 (all members), and a trial set whose first TIE_ROWS rows stand next to
    that model, so that its three equal scores are their best: n_top = 1 and 2 cut through the tie there, and larger n_top
    do wherever the tied score is the n-th.  The other rows are the case's trial rows."""
    c = ec.case(TIE_CASE)
    cohort, ccnt = make_cohort(130, c["D"], 211)
    cohort = cohort.copy()
    for at in TIE_AT[1:]:
        cohort[at] = cohort[TIE_AT[0]]
    rng = np.random.default_rng(212)
    E = np.array(c["E"][:40])
    labels = np.array(c["labels"][:40])
    near = cohort[TIE_AT[0]][None, :] + 0.05 * rng.standard_normal((TIE_ROWS, c["D"])).astype(np.float32)
    E[:TIE_ROWS] = near / np.linalg.norm(near, axis=1, keepdims=True)
    labels[:TIE_ROWS] = 0
    return ec.frozen(dict(C=130, D=c["D"], cohort=cohort, ccnt=ccnt, member=ccnt > 0, E=E.astype(np.float32), labels=labels))


@functools.lru_cache(maxsize=None)
def inf_cohort():
    """C = 17: element 0 of member 2's model is +inf and element 0 of every trial row is 0, so that member's score is NaN
    (0 x inf) for every row: behind every number.  14 finite scores and one NaN per row."""
    c = ec.case(TIE_CASE)
    cohort, ccnt = make_cohort(17, c["D"], 213)
    cohort = cohort.copy()
    cohort[2, 0] = np.inf
    E = np.array(c["E"][:20])
    E[:, 0] *= 0                       # (the ignored rows stay NaN)
    return ec.frozen(dict(C=17, D=c["D"], cohort=cohort, ccnt=ccnt, member=ccnt > 0, E=E,
                          labels=np.array(c["labels"][:20]), finite=int((ccnt > 0).sum()) - 1))


@functools.lru_cache(maxsize=None)
def empty_cohort():
    """C = 67 without a member: every count is 0 or negative and every model row NaN."""
    c = ec.case(TIE_CASE)
    cohort = np.full((67, c["D"]), np.nan, dtype=np.float32)
    ccnt = (-(np.arange(67) % 3)).astype(np.int32)
    return ec.frozen(dict(C=67, D=c["D"], cohort=cohort, ccnt=ccnt, member=ccnt > 0, E=np.array(c["E"][:20]),
                          labels=np.array(c["labels"][:20])))


def normed_thresholds(T, lo=-6.0, hi=12.0, seed=7):
    """T non-decreasing thresholds over the range of normalised scores, with repeats."""
    rng = np.random.default_rng(seed + T)
    return np.sort(rng.choice(rng.uniform(lo, hi, max(1, T // 2)), size=T)) if T > 1 else np.array([1.0])
