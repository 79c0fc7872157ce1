"""Inputs and float64 references of the enrolment / verification tests (a plain helper module, no fixtures, no GPU):
tests/test_enroll_cpu.py licenses them, tests/test_gpu_enroll.py runs them.  Every reference is computed once and read-only.

A case is a bank of K speakers of dimension D filled over TWO enrolment calls, and R trial rows.  Rows per speaker in the
first call cycle through (65, 1, 2, 64, 0, 3, 0, 5) -- one row enrols, 64 and 65 are either side of the 64-index chunk of
the accumulate kernel -- and in the second through (0, 3, 0, 1, 0, 0, 2, 4): speakers 4 mod 8 are never enrolled, speakers
6 mod 8 only by the second call, most are absent from one of the two; no speaker passes 70 rows.  Each call also holds rows
labelled -1, K and INT_MIN, filled with NaN.  Rows are unit vectors centre[speaker] + 0.5 noise, as rowlist_cases.inputs
makes them.  The trial rows are labelled with enrolled speakers in turn, except: row 1 is ignored (-1, NaN), row 3 an
unknown speaker (INT_MAX), row 5 the speaker K, row 6 a speaker that is not enrolled, row 7 ignored (INT_MIN, NaN), and the
last row of a set of 17 or more is ignored too.
"""
import functools

import numpy as np

import enroll_ref as er

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FIRST = (65, 1, 2, 64, 0, 3, 0, 5)
SECOND = (0, 3, 0, 1, 0, 0, 2, 4)
GATE = 3e-6
MARGIN = 4 * GATE

# name: (K, D, R, seed).  D: 36, 100, 256 are the three register-resident forms of the rows kernel (36 and 100 end in a
# zero-padded step), 7 and 260 take the plain loop.  K crosses the 16-speaker tile (15, 16, 17), the group of four
# accumulators = the LDS staging tile (67) and two of them (130).  R crosses the wave's 16 rows and the workgroup's 64.
VALUE_CASES = {
    "K1_D36_R1": (1, 36, 1, 11),
    "K15_D100_R16": (15, 100, 16, 12),
    "K16_D256_R17": (16, 256, 17, 13),
    "K17_D7_R63": (17, 7, 63, 14),
    "K67_D260_R64": (67, 260, 64, 15),
    "K130_D36_R65": (130, 36, 65, 16),
    "K130_D256_R130": (130, 256, 130, 17),
    "K16_D100_R130": (16, 100, 130, 18),
}
# The counts of EVERY case are compared with the float64 reference's: the seeds were chosen on the CPU so that every counted
# reference score stays at least MARGIN from each of the 50 reference thresholds (2.3e-5 at the least, K17_D7_R63;
# tests/test_enroll_cpu.py asserts it, the GPU test asserts it again before it launches).


def unit_rows(rng, centre, cls):
    x = centre[cls] + 0.5 * rng.standard_normal((len(cls), centre.shape[1]))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32)


def enroll_call(rng, centre, K, per_speaker):
    """One enrolment call: (E, labels), shuffled; three NaN rows labelled outside the bank among them."""
    lab = np.concatenate([np.repeat(np.arange(K), per_speaker), [-1, K, I32_MIN]]).astype(np.int64)
    lab = lab[rng.permutation(len(lab))]
    ok = er.valid_rows(lab, K)
    E = unit_rows(rng, centre, np.where(ok, lab, K))
    E[~ok] = np.nan
    return E, lab.astype(np.int32)


def trial_set(rng, centre, K, R, cnt):
    enrolled = np.flatnonzero(cnt > 0)
    lab = enrolled[np.arange(R) % len(enrolled)].astype(np.int64)
    unenrolled = np.flatnonzero(cnt <= 0)
    special = {1: -1, 3: I32_MAX, 5: K, 6: int(unenrolled[0]) if len(unenrolled) else K + 5, 7: I32_MIN}
    for pos, v in special.items():
        if pos < R:
            lab[pos] = v
    if R >= 17:
        lab[R - 1] = -1
    inside = (lab >= 0) & (lab < K)
    E = unit_rows(rng, centre, np.where(inside, lab, K))
    E[lab < 0] = np.nan
    return E, lab.astype(np.int32)


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: K, D, calls ((E, labels), (E, labels)), E, labels (the trials), and the float64 reference sums, cnt, models,
    scores, sums_bound."""
    K, D, R, seed = VALUE_CASES[name]
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((K + 1, D))
    calls = tuple(enroll_call(rng, centre, K, np.array([pat[s % 8] for s in range(K)])) for pat in (FIRST, SECOND))
    sums, cnt = np.zeros((K, D)), np.zeros(K, dtype=np.int64)
    for E, lab in calls:
        sums, cnt = er.accumulate_ref(sums, cnt, E, lab)
    E, lab = trial_set(rng, centre, K, R, cnt)
    models = er.finalize_ref(sums, cnt)
    for c in calls:
        for a in c:
            a.setflags(write=False)
    return frozen(dict(K=K, D=D, R=R, calls=calls, E=E, labels=lab, sums=sums, cnt=cnt.astype(np.int32), models=models,
                       scores=er.scores_ref(E, lab, models, cnt), sums_bound=er.sums_bound(calls, K, D)))


def reference_thresholds():
    from speaker_embedding_ge2e_loss_amd.evaluation import THRESHOLDS
    return np.asarray(THRESHOLDS, dtype=np.float64)


def thresholds_of(T, seed=5):
    """T non-decreasing thresholds: the reference's table for T = 50, else seeded values with repeats."""
    if T == 50:
        return reference_thresholds()
    rng = np.random.default_rng(seed + T)
    return np.sort(rng.choice(rng.uniform(-0.2, 1.0, max(1, T // 2)), size=T))
