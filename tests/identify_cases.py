"""Inputs of the identification tests (a plain helper module, no fixtures, no GPU): tests/test_identify_cpu.py licenses them,
tests/test_gpu_identify.py runs them.  Everything is computed once and read-only.

The banks and trial sets are those of enroll_cases.VALUE_CASES.  Each case has two label vectors: the case's own (a row's
target is the speaker it was drawn from, with the ignored rows and the unknown, unenrolled and out-of-bank labels of
enroll_cases.trial_set) and `random_labels`: every scored row gets a random ENROLLED target (seeded), so that ranks spread
over the whole list and beyond it.  A row is DECIDED where its target's float64 score keeps at least enroll_cases.MARGIN
from every other enrolled speaker's: there the rank is the float64 reference's whatever the fp32 rounding did.  At most
UNDECIDED_CAP of a label vector's rows with a target may be undecided.
"""
import functools

import numpy as np

import enroll_cases as ec
import enroll_ref as er
import identify_ref as ir

TOPS = (1, 5, 32)          # 32 = GE2E_IDENTIFY_MAX_TOP exceeds the enrolled count of the small banks: -1 / -inf tails
SEED = 3
UNDECIDED_CAP = 0.05


def slices_of(K):
    """0 = the product's choice, then forced: one slice, two, three, and one per group of 64 speakers."""
    return sorted({0, 1, 2, 3, -(-K // 64)})


@functools.lru_cache(maxsize=None)
def random_labels(name):
    c = ec.case(name)
    rng = np.random.default_rng(SEED)
    enrolled = np.flatnonzero(c["cnt"] > 0)
    lab = np.array(c["labels"])
    scored = lab >= 0
    lab[scored] = enrolled[rng.integers(0, len(enrolled), int(scored.sum()))]
    lab.setflags(write=False)
    return lab


def label_vectors(name):
    return {"own": ec.case(name)["labels"], "random": random_labels(name)}


@functools.lru_cache(maxsize=None)
def undecided(name, which):
    """-> (number of undecided rows, number of rows with a target, decided (R,) bool)."""
    c = ec.case(name)
    lab = label_vectors(name)[which]
    _, target, _ = er.classes(lab, c["cnt"], c["R"])
    dec = ir.decided(c["scores"], lab, c["cnt"], ec.MARGIN)
    dec.setflags(write=False)
    return int(((target >= 0) & ~dec).sum()), int((target >= 0).sum()), dec


def assert_cap(name, which):
    n, of, _ = undecided(name, which)
    assert n <= UNDECIDED_CAP * of, f"{name} / {which}: {n} of {of} rows with a target are undecided"
    return n, of


@functools.lru_cache(maxsize=None)
def tie_bank(cnt67=1):
    """The hand-made bank of the tie tests, passed to ge2e_identify directly: K = 130, D = 36, unit models of which 3, 67
    and 129 are equal bit for bit (either side of the slice boundaries at 64 and 128); everybody enrolled except 5 and,
    with cnt67 = 0, 67.  Trial rows: 0 and 4 near the tied model (the three tie for the first place), 1 all zero (every
    score is eps), 2 NaN and scored, 3 and 9 NaN and ignored, the rest random; labels with targets 3, 67 and 129 on the
    tied rows, an unenrolled target (5), one past the bank (130), and random enrolled ones."""
    K, D, R = 130, 36, 21
    rng = np.random.default_rng(130)
    models = rng.standard_normal((K, D))
    models /= np.linalg.norm(models, axis=1, keepdims=True)
    models = models.astype(np.float32)
    models[67] = models[3]
    models[129] = models[3]
    cnt = np.ones(K, dtype=np.int32)
    cnt[5] = 0
    cnt[67] = cnt67
    E = rng.standard_normal((R, D)).astype(np.float32)
    E[0] = models[3] + 0.01 * rng.standard_normal(D).astype(np.float32)
    E[4] = 2.0 * models[3]
    E[1] = 0.0
    E[[2, 3, 9]] = np.nan
    labels = rng.integers(0, K, R).astype(np.int32)
    labels[:10] = [129, 7, 3, -1, 67, 5, 130, 3, ec.I32_MAX, ec.I32_MIN]
    assert np.array_equal(models[3].view(np.uint32), models[67].view(np.uint32))
    return ec.frozen(dict(K=K, D=D, R=R, models=models, cnt=cnt, E=E, labels=labels))
