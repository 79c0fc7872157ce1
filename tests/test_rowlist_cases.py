"""CPU: the inputs of tests/rowlist_cases.py against what they are drawn for (no GPU, no launch).  The committed default
list of random cases must reach every instantiation of the wide rows kernel, every cut of GC's K loop and every range of
active speakers that the GPU test is there for; if a seed misses a condition, the seed is changed, not the condition.
"""
import collections

import numpy as np
import pytest

import rowlist_cases as rc
from conftest import golden_names, rel_fro

CASES = rc.cases()


def count(pred):
    return sum(1 for c in CASES if pred(c))


def test_default_list():
    assert len(CASES) == rc.N_DEFAULT == 48 and len(set(CASES)) == 48
    assert CASES == rc.cases(48, rc.SEED_DEFAULT) and CASES[:10] == rc.cases(10, rc.SEED_DEFAULT)
    for B, N, R, D, n_active, n_lone, n_ignored, variant, kind, scale, w, b, seed in CASES:
        assert 1 <= B <= 4 and 2 <= N <= 90 and 4 <= R <= 330 and D in rc.DS and n_active >= 2
        assert n_active + n_lone < N and 2 * n_active + n_lone + n_ignored <= R
        assert variant in ("softmax", "contrast") and kind in rc.KINDS and scale in rc.SCALES
        assert -4 <= w < 14 and -6 <= b < 3


def test_coverage_of_the_default_list():
    D, R, NACT = 3, 2, 4
    # the instantiations of wide_rows_kernel: <4>, <8>, <16> (D % 4 == 0, D <= 64, 128, 256), <0> for D % 4 != 0 and for D = 260
    assert count(lambda c: c[D] % 4 == 0 and c[D] <= 64) >= 3
    assert count(lambda c: c[D] % 4 == 0 and 64 < c[D] <= 128) >= 3
    assert count(lambda c: c[D] % 4 == 0 and 128 < c[D] <= 256) >= 3
    assert count(lambda c: c[D] % 4 != 0) >= 3
    assert count(lambda c: c[D] == 260) >= 3
    splits = collections.Counter(rc.wide_split(c[R]) for c in CASES)
    assert all(splits[s] >= 5 for s in (1, 2, 3)), splits
    assert count(lambda c: c[NACT] <= 16) >= 3 and count(lambda c: 17 <= c[NACT] <= 64) >= 3 and count(lambda c: c[NACT] > 64) >= 3
    assert count(lambda c: c[7] == "contrast") >= 10
    assert count(lambda c: c[10] < 0) >= 5
    for kind in rc.KINDS:
        assert count(lambda c: c[8] == kind) >= 8, kind
    for scale in rc.SCALES:
        assert count(lambda c: c[9] == scale) >= 8, scale


def test_wide_split_is_the_library_s():
    import os
    import re
    hpp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speaker_embedding_ge2e_loss_amd", "csrc",
                       "ge2e_labeled_wide.hpp")
    with open(hpp) as f:
        text = f.read()
    assert int(re.search(r"kWideSplitRows = (\d+);", text).group(1)) == 128
    assert int(re.search(r"kWideMaxSplit = (\d+);", text).group(1)) == 8
    assert [rc.wide_split(r) for r in (4, 128, 129, 256, 257, 330, 5000)] == [1, 1, 2, 2, 3, 3, 8]


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_reference_is_finite_and_active_is_what_was_drawn(case):
    B, N, R, D, n_active, n_lone, n_ignored = case[:7]
    E, labels = rc.case_inputs(case)
    assert E.shape == (B, R, D) and E.dtype == np.float32 and labels.shape == (B, R) and np.isfinite(E).all()
    assert B == 1 or not np.array_equal(labels[0], labels[1])
    norm = np.linalg.norm(E.astype(np.float64), axis=2) / case[9]
    assert np.allclose(norm, 1.0, atol=1e-6) if case[8] == "unit" else (norm.std() > 0.1 * norm.mean())
    for i, ref in enumerate(rc.case_references(case)):                    # (finite: case_references asserts it)
        idx = ref["index"]
        assert idx["active"].tolist() == [n_active, R - n_lone - n_ignored], f"batch {i}"
        assert int(((labels[i] < 0) | (labels[i] >= N)).sum()) == n_ignored
        assert np.abs(ref["dE"]).max() > 0 and not ref["dE"][~idx["active_row"]].any()


def test_at_most_two_contrast_cases_tie():
    tied = [rc.case_id(c) for c in CASES if rc.tied_batches(c)]
    print("tied:", tied)
    assert len(tied) <= 2, tied


def test_the_tie_rule_sees_a_tie():
    """Two speakers' rows mirrored about a third's: every row of that one has its two other similarities equal."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 6))
    mid = rng.standard_normal((3, 6))
    mid[:, 0] = 0.0
    flip = a * np.array([-1, 1, 1, 1, 1, 1.0])
    E = np.concatenate([a, flip, mid]).astype(np.float32)
    idx = rc.mr.index_ref(np.array([0, 0, 1, 1, 2, 2, 2]), 3)
    assert rc.ties(E, idx, 10.0, -5.0)
    E[2, 1] += 0.5
    assert not rc.ties(E, idx, 10.0, -5.0)


@pytest.mark.parametrize("name", golden_names())
def test_golden_rows(name):
    E, labels, N, ref, w, b = rc.golden_rows(name)
    g = rc.load_golden(name)
    n, m, d = g["E"].shape
    idx = ref["index"]
    rest = ~idx["active_row"]
    assert N == n + 3 and E.shape == (n * m + 5, d) and idx["active"].tolist() == [n, n * m] and rest.sum() == 5
    assert sorted(labels[rest].tolist()) == [-1, n, n + 1, n + 2, 2 ** 31 - 1]
    bad = E[np.isin(labels, [-1, n + 2, 2 ** 31 - 1])]
    assert np.isnan(bad).all(axis=1).sum() == 1 and (bad == np.inf).all(axis=1).sum() == 1 and (bad == -np.inf).all(axis=1).sum() == 1
    assert np.isfinite(E[labels == n]).all() and np.isfinite(E[labels == n + 1]).all()
    # the scattered rows are the fixture's, speaker by speaker, and the scattered numbers go with them
    c = ref["counted"]
    assert np.array_equal(E[c].reshape(n, m, d), g["E"]) and np.array_equal(labels[c], np.repeat(np.arange(n), m))
    assert np.array_equal(ref["per"][c].reshape(n, m), g["per64"]) and not ref["per"][rest].any() and not ref["dE"][rest].any()
    assert not np.array_equal(labels, np.sort(labels))
    if "degenerate" not in name:
        # the fixture's numbers are what masked_ref gives on the row list: two references that share no code
        mine = rc.mr.masked_loss(np.where(rest[:, None], 0, E), labels, N, w, b)
        # (a fixture without dE64 keeps the reference project's own float32 gradient)
        fro = rel_fro(ref["dE"], mine["dE"])
        print(f"{name}: loss {abs(mine['loss'] - ref['loss']):.2e} dE rel-fro {fro:.2e}")
        assert np.allclose(mine["loss"], ref["loss"], rtol=1e-9) and fro <= (1e-9 if "dE64" in g else 1e-6)


@pytest.mark.parametrize("variant", ("softmax", "contrast"))
@pytest.mark.parametrize("kind", list(rc.DEG_KINDS))
def test_degenerate_cases(kind, variant):
    E, labels, N, ref, deg = rc.degenerate_case(kind, variant)      # (finite, huge where it has to be: asserted there)
    spk = rc.DEG_KINDS[kind]
    assert deg.sum() == rc.DEG_COUNTS[spk] and np.array_equal(deg, labels == spk)
    rows = E[deg].astype(np.float64)
    norms = np.linalg.norm(rows, axis=1)
    total = rows.sum(axis=0)
    loo = (total - rows) / (len(rows) - 1)
    assert np.allclose(np.linalg.norm(E[~deg & (labels >= 0)].astype(np.float64), axis=1), 1.0, atol=1e-6)
    if kind == "zero_row":
        assert sorted(norms)[0] == 0.0 and sorted(norms)[1] > 0.9
    elif kind == "tiny_row":
        assert 0 < sorted(norms)[0] < rc.EPS_COS and np.float32(sorted(norms)[0]) ** 2 > np.finfo(np.float32).tiny
    elif kind == "identical_rows":
        assert len(rows) == 4 and (rows == rows[0]).all()
    elif kind == "loo_zero":
        assert len(rows) == 3 and (np.abs(loo).max(axis=1) == 0.0).sum() == 1 and np.array_equal(rows * 64, np.round(rows * 64))
    elif kind == "zero_centroid":
        assert len(rows) == 2 and not total.any() and np.array_equal(rows * 64, np.round(rows * 64))
