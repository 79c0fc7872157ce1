"""GPU: seeded random row lists (tests/rowlist_cases.cases: shapes, both variants, unit and raw rows, three scales, w in
(-4, 14), b in (-6, 3)) through the whole row-list family: the wide entry, the masked entry, and the ragged entry on the
compacted rows -- what tests/test_gpu_fuzz.py is to the dense path.  tests/test_rowlist_cases.py holds the committed list,
without a GPU, to reach every instantiation of the wide rows kernel, every cut of GC's K loop and every range of active
speakers.

Reference, never the code under test: tests/masked_ref.py (torch autograd in float64).  Every C call goes through the
guarded buffers of tests/guarded.py.  Gate: rowlist_harness.check_rows, unchanged, through rowlist_harness.check_masked; the
wide entry against the masked one at factor 2 (two fp32 results); the masked entry against the ragged one bit for bit.
A batch of a contrast case that falls under the tie rule of test_gpu_fuzz.py (rowlist_cases.ties) skips its dE / dw / db
comparisons only, never the forward.  `-s` prints every figure before it is asserted; profiles/rowlist_inputs_gate.txt
keeps the worst of them.
"""
import os

import numpy as np
import pytest

import rowlist_cases as rc
from capi import lib  # noqa: F401
from rowlist_harness import KEYS, batch_of, check_masked, check_rows, poisoned, ragged_on_compacted, run_masked, run_wide, same_bits

pytestmark = pytest.mark.gpu

# (GE2E_ROWLIST_FUZZ_N / GE2E_ROWLIST_FUZZ_SEED: a longer one-off soak with other draws; the committed default is what the
# suite runs and what tests/test_rowlist_cases.py checks)
CASES = rc.cases(int(os.environ.get("GE2E_ROWLIST_FUZZ_N", rc.N_DEFAULT)), int(os.environ.get("GE2E_ROWLIST_FUZZ_SEED", rc.SEED_DEFAULT)))
FORWARD = ("loss", "per", "active")


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_random_row_lists(lib, case):
    B, N, R, D, n_active, n_lone, n_ignored, variant, kind, scale, w, b, _ = case
    E, labels = rc.case_inputs(case)
    refs = rc.case_references(case)                              # (finite, and active what was drawn: test_rowlist_cases.py)
    tied = rc.tied_batches(case)
    name = rc.case_id(case)
    print(f"{name}: w {w:.3f} b {b:.3f} lone {n_lone} ignored {n_ignored} tied batches {list(tied)}")
    bad = np.stack([poisoned(E[i], refs[i]["index"]) for i in range(B)])

    # the wide entry three ways: with a gradient; forward only; NaN / Inf on the rows that do not count over a 0x00 workspace
    full = run_wide(lib, E, labels, N, variant, True, 0xFF, w=w, b=b)
    fwd = run_wide(lib, bad, labels, N, variant, False, 0xFF, w=w, b=b)
    assert set(fwd) == set(FORWARD)
    for k in fwd:
        assert same_bits(fwd[k], full[k]), f"{name}: forward-only {k} differs"
    nan = run_wide(lib, bad, labels, N, variant, True, 0x00, w=w, b=b)
    for k in full:
        assert same_bits(nan[k], full[k]), f"{name}: {k} depends on a row that does not count, or on the workspace"
    masked = run_masked(lib, E, labels, N, variant, True, 0xFF, w=w, b=b)
    assert np.array_equal(masked["active"], full["active"])

    for i in range(B):
        # a tied batch: the forward only (the row's gradient may have moved to the other of the two centroids)
        keep = FORWARD if i in tied else KEYS + ("active",)
        o_wide, o_masked = ({k: batch_of(o, i)[k] for k in keep} for o in (full, masked))
        check_masked(o_wide, refs[i], f"[fuzz wide] {name} batch {i}")
        check_masked(o_masked, refs[i], f"[fuzz masked] {name} batch {i}")
        check_rows({k: o_wide[k] for k in keep if k != "active"}, {k: np.asarray(o_masked[k], np.float64) for k in keep if k != "active"},
                   f"[fuzz wide-vs-masked] {name} batch {i}", factor=2)
        want = ragged_on_compacted(lib, E[i], refs[i], variant, w=w, b=b)
        for k in KEYS:
            assert same_bits(masked[k][i:i + 1], want[k]), f"{name} batch {i}: masked {k} is not the ragged entry's on the compacted batch"
