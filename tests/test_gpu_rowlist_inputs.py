"""GPU: the wide and the masked labelled loss (ge2e_loss_fwd_bwd_labeled_wide, ge2e_loss_fwd_bwd_labeled_masked) on inputs that
the row-list tests had never fed them: the golden vectors of the reference project as shuffled row lists, and degenerate
rows among ragged counts.  tests/rowlist_cases.py builds the inputs; tests/test_rowlist_cases.py holds them, without a GPU,
to what they are named for.

References, never the code under test: the golden files' float64 numbers; tests/masked_ref.py (torch autograd in float64).
Every C call goes through the guarded buffers of tests/guarded.py (run_wide, run_masked and run_ragged of
tests/rowlist_harness.py).

Gates.  Golden vectors: rowlist_harness.check_rows(strict=True) on the fixture's rows, as test_gpu_ragged.py holds the ragged
entry; g8_degenerate as it is held there.  Degenerate rows: the two-part rule of rowlist_harness.two_part.  The wide entry against
the masked one: the same rules at factor 2 (two fp32 results); the masked entry against ge2e_loss_fwd_bwd_ragged on the
compacted rows: bit for bit.  The rows that do not count: exact +0, whatever they hold.  `-s` prints every figure before it
is asserted; profiles/rowlist_inputs_gate.txt keeps the worst of them.
"""
import numpy as np
import pytest

import rowlist_cases as rc
from capi import lib  # noqa: F401
from conftest import golden_names
from rowlist_harness import (BIAS, KEYS, VARIANTS, W, batch_of, check_masked, check_rows, is_zero, ragged_on_compacted, run_masked,
                             run_wide, same_bits, two_part)

pytestmark = pytest.mark.gpu


def as_ref(o):
    return {k: np.asarray(o[k], np.float64) for k in KEYS}


def zeros_and_active(o, idx, what):
    assert o["active"].tolist() == idx["active"].tolist(), f"{what}: active {o['active']} vs {idx['active']}"
    rest = ~idx["active_row"]
    for k in ("per", "dE"):
        assert is_zero(o[k][rest], plus=True), f"{what}: {k} is not +0 on a row that does not count"


def g8_rule(o, ref, what, factor=1.0):
    """test_gpu_ragged.test_golden_vectors_as_equal_counts on g8_degenerate: 1e8-scale gradients on the clamped rows, so dE is
    compared relative to its largest entry and the loss relatively."""
    err, top = float(np.abs(o["dE"] - ref["dE"]).max()), float(np.abs(ref["dE"]).max())
    lerr, lref = abs(float(o["loss"]) - float(ref["loss"])), abs(float(ref["loss"]))
    print(f"{what}: loss {lerr:.3e} / {factor * 1e-5 * lref:.3e}  dE max-abs {err:.3e} / {factor * 1e-5 * top:.3e}")
    assert err <= factor * 1e-5 * top, f"{what}: dE max-abs {err} of {top}"
    assert lerr <= factor * 1e-5 * lref, f"{what}: loss {float(o['loss'])} vs {float(ref['loss'])}"


# ---- 1. the golden vectors, rows shuffled, lone and ignored rows among them -------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_golden_vectors_as_row_lists(lib, name):
    E, labels, N, ref, w, b = rc.golden_rows(name)
    idx, counted = ref["index"], ref["counted"]

    def on_fixture_rows(o):     # the outputs of the fixture's rows in the fixture's order: what check_rows(strict=True) is worded for
        return dict(o, per=o["per"][counted], dE=o["dE"][counted])

    fixture = on_fixture_rows(ref)
    rule = g8_rule if "degenerate" in name else (lambda o, r, what, factor=1.0: check_rows(o, r, what, strict=True, factor=factor))
    masked = run_masked(lib, E[None], labels[None], N, "softmax", True, 0xFF, w=w, b=b)
    got = {"wide": batch_of(run_wide(lib, E[None], labels[None], N, "softmax", True, 0xFF, w=w, b=b), 0), "masked": batch_of(masked, 0)}
    for entry, o in got.items():
        zeros_and_active(o, idx, f"{name}/{entry}")
        rule(on_fixture_rows(o), fixture, f"[golden {entry}] {name}")
    rule(on_fixture_rows(got["wide"]), as_ref(on_fixture_rows(got["masked"])), f"[golden wide-vs-masked] {name}", factor=2.0)
    want = ragged_on_compacted(lib, E, ref, "softmax", w=w, b=b)
    for k in KEYS:
        assert same_bits(masked[k], want[k]), f"{name}: masked {k} is not the ragged entry's on the compacted batch"


# ---- 2. degenerate rows with ragged counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", list(rc.DEG_KINDS))
def test_degenerate_rows_among_ragged_counts(lib, kind, variant):
    E, labels, N, ref, deg = rc.degenerate_case(kind, variant)       # (finite, huge where it has to be: asserted there)
    idx = ref["index"]
    masked = run_masked(lib, E[None], labels[None], N, variant, True, 0xFF, w=W, b=BIAS)
    got = {"wide": batch_of(run_wide(lib, E[None], labels[None], N, variant, True, 0xFF, w=W, b=BIAS), 0), "masked": batch_of(masked, 0)}
    for entry, o in got.items():
        zeros_and_active(o, idx, f"{kind}/{variant}/{entry}")
        two_part(o, ref, deg, idx["active_row"], f"[degenerate {entry}] {kind}/{variant}")
        if kind not in rc.DEG_HUGE:
            # nothing is large here (rowlist_cases.degenerate_case asserts it), so the ordinary gate holds as well
            check_masked(o, ref, f"[degenerate {entry}] {kind}/{variant} ordinary gate")
    two_part(got["wide"], as_ref(got["masked"]), deg, idx["active_row"], f"[degenerate wide-vs-masked] {kind}/{variant}", factor=2.0)
    want = ragged_on_compacted(lib, E, ref, variant)
    for k in KEYS:
        assert same_bits(masked[k], want[k]), f"{kind}/{variant}: masked {k} is not the ragged entry's on the compacted batch"
