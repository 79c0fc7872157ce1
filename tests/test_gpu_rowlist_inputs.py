"""GPU: the wide and the masked labelled loss (ge2e_loss_fwd_bwd_labeled_wide, ge2e_loss_fwd_bwd_labeled_masked) on inputs that
the row-list tests had never fed them: the golden vectors of the reference project as shuffled row lists, and degenerate
rows among ragged counts.  tests/rowlist_cases.py builds the inputs; tests/test_rowlist_cases.py holds them, without a GPU,
to what they are named for.

References, never the code under test: the golden files' float64 numbers; tests/masked_ref.py (torch autograd in float64).
Every C call goes through the guarded buffers of tests/guarded.py (the `run` helpers of test_gpu_labeled_wide.py,
test_gpu_masked.py and test_gpu_ragged.py).

Gates.  Golden vectors: test_gpu_ragged.check(strict=True) on the fixture's rows, as test_gpu_ragged.py holds the ragged
entry; g8_degenerate as it is held there.  Degenerate rows: the two-part rule of `two_part` below.  The wide entry against
the masked one: the same rules at factor 2 (two fp32 results); the masked entry against ge2e_loss_fwd_bwd_ragged on the
compacted rows: bit for bit.  The rows that do not count: exact +0, whatever they hold.  `-s` prints every figure before it
is asserted; profiles/rowlist_inputs_gate.txt keeps the worst of them.
"""
import numpy as np
import pytest
import torch

import rowlist_cases as rc
from conftest import golden_names
from test_gpu_labeled_wide import run as run_wide
from test_gpu_masked import KEYS, check_masked, is_zero, ragged_on_compacted
from test_gpu_masked import run as run_masked
from test_gpu_ragged import BIAS, GT, LT, VARIANTS, W, batch_of, check, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from speaker_embedding_ge2e_loss_amd import _lib
    return _lib.load()


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

    def on_fixture_rows(o):     # the outputs of the fixture's rows in the fixture's order: what check(strict=True) is worded for
        return dict(o, per=o["per"][counted], dE=o["dE"][counted])

    fixture = on_fixture_rows(ref)
    rule = g8_rule if "degenerate" in name else (lambda o, r, what, factor=1.0: check(o, r, what, strict=True, factor=factor))
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
def two_part(o, ref, deg, active_row, what, factor=1.0):
    """The gate where one speaker's gradients are 1e6 to 1e9 times the others':
      loss rtol 1e-5, and dE on the degenerate speaker's rows max-abs <= 1e-5 max|dE_ref| (the rule of g8_degenerate);
      every other speaker's rows at the ordinary row bound of test_gpu_ragged.check, max-abs <= 4e-5 max(1, max|dE_ref| over
      THOSE rows), so that the large entries cannot hide them, and per there at check's per bound: these rows get terms of
      ordinary size only."""
    rest = active_row & ~deg
    dref = np.asarray(ref["dE"], np.float64)
    top, plain = float(np.abs(dref).max()), max(1.0, float(np.abs(dref[rest]).max()))
    derr, rerr = float(np.abs(o["dE"][deg] - dref[deg]).max()), float(np.abs(o["dE"][rest] - dref[rest]).max())
    lerr, lref = abs(float(o["loss"]) - float(ref["loss"])), abs(float(ref["loss"]))
    per_ref = np.asarray(ref["per"], np.float64)[rest]
    pshare = float((np.abs(o["per"][rest] - per_ref) / (factor * (2e-5 + 20 * LT * np.abs(per_ref)))).max())
    print(f"{what}: loss {lerr:.3e} / {factor * 1e-5 * lref:.3e}  per worst share {pshare:.3f}"
          f"  dE degenerate rows max-abs {derr:.3e} / {factor * 1e-5 * top:.3e}  other rows max-abs {rerr:.3e} / {factor * 4 * GT * plain:.3e}")
    assert lerr <= factor * 1e-5 * lref, f"{what}: loss {float(o['loss'])} vs {float(ref['loss'])}"
    assert derr <= factor * 1e-5 * top, f"{what}: dE of the degenerate speaker's rows {derr} of {top}"
    assert rerr <= factor * 4 * GT * plain, f"{what}: dE of the other speakers' rows {rerr}"
    assert pshare <= 1.0, f"{what}: per of the other speakers' rows"


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
