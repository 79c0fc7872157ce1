"""CPU: the tables of tests/encoder_cases.py against what they are there for (no GPU, no launch).  Every condition rests on
the float64 reference alone, so a case of tests/test_gpu_encoder.py cannot pass by being insensitive to what it is named for;
if a seed misses a condition, the seed is changed, not the condition."""
import numpy as np
import pytest

import encoder_cases as ec
import encoder_ref as enc


def test_the_grid_covers_every_supported_pair_with_a_recurrence():
    pairs = sorted((H, L) for _, T, _, H, L, _ in ec.GRID.values() if T >= 2)
    assert pairs == [(H, L) for H in (128, 256) for L in (1, 2, 3, 4)]
    assert len(set(ec.SEEDS.get(n, 1000 + i) for i, n in enumerate(ec.TABLES))) == len(ec.TABLES)
    assert len(ec.TABLES) == len(ec.GRID) + len(ec.N_MELS_EDGES) + len(ec.D_EDGES)


@pytest.mark.parametrize("name", list(ec.GRID))
def test_the_top_layers_recurrence_shows_in_the_output(name):
    c = ec.case(name)
    gate = max(enc.gate(c["err_ref"]), ec.rows_gate(c["ref32"], c["ref"]))
    moved = enc.rel_err(ec.zeroed_top_recurrence(name), c["ref"])
    print(f"{name}: zeroing the top weight_hh moves the output by {moved:.3f}, gate {gate:.3e}")
    assert moved > 1000 * gate, (name, moved, gate)


@pytest.mark.parametrize("name", list(ec.TABLES))
def test_cases_are_finite_and_their_yardstick_is_float32s(name):
    c = ec.case(name)
    R, T, n_mels, H, L, D = c["shape"]
    assert c["x"].shape == (R, T, n_mels) and c["x"].dtype == np.float32 and 0.0 <= c["x"].min() and c["x"].max() < 0.96
    assert c["ref"].shape == (R, D) and np.isfinite(c["ref"]).all() and np.isfinite(c["raw"]).all()
    worst = ec.row_errs(c["ref32"], c["ref"]).max()
    assert c["err_ref"] <= worst and c["err_ref_raw"] > 0, (name, c["err_ref"], worst, c["err_ref_raw"])   # (a max over rows)
    assert c["err_ref"] > 0 or D == 1                                          # (D = 1 normalises to +-1 exactly)


def test_d1_has_both_signs_and_no_row_near_zero():
    raw = ec.case("h128_d1")["raw"]
    assert raw.shape == (3, 1) and (raw > 0).any() and (raw < 0).any() and np.abs(raw).min() >= 1e-3, raw.ravel()
    assert np.array_equal(ec.case("h128_d1")["ref"], np.sign(raw))


@pytest.mark.parametrize("at", ec.POISON_AT)
@pytest.mark.parametrize("name", list(ec.POISON_SHAPES))
def test_a_nan_poisons_its_row_of_the_reference_alone(name, at):
    clean, c = ec.case(name), ec.poisoned(name, at, "nan")
    others = np.arange(clean["shape"][0]) != at[0]
    assert np.isnan(c["x"]).sum() == 1 and np.isnan(c["x"][at])
    for k in ("ref", "raw"):
        assert np.isnan(c[k][at[0]]).all() and np.array_equal(c[k][others], clean[k][others]), (name, at, k)


@pytest.mark.parametrize("value", ["inf", "-inf"])
@pytest.mark.parametrize("at", ec.POISON_AT)
@pytest.mark.parametrize("name", list(ec.POISON_SHAPES))
def test_an_inf_saturates_the_gates_and_the_reference_stays_finite(name, at, value):
    clean, c = ec.case(name), ec.poisoned(name, at, value)
    others = np.arange(clean["shape"][0]) != at[0]
    assert np.isinf(c["x"]).sum() == 1 and c["x"][at] == ec.POISON_VALUES[value]
    for k in ("ref", "raw"):
        assert np.isfinite(c[k]).all() and np.array_equal(c[k][others], clean[k][others]), (name, at, value, k)
        assert not np.array_equal(c[k][at[0]], clean[k][at[0]])
    # torch's float32 path, the yardstick of the poisoned row, stays finite too; a case where it did not would have no
    # accuracy check on the GPU
    print(f"{name} {at} {value}: float32 yardstick of the poisoned row {ec.row_errs(c['ref32'], c['ref'])[at[0]]:.3e}")
    assert np.isfinite(c["ref32"]).all() and np.isfinite(c["raw32"]).all()


@pytest.mark.parametrize("shape", ec.PACK_SHAPES)
def test_integer_params_are_distinct_exact_and_counted(shape):
    n_mels, H, L, D = shape
    ps, expected = ec.integer_params(*shape)
    flat = enc.flat(ps)
    assert flat.size == 4 * H * (n_mels + H + 2) + (L - 1) * 4 * H * (2 * H + 2) + D * H + D
    weights = np.concatenate([p.ravel() for p in ps if p.ndim == 2])
    assert weights.min() == 1 and weights.max() == weights.size < 2 ** 24 and np.unique(weights).size == weights.size
    assert all((p == 0.5).all() for p in ps[3:-2:4]) and (ps[-1] < 0).all() and np.unique(ps[-1]).size == D
    sums = np.concatenate([ps[4 * l + 2] + ps[4 * l + 3] for l in range(L)])
    assert np.array_equal(expected, np.sort(np.concatenate([weights, sums, ps[-1]])))
    assert np.unique(expected).size == expected.size and not (expected == 0).any()
    assert expected.size < ec.packed_floats(*shape) or (n_mels % 16 == 0 and D % 16 == 0)
    assert (ec.packed_floats(*shape) > 4096 * 256) == (shape == ec.PACK_SHAPES[-1])
