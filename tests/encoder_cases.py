"""Inputs and float64 references of the encoder's shape, edge and poison tests (a plain module, no fixtures, no GPU code);
tests/test_encoder_cases.py holds every table to what it is there for without a GPU.

    finish(c) / row_errs / rows_gate     the references and yardsticks of one case; the per-row error and its gate
    GRID / N_MELS_EDGES / D_EDGES        name -> (R, T, n_mels, H, L, D): every (H, L) with a recurrence; the n_mels and the D
                                         at which ge2e_encode takes another path
    case(name)                           one of those, built as tests/test_gpu_encoder.py builds its own
    POISON_SHAPES / POISON_AT / poisoned one NaN or +-Inf element in one row of a clean case
    zeroed_top_recurrence(name)          the float64 output with the top layer's weight_hh zeroed
    PACK_SHAPES / integer_params         parameters whose packed image can be counted: every value distinct and exact

Every case is built the same way: enc.random_params, uniform mels in [0, 0.96), encoder_ref in float64, and torch's CPU
float32 modules on the same inputs as the yardstick.  Whatever is expensive is computed once (functools.lru_cache), shared
and read-only."""
import functools

import numpy as np
import torch

import encoder_ref as enc

# ---- the tables ---------------------------------------------------------------------------------------------------------------
# every supported (H, L) at T > 1: 17 rows fill both 16-row halves of a tile and leave pad rows, 20 mels take the vector
# path with a partly filled second group
GRID = {f"h{H}_l{L}": (17, 5, 20, H, L, 24) for H in (128, 256) for L in (1, 2, 3, 4)}
# 1 and 3: the scalar path; 4: the vector path where only lane group 0 loads; 15 / 16 / 17: around a group of 16;
# 255 / 256: the upper limit, with more input groups than recurrent ones at H = 128
N_MELS_EDGES = {f"h{H}_mels{n}": (3, 2, n, H, 1, 8)
                for H, ns in ((128, (1, 3, 4, 15, 16, 17, 255, 256)), (256, (17, 256))) for n in ns}
# 1: a norm of one element; 15 / 16 / 17: around a projection tile; 127 / 128 / 129: the eighth wave's tile, and the first
# wave's second one; 255 / 256 at H = 128, L = 1: the projection plane is larger than the h planes
D_EDGES = {f"h{H}_d{D}": (3, 2, 12, H, 1, D)
           for H, ds in ((128, (1, 15, 16, 17, 127, 128, 129, 255, 256)), (256, (129, 256))) for D in ds}
TABLES = {**GRID, **N_MELS_EDGES, **D_EDGES}
# a seed is the case's place in TABLES (new cases go to the end of a new table) unless it is named here
SEEDS = {"h128_d1": 2002}         # D = 1: both signs of the raw projection among the three rows, none near zero

POISON_SHAPES = {"h128_l2": (33, 4, 13, 128, 2, 16), "h256_l4": (33, 4, 20, 256, 4, 24)}
# (row, frame, channel): the tile's first half, its second half, the tail tile's only row
POISON_AT = ((3, 0, 0), (20, 3, -1), (32, 1, 5))
POISON_VALUES = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}

# (n_mels, H, L, D) of the pack tests; only the last has more elements than one pass of the pack kernel's grid
PACK_SHAPES = ((13, 128, 1, 37), (20, 256, 2, 24), (256, 128, 1, 256), (80, 256, 3, 256))


# ---- references ---------------------------------------------------------------------------------------------------------------
def row_errs(a, ref):
    """The relative 2-norm error of every row."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)


def rows_gate(ref32, ref):
    """encoder_ref.gate on the worst row: 4 x the worst row of torch's CPU fp32 path, plus the same floor."""
    return enc.gate(float(row_errs(ref32, ref).max()))


def finish(c):
    """Adds to `params` and `x`: the float64 outputs `ref` (normalised) and `raw`, torch's CPU float32 outputs `ref32` and
    `raw32`, and their batch errors `err_ref` and `err_ref_raw`; every array read-only."""
    x64 = c["x"].astype(np.float64)
    with np.errstate(all="ignore"):                                            # (a poisoned input)
        c["ref"] = enc.encode_ref(c["params"], x64)
        c["raw"] = enc.encode_ref(c["params"], x64, normalize=False)
        c["ref32"] = enc.torch_encode(c["params"], c["x"], torch.float32)
        c["raw32"] = enc.torch_encode(c["params"], c["x"], torch.float32, normalize=False)
        c["err_ref"] = enc.rel_err(c["ref32"], c["ref"])
        c["err_ref_raw"] = enc.rel_err(c["raw32"], c["raw"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def build(shape, seed, wscale=1.0, xscale=1.0):
    R, T, n_mels, H, L, D = shape
    ps = enc.random_params(n_mels, H, L, D, seed=100 + seed, scale=wscale)
    x = (np.random.default_rng(200 + seed).uniform(0.0, 0.96, (R, T, n_mels)) * xscale).astype(np.float32)
    return finish(dict(shape=tuple(shape), params=ps, x=x))


@functools.lru_cache(maxsize=None)
def case(name):
    """Parameters, inputs, references and yardsticks of a case of TABLES or POISON_SHAPES."""
    if name in POISON_SHAPES:
        return build(POISON_SHAPES[name], 3000 + sorted(POISON_SHAPES).index(name))
    return build(TABLES[name], SEEDS.get(name, 1000 + list(TABLES).index(name)))


@functools.lru_cache(maxsize=None)
def poisoned(name, at, value):
    """case(name) with POISON_VALUES[value] written into element `at` = (row, frame, channel) of the mels; the references
    and yardsticks are those of the poisoned input."""
    c = case(name)
    x = c["x"].copy()
    x[at] = POISON_VALUES[value]
    return finish(dict(shape=c["shape"], params=c["params"], x=x, row=at[0]))


@functools.lru_cache(maxsize=None)
def zeroed_top_recurrence(name):
    """The float64 output of case(name) with the top layer's weight_hh set to zero."""
    c = case(name)
    L = c["shape"][4]
    ps = list(c["params"])
    ps[4 * (L - 1) + 1] = np.zeros_like(ps[4 * (L - 1) + 1])
    return enc.encode_ref(ps, c["x"].astype(np.float64))


# ---- parameters whose packed image can be counted -------------------------------------------------------------------------------
def integer_params(n_mels, H, L, D):
    """Parameters in pack order, float32 and exact: every weight a distinct positive integer below 2^24, bias_ih distinct
    positive integers, bias_hh 0.5 everywhere (every bias sum a distinct k + 0.5, no weight's value), the projection bias
    distinct negative integers.  -> (params, expected): `expected` the sorted values a packed buffer holds beside its
    zero padding."""
    ps, nw, nb = [], 0, 0
    for l in range(L):
        I = n_mels if l == 0 else H
        for shape in ((4 * H, I), (4 * H, H)):
            n = shape[0] * shape[1]
            ps.append(np.arange(nw + 1, nw + n + 1, dtype=np.float32).reshape(shape))
            nw += n
        ps.append(np.arange(nb + 1, nb + 4 * H + 1, dtype=np.float32))
        ps.append(np.full(4 * H, 0.5, dtype=np.float32))
        nb += 4 * H
    ps.append(np.arange(nw + 1, nw + D * H + 1, dtype=np.float32).reshape(D, H))
    nw += D * H
    ps.append(-np.arange(1, D + 1, dtype=np.float32))
    assert nw < 2 ** 24
    expected = np.sort(np.concatenate([np.arange(1, nw + 1), np.arange(1, nb + 1) + 0.5, -np.arange(1.0, D + 1)]).astype(np.float32))
    return ps, expected


def packed_floats(n_mels, H, L, D):
    """The packed buffer's length as include/ge2e_hip.h describes it: per layer [pad16(I) + H][4 H] and 4 H bias sums, then
    [H][pad16(D)] and pad16(D) biases."""
    pad16 = lambda n: (n + 15) // 16 * 16                                      # noqa: E731
    layer = lambda I: (pad16(I) + H) * 4 * H + 4 * H                           # noqa: E731
    return layer(n_mels) + (L - 1) * layer(H) + H * pad16(D) + pad16(D)
