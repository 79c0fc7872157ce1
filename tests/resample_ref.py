"""The float64 oracle of the resampling stage (a plain helper module): the definition of include/ge2e_hip.h restated with
numpy, nothing shared with the code under test.

    y[n] = sum_{k=0}^{W-1} taps[p][k] x[i0 + lead - k],   t = n M, i0 = t div L, p = t mod L,   n < ceil(len L / M)

with x zero outside its own extent, and the per-utterance gain of normalize_volume.
"""
import math

import numpy as np

PRESETS = {"kaiser_best": (64, 0.9475937167399596, 14.769656459379492), "kaiser_fast": (16, 0.85, 8.555504641634386)}


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g                      # L (up), M (down)


def out_length(n, L, M):
    return -((-n * L) // M)                             # ceil


def bank(L, M, Z, rolloff, beta):
    """The project's Kaiser-windowed sinc bank from its formula, float64 -> (lead, taps[L][2 lead + 1]).  I0 by its power
    series (every term positive: no cancellation), so that audio.resample_bank is held to another implementation."""
    s = min(1.0, L / M)
    assert float(Z).is_integer()
    lead = -((-int(Z) * M) // L) if L < M else int(Z)   # ceil(Z / s), exactly

    def i0(v):
        v = np.asarray(v, dtype=np.float64)
        term, total = np.ones_like(v), np.ones_like(v)
        for j in range(1, 200):
            term = term * (v / (2.0 * j)) ** 2
            total = total + term
        return total

    k = np.arange(2 * lead + 1)[None, :]
    p = np.arange(L)[:, None]
    u = (k - lead + p / L) * s
    inside = np.abs(u) < Z
    arg = np.pi * rolloff * u
    sinc = np.where(arg == 0, 1.0, np.sin(arg) / np.where(arg == 0, 1.0, arg))
    win = i0(beta * np.sqrt(np.where(inside, 1.0 - (u / Z) ** 2, 0.0))) / i0(beta)
    return lead, np.where(inside, s * rolloff * sinc * win, 0.0)


def indices(n_in, L, M, lead, W):
    """(n_out, W) sample index of tap k of output n, and the phase of every output; Python integers are exact."""
    n_out = out_length(n_in, L, M)
    t = np.arange(n_out, dtype=np.int64) * M
    return (t // L)[:, None] + lead - np.arange(W, dtype=np.int64)[None, :], t % L


def resample_ref(x, taps, L, M, lead):
    """-> (y, mag): y float64 of the definition on x and taps as given (cast to float64), mag[n] = sum_k |taps x|."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    W = 2 * lead + 1
    assert taps.shape == (L, W)
    idx, phase = indices(len(x), L, M, lead, W)
    inside = (idx >= 0) & (idx < len(x))
    xs = np.where(inside, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    prod = taps[phase] * xs
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def windows_holding(n_in, L, M, lead, j):
    """Which outputs' windows [i0 + lead - W + 1, i0 + lead] contain sample j."""
    idx, _ = indices(n_in, L, M, lead, 2 * lead + 1)
    return (idx == j).any(axis=1)


def gain_ref(x, target_dbfs=-30.0, increase_only=True):
    """The factor of normalize_volume in float64 (inf for silence, NaN for no samples)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rms = np.sqrt(np.float64(math.fsum(x * x)) / np.float64(len(x)))
        change = target_dbfs - 20.0 * np.log10(rms)
        gain = np.float64(10.0) ** (change / 20.0)
    return np.float64(1.0) if increase_only and change < 0 else gain


def float32_neighbours(v):
    """The float32 rounding of a float64 and the float32 values either side of it."""
    r = np.float32(v)
    return {r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))}
