"""The oracle of the silence-trimming stage (ge2e_vad_flags / ge2e_vad_mask / ge2e_vad_trim): numpy float32 for the
quantiser, as the reference's ``np.round(wav * int16_max)`` computes it, numpy int64 for the sums and Python integers for
the comparison whose products pass 64 bits.  A plain helper module; everything here is exact.

    quantise   q = sat16(rint(fl32(fl32(x * gain) * 32767)))      NaN -> 0
    energies   e = S sum(q^2) - (sum q)^2 per window of S samples
    flags      e >= min_energy and e * 256 > min(e over |v - w| <= span, same utterance) * ratio_q8
    mask       m = 2 sum(flag[w - (A-1)//2 .. w + A//2]) > A;  keep = any m[i - (n-1)//2 .. i + n//2], n = max_silence + 1
    dst        the rank of a kept window among its utterance's kept windows, -1 for a dropped one
    trim       the kept windows' samples, untouched
"""
import numpy as np


def ratio_q8(ratio_db):
    return int(round(10.0 ** (ratio_db / 10.0) * 256))


def min_energy(S, min_level_dbfs):
    return int(round(S * S * (32767.0 * 10.0 ** (min_level_dbfs / 20.0)) ** 2))


def quantise(x, gain=1.0):
    """int64 array: the int16 value of every sample, saturating."""
    with np.errstate(all="ignore"):
        t = (np.asarray(x, dtype=np.float32) * np.float32(gain)).astype(np.float32) * np.float32(32767.0)
        r = np.rint(t.astype(np.float32))
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, -32768.0, 32767.0).astype(np.int64)


def exact_halves(ks, gain=1.0):
    """float32 samples whose scaled value fl32(fl32(x * gain) * 32767) is exactly k + 1/2 for a k of ``ks``: the float32
    neighbours of (k + 1/2) / (32767 gain), filtered with the quantiser's own arithmetic -> [(x, k)]."""
    found = []
    g = np.float32(gain)
    for k in ks:
        x = np.float32((k + 0.5) / (32767.0 * float(g)))
        cands = [x]
        for _ in range(8):
            cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
        for c in cands:
            if float(np.float32(np.float32(c * g) * np.float32(32767.0))) == k + 0.5:
                found.append((np.float32(c), k))
    return found


def energies(x, S, gain=1.0):
    """e[w] for the len(x) // S whole windows of one utterance (the rest is not looked at), int64."""
    W = len(x) // S
    q = quantise(np.asarray(x)[:W * S], gain).reshape(W, S)
    return S * (q * q).sum(axis=1) - q.sum(axis=1) ** 2


def flags_from_energies(e, span, ratio, floor_energy):
    e = [int(v) for v in e]
    out = np.zeros(len(e), dtype=np.uint8)
    for w, ew in enumerate(e):
        fl = min(e[max(0, w - span):w + span + 1])
        out[w] = ew >= floor_energy and ew * 256 > fl * ratio
    return out


def flags(x, S, gain=1.0, span=100, ratio=None, floor_energy=None):
    ratio = ratio_q8(9.0) if ratio is None else ratio
    floor_energy = min_energy(S, -60.0) if floor_energy is None else floor_energy
    return flags_from_energies(energies(x, S, gain), span, ratio, floor_energy)


def mask(flag, A, max_silence):
    """keep[w] (bool) of one utterance's flags."""
    f = (np.asarray(flag) != 0).astype(np.int64)
    W, n = len(f), max_silence + 1
    if W == 0:
        return np.zeros(0, dtype=bool)
    windows = np.lib.stride_tricks.sliding_window_view
    fp = np.concatenate([np.zeros((A - 1) // 2, np.int64), f, np.zeros(A // 2, np.int64)])
    m = (2 * windows(fp, A).sum(axis=1) > A).astype(np.int64)          # row w: fp[w .. w + A) = f[w - (A-1)//2 .. w + A//2]
    mp = np.concatenate([np.zeros((n - 1) // 2, np.int64), m, np.zeros(n // 2, np.int64)])
    return windows(mp, n).any(axis=1)


def ranks(keep):
    """dst (int32) of one utterance and its kept count."""
    keep = np.asarray(keep, dtype=bool)
    dst = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return dst, int(keep.sum())


def trim(x, S, keep):
    x = np.asarray(x)
    W = len(x) // S
    return x[:W * S].reshape(W, S)[np.asarray(keep, dtype=bool)].reshape(-1)


def trim_silences(x, S, gain=1.0, A=8, max_silence=6, voice_flags=None, **detector):
    """One utterance through the whole stage -> (trimmed samples, flags, keep)."""
    f = flags(x, S, gain, **detector) if voice_flags is None else np.asarray(voice_flags)
    keep = mask(f, A, max_silence)
    return trim(x, S, keep), f, keep


def bursts(seed, snr_db, sr=16000, seconds=8.0):
    """The detector's test signal: three bursts of a 19-harmonic tone (f0 120 Hz, 5 Hz vibrato of 3 %, a 4 Hz envelope
    between 0.5 and 1) over white noise ``snr_db`` below the bursts' power -> (float32 samples, [(start, stop)] in samples)."""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    phase = 2 * np.pi * 120.0 * t + 0.03 * 120.0 / 5.0 * np.sin(2 * np.pi * 5.0 * t)
    tone = sum(np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 20))
    tone *= 0.75 + 0.25 * np.sin(2 * np.pi * 4.0 * t)
    spans = [(int(0.9 * sr), int(2.3 * sr)), (int(3.6 * sr), int(4.7 * sr)), (int(6.0 * sr), int(7.2 * sr))]
    gate = np.zeros(n)
    for a, b in spans:
        gate[a:b] = 1.0
    speech = 0.1 * tone / np.sqrt(np.mean(tone ** 2)) * gate
    noise = rng.standard_normal(n) * 0.1 * 10.0 ** (-snr_db / 20.0)
    return (speech + noise).astype(np.float32), spans
