"""The mel front end restated in numpy (a plain helper module, no fixtures): the reference's ``pySTFT`` and lines 41-50 of
``get_mel_spects_from_audio`` -- np.pad reflect, strided frames, scipy's periodic Hann window, rfft, |.|, the mel basis,
20 log10 and the clip -- in float64 as the reference of the GPU tests and in float32 throughout as their yardstick
(scipy.fft.rfft keeps float32; np.fft.rfft would not), the Slaney filterbank ``librosa.filters.mel`` returns by default,
and the error measure and gate of those tests."""
import numpy as np
import scipy.fft
import scipy.signal


def hz_to_mel(f):
    """Slaney's scale: linear below 1 kHz (200/3 Hz a mel), logarithmic above with step log(6.4) / 27."""
    f = np.asarray(f, dtype=np.float64)
    min_log_mel, logstep = 1000.0 / (200.0 / 3), np.log(6.4) / 27.0
    return np.where(f >= 1000.0, min_log_mel + np.log(np.maximum(f, 1e-9) / 1000.0) / logstep, f / (200.0 / 3))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    min_log_mel, logstep = 1000.0 / (200.0 / 3), np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, 1000.0 * np.exp(logstep * (m - min_log_mel)), m * (200.0 / 3))


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """(n_mels, n_fft/2 + 1) float64, librosa.filters.mel's layout: triangles between n_mels + 2 points equally spaced
    on the mel scale, each weighted by 2 / (f[i+2] - f[i])."""
    fmax = sr / 2.0 if fmax is None else fmax
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, len(fft_f)))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def hann(n_fft, dtype=np.float64):
    return scipy.signal.get_window("hann", n_fft, fftbins=True).astype(dtype)


def magnitudes(x, n_fft, hop, dtype=np.float64, window=None):
    """|rfft(window . frame)| of every frame of x, (len(x) // hop + 1, n_fft/2 + 1), computed in `dtype` throughout."""
    x = np.pad(np.asarray(x).astype(dtype), n_fft // 2, mode="reflect")
    F = (len(x) - (n_fft - hop)) // hop
    frames = np.lib.stride_tricks.as_strided(x, (F, n_fft), (hop * x.strides[0], x.strides[0]))
    window = hann(n_fft, dtype) if window is None else np.asarray(window).astype(dtype)
    S = np.abs(scipy.fft.rfft(window * frames, n=n_fft, axis=1))
    assert S.dtype == dtype, S.dtype
    return S


def epilogue(mel, min_level_db=-100.0, ref_level_db=16.0):
    """Lines 47-50 in the dtype of `mel`: clip((20 log10(max(min_level, mel)) - ref - min_db) / -min_db, 0, 1)."""
    dt = mel.dtype.type
    min_level = dt(np.exp(min_level_db / 20.0 * np.log(10.0)))
    db = dt(20.0) * np.log10(np.maximum(min_level, mel)) - dt(ref_level_db)
    return np.clip((db - dt(min_level_db)) / dt(-min_level_db), dt(0.0), dt(1.0))


def melspec_ref(x, basis, n_fft, hop, dtype=np.float64, padded_len=None, gain=1.0, window=None, min_level_db=-100.0,
                ref_level_db=16.0):
    """(linear mel, normalised dB mel) of one waveform: `x` times `gain`, extended with zeros to `padded_len`; `basis`
    (n_fft/2 + 1, n_mels); `window` the periodic Hann window unless given."""
    x = np.asarray(x).astype(dtype) * dtype(gain)
    if padded_len is not None and padded_len > len(x):
        x = np.pad(x, (0, padded_len - len(x)))
    mel = magnitudes(x, n_fft, hop, dtype, window) @ np.asarray(basis).astype(dtype)
    return mel, epilogue(mel, min_level_db, ref_level_db)


def rel_err(got, ref):
    """The largest per-frame relative Frobenius error."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref, axis=-1)
    return float((np.linalg.norm(got - ref, axis=-1) / np.where(den > 0, den, 1.0)).max())


def gate(err_ref, floor=2.0 ** -22):
    """What the native output may be off by: four times the float32 yardstick's own error on the same inputs, plus a floor."""
    return 4.0 * err_ref + floor
