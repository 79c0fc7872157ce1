"""Capture the reference's own ``trim_long_silences`` on seeded waveforms and recorded voice flags (build container only).

    python tests/golden/make_vad_golden.py <path of the reference checkout>

Imports ``utils/audio_utils.py`` of the reference with ``librosa`` replaced by a stub module (as make_melspec_golden.py
does) and ``webrtcvad`` by a class that replays recorded flags, one per ``is_speech`` call, and checks that every call gets
one window of 16-bit samples; ``np.bool``, which the reference still uses, is set to ``bool``.  Per case it records (data
only):

    wav        the waveform (float32; a length that is no multiple of the window, except v3's)
    flags      the voice flags the stub replayed, one per whole window (uint8)
    cfg        sampling_rate, vad_window_length, vad_moving_average_width, vad_max_silence_length (int64)
    trimmed    what AudioUtils.trim_long_silences(wav) returned (float32)

Sampling rate 1000 and windows of 30 ms, so 30 samples a window.  Cases: v0 the reference's widths (8, 6) on runs of
voiced and unvoiced windows; v1 an odd width and no dilation (3, 0); v2 an even width under a long dilation (4, 9), sparse
flags; v3 (1, 1) on dense random flags; v4 all flags zero (nothing kept).  Written: ``tests/golden/callers/vad.npz`` (beside melspec.npz: tests/golden/*.npz itself is the loss fixtures' directory, every file of which the suite loads as one).
"""
import os
import sys
import types
import warnings
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import melspec_ref as ref  # noqa: E402

SR, WINDOW_MS = 1000, 30
CASES = {
    # name: (samples, moving average width, max silence, flag density, run length, seed)
    "v0": (4217, 8, 6, 0.5, 7, 1),
    "v1": (3010, 3, 0, 0.5, 2, 2),
    "v2": (5999, 4, 9, 0.25, 3, 3),
    "v3": (2400, 1, 1, 0.7, 1, 4),
    "v4": (1234, 8, 6, 0.0, 1, 5),
}


def recorded_flags(n_windows, density, run, seed):
    rng = np.random.default_rng(seed)
    runs = rng.random(n_windows // run + 1) < density
    return np.repeat(runs, run)[:n_windows].astype(np.uint8)


def capture(reference):
    warnings.simplefilter("ignore")
    replay = {}

    class Vad:
        def __init__(self, mode=None):
            self.at = 0

        def is_speech(self, buf, sample_rate):
            assert sample_rate == SR and len(buf) == 2 * (WINDOW_MS * SR // 1000)
            self.at += 1
            return bool(replay["flags"][self.at - 1])

    librosa, filters = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
    filters.mel = lambda sr, n_fft, fmin=0.0, fmax=None, n_mels=128: ref.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    librosa.filters = filters
    sys.modules["librosa"], sys.modules["librosa.filters"] = librosa, filters
    webrtcvad = types.ModuleType("webrtcvad")
    webrtcvad.Vad = Vad
    sys.modules["webrtcvad"] = webrtcvad
    if not hasattr(np, "bool"):
        np.bool = bool
    sys.path.insert(0, reference)
    from utils.audio_utils import AudioUtils

    out = {}
    for name, (n, width, silence, density, run, seed) in CASES.items():
        hp = NS(audio=NS(sampling_rate=SR, n_fft=64, hop_length=16, mel_n_channels=8),
                vad=NS(vad_window_length=WINDOW_MS, vad_moving_average_width=width, vad_max_silence_length=silence))
        au = AudioUtils(hp)
        rng = np.random.default_rng(100 + seed)
        wav = (0.3 * rng.standard_normal(n)).astype(np.float32)
        flags = recorded_flags(n // (WINDOW_MS * SR // 1000), density, run, seed)
        replay["flags"] = flags
        trimmed = np.asarray(au.trim_long_silences(wav))
        assert trimmed.dtype == np.float32
        out[name + "_wav"], out[name + "_flags"], out[name + "_trimmed"] = wav, flags, trimmed
        out[name + "_cfg"] = np.array([SR, WINDOW_MS, width, silence], dtype=np.int64)
        print(name, "windows", len(flags), "voiced", int(flags.sum()), "kept samples", len(trimmed), "of", n)
    path = os.path.join(HERE, "callers", "vad.npz")
    np.savez_compressed(path, **out)
    print(f"vad.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    capture(sys.argv[1])
