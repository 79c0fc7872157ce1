"""Capture the reference's own audio front end on seeded synthetic waveforms (build container only).

    python tests/golden/make_melspec_golden.py <path of the reference checkout>

Imports ``utils/audio_utils.py`` of the reference with ``librosa`` and ``webrtcvad`` replaced by stub modules in
``sys.modules`` -- ``librosa.filters.mel`` is the Slaney filterbank of ``tests/melspec_ref.py``, ``librosa.load`` hands
back the given array -- and records, per case, what ``AudioUtils`` itself computes (float64, data only):

    wav        the waveform (float32: noise plus a tone and a chirp)
    full       get_mel_spects_from_audio(partial_slices=False, clean_data=False)   (frames, n_mels)
    partial    get_mel_spects_from_audio(partial_slices=True, clean_data=False)    (partials, partials_n_frames, n_mels)
    mel_slices, wav_slices   compute_partial_slices(len(wav)) as (n, 2) start / stop
    normed     normalize_volume(wav, increase_only=True)
    basis      AudioUtils.mel_basis                                                (n_fft/2 + 1, n_mels)
    cfg        sampling_rate, n_fft, hop_length, mel_window_step, mel_n_channels, partials_n_frames, rate_partial_slices,
               min_coverage, audio_norm_target_dBFS

Cases: c0 the reference's settings (strings/constants.py) at 1.3 s, one partial of 180 frames; c1 n_fft 256, hop 64, 40
channels, partials of 20 frames, one partial (the waveform is zero-padded to it); c2 n_fft 512, hop 160, three partials kept
and a fourth dropped by min_coverage.  Written: ``tests/golden/callers/melspec.npz``.
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

CASES = {
    # name: (n_fft, hop, n_mels, partials_n_frames, rate, samples, amplitude, seed)
    "c0": (1024, 128, 80, 180, 1.3, 20800, 0.05, 1),
    "c1": (256, 64, 40, 20, 10.0, 2500, 0.004, 2),
    "c2": (512, 160, 40, 20, 10.0, 6500, 0.3, 3),
}


def waveform(n, amp, seed, sr=16000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.3 * rng.standard_normal(n) + np.sin(2 * np.pi * 440.0 * t) + 0.7 * np.sin(2 * np.pi * (500.0 + 9000.0 * t) * t)
    return (amp * x).astype(np.float32)


def capture(reference):
    warnings.simplefilter("ignore")
    current = {}
    librosa, filters = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
    filters.mel = lambda sr, n_fft, fmin=0.0, fmax=None, n_mels=128: ref.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    librosa.filters = filters
    librosa.load = lambda path, sr=None: (current[path], 16000)
    sys.modules["librosa"], sys.modules["librosa.filters"] = librosa, filters
    sys.modules["webrtcvad"] = types.ModuleType("webrtcvad")
    sys.path.insert(0, reference)
    from utils.audio_utils import AudioUtils

    out = {}
    for name, (n_fft, hop, n_mels, pframes, rate, n, amp, seed) in CASES.items():
        hp = NS(audio=NS(sampling_rate=16000, n_fft=n_fft, hop_length=hop, mel_window_step=10, mel_n_channels=n_mels,
                         partials_n_frames=pframes),
                vad=NS(rate_partial_slices=rate, min_coverage=0.75, audio_norm_target_dBFS=-30))
        au = AudioUtils(hp)
        wav = waveform(n, amp, seed)
        current["w"] = wav
        wav_slices, mel_slices = au.compute_partial_slices(len(wav))
        out[name + "_wav"] = wav
        out[name + "_full"] = au.get_mel_spects_from_audio("w", partial_slices=False, clean_data=False)
        out[name + "_partial"] = au.get_mel_spects_from_audio("w", partial_slices=True, clean_data=False)
        out[name + "_mel_slices"] = np.array([(s.start, s.stop) for s in mel_slices], dtype=np.int64)
        out[name + "_wav_slices"] = np.array([(s.start, s.stop) for s in wav_slices], dtype=np.int64)
        out[name + "_normed"] = np.asarray(au.normalize_volume(wav, increase_only=True))
        out[name + "_basis"] = np.asarray(au.mel_basis, dtype=np.float64)
        out[name + "_cfg"] = np.array([16000, n_fft, hop, 10, n_mels, pframes, rate, 0.75, -30], dtype=np.float64)
        print(name, "full", out[name + "_full"].shape, "partial", out[name + "_partial"].shape, "slices",
              out[name + "_mel_slices"].tolist(), "wav stop", int(out[name + "_wav_slices"][-1, 1]), "gain",
              float(out[name + "_normed"][5] / wav[5]))
    path = os.path.join(HERE, "callers", "melspec.npz")
    np.savez_compressed(path, **out)
    print(f"melspec.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    capture(sys.argv[1])
