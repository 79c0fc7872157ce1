"""The audio front end of the reference (``utils/audio_utils.py``, s0) around ``functional.melspec``: the tables the
reference takes from scipy and librosa -- a periodic Hann window, the Slaney mel filterbank -- built here in float64, its
partial-utterance arithmetic (``compute_partial_slices``), the per-utterance gain of ``normalize_volume``, and
``MelFrontEnd``, which holds the packed tables per device and turns waveforms into the frames ``functional.encode`` reads.

A recording at another rate is resampled on the device first (``resample_bank``, ``functional.resample``: the reference's
``librosa.resample`` step, with the project's own exact-phase Kaiser-windowed sinc), and its gain then comes from
``functional.volume_gain``.

The reference's ``trim_long_silences`` runs on the device too (``trim_silences=True``; ``functional.trim_silences``): its
window arithmetic, int16 quantisation, moving average, rounding, dilation and selection of samples are reproduced exactly.
The per-window voice decision, which the reference takes from webrtcvad, is the project's own integer detector and NOT
webrtcvad's (webrtcvad is no part of this project): a caller who wants the reference's trimming to the sample passes
webrtcvad's flags -- or any detector's -- as ``voice_flags=``.

Out of scope: decoding audio files.  The caller hands in samples and their rate.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

def hann_window(n_fft: int) -> torch.Tensor:
    """The periodic Hann window scipy's ``get_window('hann', n_fft, fftbins=True)`` returns, (n_fft,) float64."""
    k = torch.arange(n_fft, dtype=torch.float64)
    return 0.5 - 0.5 * torch.cos(2.0 * math.pi * k / n_fft)


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    min_log_mel, logstep = 1000.0 / (200.0 / 3), np.log(6.4) / 27.0
    return np.where(f >= 1000.0, min_log_mel + np.log(np.maximum(f, 1e-9) / 1000.0) / logstep, f / (200.0 / 3))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    min_log_mel, logstep = 1000.0 / (200.0 / 3), np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, 1000.0 * np.exp(logstep * (m - min_log_mel)), m * (200.0 / 3))


def mel_filterbank(sr: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> torch.Tensor:
    """What ``librosa.filters.mel(sr, n_fft, n_mels=, fmin=, fmax=)`` returns by default, transposed to the layout
    ``melspec_pack`` takes: (n_fft/2 + 1, n_mels) float64.  Slaney's mel scale -- linear below 1 kHz at 200/3 Hz a mel,
    logarithmic above with step log(6.4) / 27 --, triangles between n_mels + 2 equally spaced mel points, each
    area-normalised by 2 / (f[i+2] - f[i]).  The reference calls it with fmin 90 and fmax 7600 (s0:22-26)."""
    fmax = sr / 2.0 if fmax is None else fmax
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return torch.from_numpy(np.ascontiguousarray(w.T))


class PartialSlices(NamedTuple):
    mel_starts: list      # the first mel frame of every partial utterance
    padded_length: int    # the sample count the waveform is zero-extended to: max(n_samples, the last slice's end)


def partial_slices(n_samples: int, *, sampling_rate: int = 16000, mel_window_step: float = 10, partials_n_frames: int = 180,
                   rate: float = 1.3, min_coverage: float = 0.75) -> PartialSlices:
    """``compute_partial_slices`` (s0:150-199): where the partial utterances of ``partials_n_frames`` mel frames start,
    ``rate`` of them a second, the last one dropped where it would cover less than ``min_coverage`` (never the only one).
    As in the reference, ``samples_per_frame`` comes from ``mel_window_step`` (milliseconds) although the spectrogram's
    hop is ``hop_length``: the mel starts index the spectrogram as they are."""
    if not 0 < min_coverage <= 1:
        raise ValueError("min_coverage must be in (0, 1]")
    samples_per_frame = int(sampling_rate * mel_window_step / 1000)
    n_frames = int(math.ceil((n_samples + 1) / samples_per_frame))
    frame_step = int(np.round((sampling_rate / rate) / samples_per_frame))
    if not 0 < frame_step <= partials_n_frames:
        raise ValueError(f"rate {rate} gives a step of {frame_step} frames; it must be in 1 .. {partials_n_frames}")
    starts = list(range(0, max(1, n_frames - partials_n_frames + frame_step + 1), frame_step))
    last = starts[-1] * samples_per_frame
    coverage = (n_samples - last) / (partials_n_frames * samples_per_frame)
    if coverage < min_coverage and len(starts) > 1:
        starts = starts[:-1]
    stop = (starts[-1] + partials_n_frames) * samples_per_frame
    return PartialSlices(starts, max(n_samples, stop))


def volume_gain(wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, target_dbfs: float = -30.0,
                increase_only: bool = True) -> torch.Tensor:
    """The factor ``normalize_volume`` (s0:94-105) multiplies every utterance by, (U,) float32 on wav's device, made with
    torch ops (no read-back): 10^((target - dBFS) / 20) with dBFS = 20 log10(rms), and, with ``increase_only``, 1 where that
    would lower the volume.  ``melspec(gain=...)`` applies it inside the kernel."""
    ls = [wav.numel()] if lengths is None else [int(v) for v in lengths]
    sq = (wav.detach().double() ** 2)
    csum = torch.cat([sq.new_zeros(1), torch.cumsum(sq, 0)])
    ends = torch.tensor(np.cumsum(ls), dtype=torch.int64).to(wav.device)
    n = torch.tensor(ls, dtype=torch.float64).to(wav.device)
    begins = ends - n.long()
    rms = torch.sqrt((csum[ends] - csum[begins]) / n)
    change = target_dbfs - 20.0 * torch.log10(rms)
    gain = 10.0 ** (change / 20.0)
    if increase_only:
        gain = torch.where(change < 0, torch.ones_like(gain), gain)
    return gain.float()


class ResampleBank(NamedTuple):
    up: int               # L = sr_out / gcd
    down: int             # M = sr_in / gcd
    lead: int             # taps either side of the centre: the width of a phase is 2 lead + 1
    taps: torch.Tensor    # (up, 2 lead + 1) float64


# (zero crossings, roll-off, Kaiser beta): the constants resampy publishes for its filters of the same names
RESAMPLE_PRESETS = {"kaiser_best": (64, 0.9475937167399596, 14.769656459379492),
                    "kaiser_fast": (16, 0.85, 8.555504641634386)}


def resample_bank(sr_in: int, sr_out: int, filter="kaiser_best") -> ResampleBank:
    """The polyphase bank of a Kaiser-windowed sinc for ``sr_in -> sr_out``, in float64 (``functional.resample_pack`` rounds
    it once to float32).  With g = gcd, L = sr_out / g, M = sr_in / g, s = min(1, L / M), Z zero crossings,
    lead = ceil(Z / s) and u = (k - lead + p / L) s:
        taps[p][k] = s rolloff sinc(rolloff u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta)   for |u| < Z, else 0
    so that output n, with i0 = n M div L and p = n M mod L, is sum_k taps[p][k] x[i0 + lead - k].  ``filter``:
    "kaiser_best", "kaiser_fast" or ``(zeros, rolloff, beta)``.  Every phase is exact: no table interpolation."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError("the rates must be positive")
    if isinstance(filter, str):
        if filter not in RESAMPLE_PRESETS:
            raise ValueError(f"filter must be one of {sorted(RESAMPLE_PRESETS)} or (zeros, rolloff, beta), got {filter!r}")
        filter = RESAMPLE_PRESETS[filter]
    Z, rolloff, beta = filter
    if not (Z > 0 and 0 < rolloff <= 1 and beta >= 0):
        raise ValueError("(zeros, rolloff, beta) needs zeros > 0, 0 < rolloff <= 1 and beta >= 0")
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    if L >= M:
        s, lead = 1.0, int(math.ceil(Z))
    else:
        s = L / M
        lead = -((-Z * M) // L) if isinstance(Z, int) else int(math.ceil(Z * M / L))
    k = np.arange(2 * lead + 1, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    u = (k - lead + p / L) * s
    inside = np.abs(u) < Z
    window = np.i0(beta * np.sqrt(np.where(inside, 1.0 - (u / Z) ** 2, 0.0))) / np.i0(beta)
    taps = np.where(inside, s * rolloff * np.sinc(rolloff * u) * window, 0.0)
    return ResampleBank(L, M, lead, torch.from_numpy(np.ascontiguousarray(taps)))


def resampled_length(n: int, up: int, down: int) -> int:
    """The samples ``n`` samples become: ceil(n up / down), as librosa sizes its output."""
    return (int(n) * int(up) + int(down) - 1) // int(down)


class MelFrontEnd:
    """Waveforms to mel frames at one set of audio settings.  The window and filterbank are built once in float64 and
    packed once per device (``functional.melspec_pack``); ``frames`` is one ``functional.melspec`` call over all the
    waveforms, ``partials`` the partial utterances of every waveform as ``get_mel_spects_from_audio`` returns them.

    ``source_rate``: the rate of the waveforms handed in where it is not ``sampling_rate``.  They are then resampled on the
    device in one launch (``functional.resample`` with ``resample_bank(source_rate, sampling_rate, resample_filter)``,
    packed once per (rate, filter, device)), the partial-slice arithmetic runs on the resampled lengths and the gain of
    ``normalize_volume`` comes from ``functional.volume_gain`` on the resampled signal.  One rate for all the waveforms of
    a call: a different rate per waveform is not built (call once per rate).

    ``trim_silences`` / ``voice_flags``: the reference's ``trim_long_silences`` between the gain and the spectrogram
    (``functional.trim_silences`` with this front end's ``vad_*`` settings).  The order is the reference's: resample, gain
    of the untrimmed signal, trim, spectrogram of the trimmed lengths.  The built-in voice flags are the project's own
    detector (``vad_floor_span``, ``vad_ratio_db``, ``vad_min_level_dbfs``), not webrtcvad's; ``voice_flags`` hands in
    others, one per window of ``vad_window_length`` ms, utterance after utterance (passing it implies the trimming).  It
    costs one read-back of the kept lengths per call."""

    def __init__(self, sampling_rate: int = 16000, n_fft: int = 1024, hop_length: int = 128, n_mels: int = 80,
                 fmin: float = 90.0, fmax: float = 7600.0, mel_window_step: float = 10, partials_n_frames: int = 180,
                 rate_partial_slices: float = 1.3, min_coverage: float = 0.75, target_dbfs: float = -30.0,
                 min_level_db: float = -100.0, ref_level_db: float = 16.0, vad_window_length: int = 30,
                 vad_moving_average_width: int = 8, vad_max_silence_length: int = 6, vad_floor_span: int = 100,
                 vad_ratio_db: float = 9.0, vad_min_level_dbfs: float = -60.0):
        self.vad_window_length, self.vad_moving_average_width = vad_window_length, vad_moving_average_width
        self.vad_max_silence_length, self.vad_floor_span = vad_max_silence_length, vad_floor_span
        self.vad_ratio_db, self.vad_min_level_dbfs = vad_ratio_db, vad_min_level_dbfs
        self.sampling_rate, self.n_fft, self.hop_length, self.n_mels = sampling_rate, n_fft, hop_length, n_mels
        self.mel_window_step, self.partials_n_frames = mel_window_step, partials_n_frames
        self.rate_partial_slices, self.min_coverage, self.target_dbfs = rate_partial_slices, min_coverage, target_dbfs
        self.min_level_db, self.ref_level_db = min_level_db, ref_level_db
        self.window = hann_window(n_fft)
        self.basis = mel_filterbank(sampling_rate, n_fft, n_mels, fmin, fmax)
        self._tables = {}
        self._resamplers = {}

    @classmethod
    def from_hp(cls, hp) -> "MelFrontEnd":
        """From the reference's hyper-parameters (``hp.audio``, ``hp.vad``; s0:22-26 fixes fmin 90 and fmax 7600)."""
        a, v = hp.audio, hp.vad
        return cls(a.sampling_rate, a.n_fft, a.hop_length, a.mel_n_channels, 90.0, 7600.0, a.mel_window_step,
                   a.partials_n_frames, v.rate_partial_slices, v.min_coverage, getattr(v, "audio_norm_target_dBFS", -30.0),
                   vad_window_length=getattr(v, "vad_window_length", 30),
                   vad_moving_average_width=getattr(v, "vad_moving_average_width", 8),
                   vad_max_silence_length=getattr(v, "vad_max_silence_length", 6),
                   vad_floor_span=getattr(v, "vad_floor_span", 100), vad_ratio_db=getattr(v, "vad_ratio_db", 9.0),
                   vad_min_level_dbfs=getattr(v, "vad_min_level_dbfs", -60.0))

    def tables(self, device):
        """The packed tables on ``device``, made on first use."""
        from . import functional as GF
        device = GF._resolve_device(device)
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = GF.melspec_pack(self.window.to(device), self.basis.to(device))
        return t

    def slices(self, n_samples: int) -> PartialSlices:
        return partial_slices(n_samples, sampling_rate=self.sampling_rate, mel_window_step=self.mel_window_step,
                              partials_n_frames=self.partials_n_frames, rate=self.rate_partial_slices,
                              min_coverage=self.min_coverage)

    def _resampling(self, source_rate) -> bool:
        return source_rate is not None and int(source_rate) != int(self.sampling_rate)

    def resampler(self, source_rate: int, device, resample_filter="kaiser_best"):
        """``functional.resample_pack`` of ``resample_bank(source_rate, sampling_rate, resample_filter)`` on ``device``,
        made on first use and kept per (rate, filter, device)."""
        from . import functional as GF
        device = GF._resolve_device(device)
        key = (int(source_rate), resample_filter if isinstance(resample_filter, str) else tuple(resample_filter), device)
        t = self._resamplers.get(key)
        if t is None:
            bank = resample_bank(source_rate, self.sampling_rate, resample_filter)
            t = self._resamplers[key] = GF.resample_pack(bank.taps.to(device), bank.up, bank.down, bank.lead)
        return t

    def resampled_lengths(self, lengths, source_rate=None) -> list:
        """The lengths ``frames`` works with: ``lengths`` themselves, or what ``source_rate`` makes of them."""
        if not self._resampling(source_rate):
            return [int(n) for n in lengths]
        g = math.gcd(int(source_rate), int(self.sampling_rate))
        return [resampled_length(n, self.sampling_rate // g, int(source_rate) // g) for n in lengths]

    @property
    def vad_window(self) -> int:
        """Samples of a voice-detection window: ``vad_window_length * sampling_rate // 1000`` (s0:115)."""
        return (int(self.vad_window_length) * int(self.sampling_rate)) // 1000

    def preprocess(self, wavs, normalize_volume: bool = False, native: Optional[bool] = None,
                   source_rate: Optional[int] = None, resample_filter="kaiser_best", trim_silences: bool = False,
                   voice_flags=None):
        """A batch's ``get_audio_as_np_array``: ``(flat, lengths, gain)`` -- the waveforms back to back at the model's rate,
        their sample counts (a Python list) and the per-utterance gain on the device (None without ``normalize_volume``),
        which stays a separate factor that ``spectrogram`` hands to the kernel.  In the reference's order: resample
        (``source_rate``), gain of the untrimmed signal, ``trim_long_silences`` (``trim_silences`` or ``voice_flags``; the
        lengths are then the trimmed ones, read back from the device once)."""
        from . import functional as GF
        wavs = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
        if not wavs:
            raise ValueError("no waveform")
        dev = wavs[0].device
        lengths = [int(w.numel()) for w in wavs]
        flat = wavs[0].detach().float().contiguous() if len(wavs) == 1 else torch.cat([w.detach().float().reshape(-1) for w in wavs])
        gain = None
        if self._resampling(source_rate):
            flat, lengths = GF.resample(self.resampler(source_rate, dev, resample_filter), flat, lengths, native=native)
            if normalize_volume:
                gain = GF.volume_gain(flat, lengths, self.target_dbfs, increase_only=True, native=native)
        elif normalize_volume:
            gain = volume_gain(flat, lengths, self.target_dbfs, increase_only=True)
        if trim_silences or voice_flags is not None:
            flat, lengths = GF.trim_silences(flat, lengths, gain=gain, voice_flags=voice_flags, window=self.vad_window,
                                             floor_span=self.vad_floor_span, ratio_db=self.vad_ratio_db,
                                             min_level_dbfs=self.vad_min_level_dbfs, avg_width=self.vad_moving_average_width,
                                             max_silence=self.vad_max_silence_length, native=native)
        return flat, lengths, gain

    def spectrogram(self, flat, lengths, gain=None, pad_to_partials: bool = False, mode: str = "db",
                    native: Optional[bool] = None):
        """``(frames, frame_start)`` of ``functional.melspec`` for what ``preprocess`` returned."""
        from . import functional as GF
        if not pad_to_partials:
            for u, n in enumerate(lengths):
                if n <= self.n_fft // 2:
                    raise ValueError(f"utterance {u} has {n} samples (after any silence trimming): the spectrogram's "
                                     f"reflection needs more than n_fft / 2 = {self.n_fft // 2}; pad_to_partials extends it")
        if flat.numel() == 0:
            flat = flat.new_zeros(1)          # every utterance trimmed to nothing: the kernel wants an address, reads nothing
        padded = [self.slices(n).padded_length for n in lengths] if pad_to_partials else None
        return GF.melspec(self.tables(flat.device), flat, lengths, hop=self.hop_length, padded_lengths=padded, gain=gain,
                          mode=mode, min_level_db=self.min_level_db, ref_level_db=self.ref_level_db, native=native)

    def frames(self, wavs, normalize_volume: bool = False, pad_to_partials: bool = False, mode: str = "db",
               native: Optional[bool] = None, source_rate: Optional[int] = None, resample_filter="kaiser_best",
               trim_silences: bool = False, voice_flags=None):
        """``(frames, frame_start)`` of ``functional.melspec`` for a list of 1-D float32 device waveforms (or one): all of
        them in one launch.  ``normalize_volume``: the gain of ``normalize_volume(increase_only=True)``, applied in the
        kernel.  ``pad_to_partials``: every waveform zero-extended to the end of its last partial slice, as
        ``get_mel_spects_from_audio(partial_slices=True)`` pads it.  ``source_rate`` / ``resample_filter``: the rate of
        the waveforms where it is not ``sampling_rate`` (see the class; None: they are at the model's rate).
        ``trim_silences`` / ``voice_flags``: the reference's silence trimming first (see the class); an utterance trimmed
        to ``n_fft / 2`` samples or fewer raises a ValueError unless ``pad_to_partials`` extends it."""
        flat, lengths, gain = self.preprocess(wavs, normalize_volume, native, source_rate, resample_filter, trim_silences,
                                              voice_flags)
        return self.spectrogram(flat, lengths, gain, pad_to_partials, mode, native)

    def partial_rows(self, lengths, frame_start, source_rate: Optional[int] = None, resample_filter=None):
        """``(row_start, owner)`` Python lists: the first row of ``frames(pad_to_partials=True)`` of every partial
        utterance and the waveform it belongs to; a partial whose frames the spectrogram does not hold is left out, as
        s0:59 leaves it out.  ``lengths``: the waveforms' own, at ``source_rate`` where that is given.
        ``resample_filter`` is accepted so that the three methods take the same arguments and is ignored: the rows
        depend on the lengths alone, which no filter changes.  After silence trimming the lengths are ``preprocess``'s
        (already at the model's rate: no ``source_rate`` then)."""
        rows, owner = [], []
        lengths = self.resampled_lengths(lengths, source_rate)
        for u, n in enumerate(lengths):
            have = frame_start[u + 1] - frame_start[u]
            for s in self.slices(n).mel_starts:
                if s + self.partials_n_frames <= have:
                    rows.append(frame_start[u] + s)
                    owner.append(u)
        return rows, owner

    def partials(self, wavs, normalize_volume: bool = False, native: Optional[bool] = None,
                 source_rate: Optional[int] = None, resample_filter="kaiser_best", trim_silences: bool = False,
                 voice_flags=None):
        """Per waveform the tensor ``get_mel_spects_from_audio(partial_slices=True)`` returns, (partials,
        partials_n_frames, n_mels) float32: gathered copies of the frames (``SpeakerEncoder.embed_audio`` addresses them
        in place instead).  ``source_rate`` / ``resample_filter`` / ``trim_silences`` / ``voice_flags`` as ``frames``; an
        utterance trimmed to nothing yields one partial of silence, as the reference does."""
        wavs = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
        flat, lengths, gain = self.preprocess(wavs, normalize_volume, native, source_rate, resample_filter, trim_silences,
                                              voice_flags)
        frames, frame_start = self.spectrogram(flat, lengths, gain, pad_to_partials=True, native=native)
        rows, owner = self.partial_rows(lengths, frame_start)
        T = self.partials_n_frames
        return [torch.stack([frames[r:r + T] for r, o in zip(rows, owner) if o == u]) if u in owner
                else frames.new_zeros(0, T, self.n_mels) for u in range(len(wavs))]
