"""The d-vector encoder the loss is trained with (the caller on the input side of the hot path).

Mirrors ``embedding_model_GE2E/s2_model_GE2E_loss_speach_embed.py:7-35``: a stacked LSTM over
(batch, frames, n_mels), the LAST frame's hidden state through one Linear, L2-normalised.  Attribute
names (``LSTM_stack``, ``projection``) and the initialisation (xavier-normal weights, zero biases
for the LSTM, s2:18-22; the Linear keeps torch's default) follow the reference so a reference
``state_dict`` loads here and the other way round (s4:130 saves exactly this module's).

In TRAINING the recurrent and projection GEMMs are by default library work (MIOpen / hipBLASLt through torch); what is
ours there is the tail: with ``normalize=False`` the module hands back the raw projection and the trainer runs the fused
L2-normalise + un-permute gather (``functional.normalize_unperm``) in one HIP kernel instead of three torch
ops.  With ``native_train=True`` the whole encoder is hand-written both ways: ``raw`` / ``forward`` go through
``functional.encode_train`` (csrc/ge2e_encoder_train.hip) -- a forward that keeps a tape, and the LSTM backward through
time, the projection's and the norm's backward in HIP -- and ``loss.backward()`` fills the ``.grad``s without the library.
It is opt-in: no speed is promised below a few thousand windows, and the tape costs 6 L H T 4 bytes a window.
For INFERENCE ``embed`` / ``embed_utterances`` run the whole forward pass -- LSTM stack, projection, norm -- as one
hand-written HIP launch (``functional.encode``, csrc/ge2e_encoder.hip); ``forward`` and ``raw`` stay torch's.
"""
from __future__ import annotations

import torch
import torch.nn as nn


# embed(native=None) takes the HIP kernel from this many windows on.  profiles/encoder_bench.txt (80 -> 3 x 256 -> 256,
# T = 160): the native call takes 32-33 ms for anything up to 8192 windows (one tile of 32 per CU), torch's route 12 ms up
# to 1024 windows, 28.9 ms at 4096 and 42.9 ms at 6144: the lines cross near 4700.
NATIVE_MIN_ROWS = 4800


class SpeakerEncoder(nn.Module):
    def __init__(self, n_mels: int = 80, hidden: int = 256, layers: int = 3, embedding: int = 256,
                 normalize: bool = True, *, native_train: bool = False):
        super().__init__()
        self.native_train = native_train
        self.LSTM_stack = nn.LSTM(n_mels, hidden, num_layers=layers, batch_first=True)  # s2:13-16
        for name, param in self.LSTM_stack.named_parameters():  # s2:18-22
            if "bias" in name:
                nn.init.constant_(param, 0.0)
            elif "weight" in name:
                nn.init.xavier_normal_(param)
        self.projection = nn.Linear(hidden, embedding)  # s2:25
        self.normalize = normalize
        self.embedding_size = embedding   # what the trainer needs to know before the forward: the loss kernel's D

    @classmethod
    def from_hp(cls, hp, normalize: bool = True):
        """Same constructor argument as the reference's class (s2:9)."""
        return cls(hp.audio.mel_n_channels, hp.m_ge2e.model_hidden_size, hp.m_ge2e.model_num_layers,
                   hp.m_ge2e.model_embedding_size, normalize=normalize).to(hp.general.device)

    def _native_train_route(self, x) -> bool:
        """native_train is set, gradients are wanted, the module has a kernel and the input is on a GPU."""
        return self.native_train and torch.is_grad_enabled() and x.is_cuda and self.native_supported()

    def _encode_train(self, x, normalize: bool):
        from . import functional as GF
        n_mels, H, L, D = self._shape()
        return GF.encode_train(self._parameters_in_pack_order(), x, hidden=H, layers=L, dim=D, normalize=normalize)

    def raw(self, x):
        if self._native_train_route(x):
            return self._encode_train(x, False)
        x, _ = self.LSTM_stack(x.float())       # s2:28
        return self.projection(x[:, x.size(1) - 1].float())  # s2:30-31

    def forward(self, x):
        if self.normalize and self._native_train_route(x):
            return self._encode_train(x, True)   # the kernel does the norm, and its backward
        y = self.raw(x)
        if not self.normalize:
            return y
        return y / torch.norm(y, dim=1).unsqueeze(1)  # s2:34


    # ---- inference without autograd: the native forward pass (functional.encode, csrc/ge2e_encoder.hip) ------------------
    def _shape(self):
        lstm = self.LSTM_stack
        return lstm.input_size, lstm.hidden_size, lstm.num_layers, self.projection.out_features

    def _parameters_in_pack_order(self):
        lstm = self.LSTM_stack
        ps = []
        for l in range(lstm.num_layers):
            ps += [getattr(lstm, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return ps + [self.projection.weight, self.projection.bias]

    def native_supported(self) -> bool:
        """Whether ``embed`` has a HIP kernel for this module: a plain float32 nn.LSTM stack of a supported shape on a GPU."""
        from . import functional as GF
        lstm = self.LSTM_stack
        plain = lstm.bias and lstm.batch_first and not lstm.bidirectional and getattr(lstm, "proj_size", 0) == 0 \
            and self.projection.bias is not None
        ps = self._parameters_in_pack_order() if plain else []
        return bool(plain) and all(p.is_cuda and p.dtype == torch.float32 for p in ps) and GF.encode_supported(*self._shape())

    def packed_weights(self) -> torch.Tensor:
        """The packed buffer ``functional.encode`` streams from, cached against the parameters' ``_version`` counters,
        their storage and device: an optimiser step, ``load_state_dict`` or ``.to()`` repacks."""
        from . import functional as GF
        ps = self._parameters_in_pack_order()
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in ps)
        cache = getattr(self, "_packed_cache", None)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1) for p in ps])
                cache = (key, GF.encoder_pack(flat, *self._shape()))
            self._packed_cache = cache
        return cache[1]

    def embed(self, x, native=None, normalize=None):
        """Inference without autograd: (R, T, n_mels) mel windows -> (R, D) d-vectors.  ``native=True`` is the HIP kernel
        (one launch; a row's bits do not depend on the batch it is in) and raises where there is none; ``native=False`` is
        torch's modules under ``no_grad``; ``native=None`` takes the kernel where ``native_supported()`` and the batch has
        at least ``NATIVE_MIN_ROWS`` windows -- below that the library was measured faster -- and torch's route
        otherwise.  ``normalize=None``: the module's own setting.  A callable for the loops of ``evaluation``."""
        from . import functional as GF
        normalize = self.normalize if normalize is None else normalize
        ok = self.native_supported() and x.is_cuda
        if native and not ok:
            raise RuntimeError(f"SpeakerEncoder.embed(native=True): no HIP kernel for (n_mels, hidden, layers, dim) = "
                               f"{self._shape()} with float32 parameters and input on a GPU")
        if native or (native is None and ok and x.shape[0] >= NATIVE_MIN_ROWS):
            n_mels, H, L, D = self._shape()
            return GF.encode(self.packed_weights(), x, hidden=H, layers=L, dim=D, normalize=normalize)
        with torch.no_grad():
            y = self.raw(x)
            return y / torch.norm(y, dim=1).unsqueeze(1) if normalize else y

    def embed_utterances(self, mels, window: int = 160, hop: int = 80):
        """Utterance d-vectors (len(mels), D) from whole spectrograms (F_i, n_mels): every window of ``window`` frames at
        hops of ``hop`` is encoded -- ONE native call over the concatenated frames, the windows addressed in place -- and an
        utterance's normalised window d-vectors are averaged and renormalised by ``enroll_accumulate`` /
        ``enroll_finalize`` with the utterance number as the label."""
        from . import functional as GF
        if not self.native_supported():
            raise RuntimeError(f"embed_utterances needs the native encoder kernel; this module {self._shape()} has none")
        if len(mels) < 1 or window < 1 or hop < 1:
            raise ValueError("embed_utterances needs at least one spectrogram and window, hop >= 1")
        n_mels, H, L, D = self._shape()
        dev = self.projection.weight.device
        starts, labels, base = [], [], 0
        for u, m in enumerate(mels):
            if m.dim() != 2 or m.shape[1] != n_mels:
                raise ValueError(f"spectrogram {u} must be (frames, {n_mels}), got {tuple(m.shape)}")
            if m.shape[0] < window:
                raise ValueError(f"spectrogram {u} has {m.shape[0]} frames, fewer than one window of {window}")
            n = (m.shape[0] - window) // hop + 1
            starts += [base + i * hop for i in range(n)]
            labels += [u] * n
            base += m.shape[0]
        flat = torch.cat([torch.as_tensor(m).to(dev).float() for m in mels])
        row_start = torch.tensor(starts, dtype=torch.int64).to(dev)
        e = GF.encode(self.packed_weights(), flat, T=window, row_start=row_start, hidden=H, layers=L, dim=D, normalize=True)
        sums = torch.zeros(len(mels), D, dtype=torch.float32, device=dev)
        cnt = torch.zeros(len(mels), dtype=torch.int32, device=dev)
        GF.enroll_accumulate(sums, cnt, e, torch.tensor(labels, dtype=torch.int32).to(dev))
        return GF.enroll_finalize(sums, cnt)


    def embed_audio(self, wavs, front_end, normalize_volume: bool = False, source_rate=None,
                    resample_filter="kaiser_best", trim_silences: bool = False, voice_flags=None):
        """Utterance d-vectors (len(wavs), D) from waveforms (1-D float32 tensors on the module's device), as the
        reference makes them from ``get_mel_spects_from_audio(partial_slices=True)``: three launches and no copy between
        them.  ``front_end`` (an ``audio.MelFrontEnd``) turns all the waveforms, each zero-extended to the end of its last
        partial slice, into one flat frame buffer (``functional.melspec``); every partial utterance of
        ``partials_n_frames`` frames is encoded where it lies (``functional.encode`` with ``row_start``); an utterance's
        normalised partial d-vectors are averaged and renormalised by ``enroll_accumulate`` / ``enroll_finalize``.
        ``source_rate``: the rate of the waveforms where it is not the front end's ``sampling_rate``; they are then
        resampled on the device first (one more launch, ``functional.resample`` with ``resample_filter``; see
        ``audio.MelFrontEnd``).  One rate for all the waveforms of a call.  ``trim_silences`` / ``voice_flags``: the
        reference's ``trim_long_silences`` between the gain and the spectrogram (``functional.trim_silences``: four more
        launches and one read-back of the kept lengths; the built-in voice flags are the project's own detector, not
        webrtcvad's -- pass other flags as ``voice_flags``).  An utterance trimmed to nothing gives the d-vector of one
        partial of silence, as the reference does."""
        from . import functional as GF
        if not self.native_supported():
            raise RuntimeError(f"embed_audio needs the native encoder kernel; this module {self._shape()} has none")
        wavs = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
        n_mels, H, L, D = self._shape()
        if front_end.n_mels != n_mels:
            raise ValueError(f"the front end makes {front_end.n_mels} mel channels, the encoder takes {n_mels}")
        dev = self.projection.weight.device
        flat, lengths, gain = front_end.preprocess([w.to(dev) for w in wavs], normalize_volume, source_rate=source_rate,
                                                   resample_filter=resample_filter, trim_silences=trim_silences,
                                                   voice_flags=voice_flags)
        frames, frame_start = front_end.spectrogram(flat, lengths, gain, pad_to_partials=True)
        rows, owner = front_end.partial_rows(lengths, frame_start)
        if sorted(set(owner)) != list(range(len(wavs))):
            raise ValueError("a waveform has no whole partial utterance in its spectrogram (hop_length above the slices' step)")
        idx = torch.tensor([rows, owner], dtype=torch.int64).to(dev)
        e = GF.encode(self.packed_weights(), frames, T=front_end.partials_n_frames, row_start=idx[0], hidden=H, layers=L,
                      dim=D, normalize=True)
        sums = torch.zeros(len(wavs), D, dtype=torch.float32, device=dev)
        cnt = torch.zeros(len(wavs), dtype=torch.int32, device=dev)
        GF.enroll_accumulate(sums, cnt, e, idx[1].to(torch.int32))
        return GF.enroll_finalize(sums, cnt)


def get_pre_trained_embedding_model(hp,use_path_as_absolute: bool = False) -> SpeakerEncoder:
    """The reference's loader of the same name (s2:38-67): a fresh encoder built from ``hp``, the encoder-only checkpoint
    ``hp.m_ge2e.best_model_path`` (joined with ``hp.general.project_root`` unless ``use_path_as_absolute``) loaded into
    it, eval mode, on ``hp.general.device``.  The file format is the reference's (s4:130: the module's ``state_dict``),
    which is also what ``DPTrainer.save_checkpoint`` writes."""
    import os
    model = SpeakerEncoder.from_hp(hp)
    path = hp.m_ge2e.best_model_path if use_path_as_absolute else os.path.join(hp.general.project_root, hp.m_ge2e.best_model_path)
    model.load_state_dict(torch.load(path, map_location=hp.general.device))
    return model.eval().to(hp.general.device)
