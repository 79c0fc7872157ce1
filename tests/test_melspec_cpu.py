"""CPU: the host side of the mel front end -- ge2e_melspec_packed_bytes / ge2e_melspec_pack / ge2e_melspec /
ge2e_melspec_plan: declared, exported and bound, the packed size, every error code and the order of the checks, the plan --
and tests/melspec_ref.py, the float64 reference of the GPU tests, together with audio.py's host arithmetic (filterbank,
window, partial slices, volume gain), held to what the reference's own AudioUtils computed
(tests/golden/callers/melspec.npz, written by tests/golden/make_melspec_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import melspec_ref as mr
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, audio, build

SYMS = ("ge2e_melspec_packed_bytes", "ge2e_melspec_pack", "ge2e_melspec", "ge2e_melspec_plan")
ERR_NULL, ERR_SHAPE, ERR_IMPL, ERR_ALIGN = -1, -2, -5, -6
I, P, LL, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
GOLD = os.path.join(os.path.dirname(__file__), "golden", "callers", "melspec.npz")
CASES = ("c0", "c1", "c2")


def fixture(name):
    z = np.load(GOLD)
    c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    sr, n_fft, hop, step, n_mels, pframes = (int(v) for v in c["cfg"][:6])
    c.update(sr=sr, n_fft=n_fft, hop=hop, step=step, n_mels=n_mels, pframes=pframes, rate=float(c["cfg"][6]),
             min_coverage=float(c["cfg"][7]), target=float(c["cfg"][8]))
    return c


def test_fixture_is_what_the_issue_asks_for():
    shapes = {n: (fixture(n)["full"].shape, fixture(n)["partial"].shape) for n in CASES}
    assert shapes["c0"] == ((163, 80), (1, 180, 80))
    assert shapes["c1"][1] == (1, 20, 40) and shapes["c2"][1] == (3, 20, 40)
    assert (fixture("c0")["n_fft"], fixture("c1")["n_fft"], fixture("c2")["n_fft"]) == (1024, 256, 512)
    assert len(fixture("c2")["mel_slices"]) == 3                      # the fourth was dropped by min_coverage
    assert fixture("c0")["wav"].dtype == np.float32 and fixture("c0")["full"].dtype == np.float64
    assert os.path.getsize(GOLD) < os.path.getsize(os.path.join(os.path.dirname(GOLD), "encoder_weights.npz"))


@pytest.mark.parametrize("name", CASES)
def test_melspec_ref_reproduces_the_references_float64_output(name):
    c = fixture(name)
    _, full = mr.melspec_ref(c["wav"], c["basis"], c["n_fft"], c["hop"])
    assert full.shape == c["full"].shape == (len(c["wav"]) // c["hop"] + 1, c["n_mels"])
    assert np.abs(full - c["full"]).max() <= 1e-12
    padded = max(len(c["wav"]), int(c["wav_slices"][-1, 1]))
    _, db = mr.melspec_ref(c["wav"], c["basis"], c["n_fft"], c["hop"], padded_len=padded)
    part = np.stack([db[a:b] for a, b in c["mel_slices"] if db[a:b].shape[0] == c["pframes"]])
    assert np.abs(part - c["partial"]).max() <= 1e-12
    # ... and the float32 yardstick is a float32 computation, close to it
    m32, db32 = mr.melspec_ref(c["wav"], c["basis"], c["n_fft"], c["hop"], dtype=np.float32)
    assert m32.dtype == np.float32 and db32.dtype == np.float32 and np.abs(db32 - full).max() < 1e-5


@pytest.mark.parametrize("name", CASES)
def test_filterbank_window_and_slices_agree_with_the_reference(name):
    c = fixture(name)
    for basis in (mr.mel_filterbank(c["sr"], c["n_fft"], c["n_mels"], 90, 7600).T,
                  audio.mel_filterbank(c["sr"], c["n_fft"], c["n_mels"], 90.0, 7600.0).numpy()):
        assert basis.shape == c["basis"].shape == (c["n_fft"] // 2 + 1, c["n_mels"]) and basis.dtype == np.float64
        assert np.abs(basis - c["basis"]).max() <= 1e-12
        assert ((basis > 0).sum(axis=0) > 0).all()                    # every filter is non-empty
        assert (basis > 0).sum(axis=1).max() <= 2                     # at most two filters meet in a bin
    w = audio.hann_window(c["n_fft"])
    assert w.dtype == torch.float64 and np.abs(w.numpy() - mr.hann(c["n_fft"])).max() <= 1e-15 and w[0] == 0
    s = audio.partial_slices(len(c["wav"]), sampling_rate=c["sr"], mel_window_step=c["step"],
                             partials_n_frames=c["pframes"], rate=c["rate"], min_coverage=c["min_coverage"])
    assert s.mel_starts == c["mel_slices"][:, 0].tolist()
    assert s.padded_length == max(len(c["wav"]), int(c["wav_slices"][-1, 1]))
    assert all(b - a == c["pframes"] for a, b in c["mel_slices"])


def test_partial_slices_over_many_lengths_against_the_formula():
    # the loop of s0:183-197 restated literally
    for n in list(range(1, 4000, 37)) + [16000, 20800, 47000, 160 * 180, 160 * 180 - 1]:
        for pframes, rate in ((180, 1.3), (20, 10.0), (20, 5.0)):
            spf, n_frames, step = 160, int(np.ceil((n + 1) / 160)), int(np.round((16000 / rate) / 160))
            starts = list(range(0, max(1, n_frames - pframes + step + 1), step))
            if (n - starts[-1] * spf) / (pframes * spf) < 0.75 and len(starts) > 1:
                starts = starts[:-1]
            s = audio.partial_slices(n, partials_n_frames=pframes, rate=rate)
            assert s.mel_starts == starts and s.padded_length == max(n, (starts[-1] + pframes) * spf), (n, pframes, rate)
    with pytest.raises(ValueError):
        audio.partial_slices(1000, partials_n_frames=20, rate=1.3)     # a step of 77 frames: the rate is too low


def test_frame_count_formula():
    # P // hop + 1 is the reference's (len + n_fft - (n_fft - hop)) // hop for every length, hop and n_fft
    for n_fft in (256, 400, 1024):
        for hop in (1, 64, 160, 1500):
            for P in (n_fft // 2 + 1, 777, 2 * hop, 2 * hop + 1, 3 * hop - 1):
                assert (P + 2 * (n_fft // 2) - (n_fft - hop)) // hop == P // hop + 1
                if P > n_fft // 2:
                    assert mr.magnitudes(np.zeros(P), n_fft, hop).shape == (P // hop + 1, n_fft // 2 + 1)


@pytest.mark.parametrize("name", CASES)
def test_volume_gain_on_cpu_tensors(name):
    c = fixture(name)
    wav = torch.from_numpy(c["wav"])
    g = audio.volume_gain(wav, target_dbfs=c["target"], increase_only=True)
    assert g.shape == (1,) and g.dtype == torch.float32
    assert np.allclose(c["wav"] * g.numpy(), c["normed"], rtol=1e-5, atol=0)
    # three utterances in one buffer: each has its own gain; a loud one is left alone
    both = torch.cat([wav, wav * 0.01, wav * 100.0])
    g3 = audio.volume_gain(both, [len(wav)] * 3, target_dbfs=c["target"]).numpy()
    rms = float(np.sqrt(np.mean(c["wav"].astype(np.float64) ** 2)))
    want = [10 ** ((c["target"] - 20 * np.log10(r)) / 20) if 20 * np.log10(r) < c["target"] else 1.0
            for r in (rms, rms * 0.01, rms * 100.0)]
    assert np.allclose(g3, want, rtol=1e-5) and g3[2] == 1.0
    assert np.allclose(audio.volume_gain(both, [len(wav)] * 3, target_dbfs=c["target"], increase_only=False).numpy()[2],
                       10 ** ((c["target"] - 20 * np.log10(rms * 100.0)) / 20), rtol=1e-5)


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_melspec_packed_bytes"] == (ctypes.c_size_t, [I, I])
    assert _lib.PROTOTYPES["ge2e_melspec_pack"] == (I, [P, P, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_melspec"] == (I, [P] * 7 + [I, LL, I, I, I, I, F, F, P, P])
    assert _lib.PROTOTYPES["ge2e_melspec_plan"] == (I, [I, LL, I, I, I, ctypes.c_char_p, ctypes.c_size_t])
    atoms = _lib.plan_atoms()
    assert len(atoms) == 94 and not any(a.startswith("melspec") for a in atoms)
    import speaker_embedding_ge2e_loss_amd as pkg
    from speaker_embedding_ge2e_loss_amd import functional as GF
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    assert pkg.MelFrontEnd is audio.MelFrontEnd and hasattr(SpeakerEncoder, "embed_audio")
    for f in ("melspec_supported", "melspec_pack", "melspec", "melspec_layout"):
        assert callable(getattr(GF, f))


def test_packed_bytes_is_zero_exactly_for_the_unsupported_shapes(lib):
    f = lib.ge2e_melspec_packed_bytes
    for n_fft in (256, 512, 1024, 2048):
        for n_mels in (1, 13, 16, 80, 128):
            want = 4 * (3 * n_fft + (n_fft // 2 + 4) * ((n_mels + 15) // 16 * 16))
            assert f(n_fft, n_mels) == want and want % 16 == 0, (n_fft, n_mels)
    for bad in ((400, 80), (128, 80), (4096, 80), (1000, 40), (0, 80), (-1024, 80), (1023, 80), (1024, 0), (1024, 129),
                (1024, -80), (512, 200)):
        assert f(*bad) == 0, bad
    from speaker_embedding_ge2e_loss_amd import functional as GF
    assert GF.melspec_supported(1024, 80) and GF.melspec_supported(512, 40) and not GF.melspec_supported(400, 40)


def test_pack_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_melspec_pack
    ok = dict(window=16, basis=32, n_fft=1024, n_mels=80, packed=48, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("window", "basis", "packed"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(n_mels=0) == ERR_SHAPE and call(n_mels=-4) == ERR_SHAPE
    for kw in (dict(n_fft=400), dict(n_fft=0), dict(n_fft=128), dict(n_fft=4096), dict(n_mels=129)):
        assert call(**kw) == ERR_IMPL, kw
    assert call(packed=40) == ERR_ALIGN and call(packed=52) == ERR_ALIGN
    assert call(window=20, basis=36, packed=40) == ERR_ALIGN          # (only packed is read sixteen bytes at a time)
    # the order: NULL, shape, implementation, alignment
    assert call(packed=None, n_mels=0) == ERR_NULL and call(basis=None, n_fft=400, packed=40) == ERR_NULL
    assert call(n_mels=0, n_fft=400) == ERR_SHAPE and call(n_mels=0, packed=40) == ERR_SHAPE
    assert call(n_fft=400, packed=40) == ERR_IMPL


def test_melspec_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_melspec
    ok = dict(packed=16, wav=36, utt_start=64, utt_len=72, utt_padded_len=None, gain=None, frame_start=80, U=2,
              total_frames=40, n_fft=1024, hop=128, n_mels=80, mode=1, min_level_db=-100.0, ref_level_db=16.0, out=96,
              stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("packed", "wav", "utt_start", "utt_len", "frame_start", "out"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("U", "hop", "n_mels", "total_frames"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -3}) == ERR_SHAPE, k
    for kw in (dict(mode=2), dict(mode=-1), dict(min_level_db=0.0), dict(min_level_db=20.0), dict(min_level_db=float("nan"))):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(n_fft=400), dict(n_fft=0), dict(n_fft=-1024), dict(n_fft=128), dict(n_fft=4096), dict(n_mels=129),
               dict(total_frames=16 * 2 ** 31)):
        assert call(**kw) == ERR_IMPL, kw
    for kw in (dict(packed=24), dict(packed=20), dict(out=104), dict(out=100), dict(wav=38), dict(wav=33)):
        assert call(**kw) == ERR_ALIGN, kw
    # the order: NULL, shape, implementation, alignment
    assert call(out=None, U=0) == ERR_NULL and call(wav=None, n_fft=400) == ERR_NULL and call(packed=None, out=100) == ERR_NULL
    assert call(hop=0, n_fft=400) == ERR_SHAPE and call(mode=3, out=100) == ERR_SHAPE
    assert call(min_level_db=1.0, n_mels=129, wav=33) == ERR_SHAPE
    assert call(n_fft=400, out=100) == ERR_IMPL and call(n_mels=200, packed=24) == ERR_IMPL


def test_melspec_plan_names_the_instantiation_and_the_grid(lib):
    assert _lib.melspec_plan(1, 163, 1024, 128, 80) == ["melspec<1024>/11"]
    assert _lib.melspec_plan(3, 16, 512, 160, 40) == ["melspec<512>/1"]
    assert _lib.melspec_plan(3, 17, 256, 64, 13) == ["melspec<256>/2"]
    assert _lib.melspec_plan(1, 2 ** 33, 2048, 1, 128) == ["melspec<2048>/%d" % 2 ** 29]
    assert lib.ge2e_melspec_plan(1, 163, 1024, 128, 80, None, 0) == len("melspec<1024>/11")   # measures
    assert lib.ge2e_melspec_plan(0, 163, 1024, 128, 80, None, 0) == ERR_SHAPE
    assert lib.ge2e_melspec_plan(1, 163, 400, 128, 80, None, 0) == ERR_IMPL
    assert lib.ge2e_melspec_plan(1, 0, 400, 128, 80, None, 0) == ERR_SHAPE                      # shape before implementation
    with pytest.raises(ValueError):
        _lib.melspec_plan(1, 163, 400, 128, 80)


def test_layout_is_host_arithmetic():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    lay = GF.melspec_layout([2500, 6500, 300], hop=160, n_fft=512, padded_lengths=[3200, 6500, 300], device="cpu")
    assert lay.frame_start == [0, 21, 62, 64] and lay.utt_start.tolist() == [0, 2500, 9000]
    assert lay.utt_padded_len.tolist() == [3200, 6500, 300] and lay.frame_start_dev.tolist() == lay.frame_start
    for bad in (dict(lengths=[256], padded_lengths=None), dict(lengths=[300], padded_lengths=[299]), dict(lengths=[], padded_lengths=None)):
        with pytest.raises(ValueError):
            GF.melspec_layout(bad["lengths"], hop=160, n_fft=512, padded_lengths=bad["padded_lengths"], device="cpu")
