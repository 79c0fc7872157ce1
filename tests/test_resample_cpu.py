"""CPU: the host side of the resampling stage -- ge2e_resample_packed_bytes / ge2e_resample_pack / ge2e_resample /
ge2e_resample_plan / ge2e_volume_gain_workspace_bytes / ge2e_volume_gain: declared, exported and bound, the packed size,
every error code and the order of the checks, the plan -- and tests/resample_ref.py, the float64 oracle of the GPU tests,
together with audio.py's host arithmetic (the bank, the lengths): the oracle resamples a sine to what the sine is at the new
rate, and agrees with scipy.signal.upfirdn where that computes the same sum."""
import ctypes
import re

import numpy as np
import pytest
import torch

import resample_ref as rr
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, audio, build

SYMS = ("ge2e_resample_packed_bytes", "ge2e_resample_pack", "ge2e_resample", "ge2e_resample_plan",
        "ge2e_volume_gain_workspace_bytes", "ge2e_volume_gain")
ERR_NULL, ERR_SHAPE, ERR_IMPL, ERR_ALIGN = -1, -2, -5, -6
I, P, LL, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_resample_packed_bytes"] == (ctypes.c_size_t, [I, I, I])
    assert _lib.PROTOTYPES["ge2e_resample_pack"] == (I, [P, I, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_resample"] == (I, [P] * 5 + [I, LL, I, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_resample_plan"] == (I, [I, LL, I, I, I, ctypes.c_char_p, ctypes.c_size_t])
    assert _lib.PROTOTYPES["ge2e_volume_gain_workspace_bytes"] == (ctypes.c_size_t, [LL, I])
    assert _lib.PROTOTYPES["ge2e_volume_gain"] == (I, [P, P, P, I, F, I, P, P, P])
    assert not any(a.startswith(("resample", "gain")) for a in _lib.plan_atoms())
    from speaker_embedding_ge2e_loss_amd import functional as GF
    for f in ("resample_supported", "resample_pack", "resample_layout", "resample", "volume_gain"):
        assert callable(getattr(GF, f))
    for f in ("resample_bank", "resampled_length"):
        assert callable(getattr(audio, f))
    assert hasattr(audio.MelFrontEnd, "resampler")


def test_packed_bytes_is_zero_exactly_for_the_unsupported_shapes(lib):
    f = lib.ge2e_resample_packed_bytes
    for L in (1, 2, 3, 160, 320, 639, 640):
        for M in (1, 3, 441, 640):
            for W in (1, 3, 129, 355, 385, 1025):
                want = 4 * W * ((L + 3) // 4 * 4)
                assert f(L, M, W) == want and want % 16 == 0, (L, M, W)
    for bad in ((0, 3, 13), (-1, 3, 13), (641, 3, 13), (1, 0, 13), (1, -3, 13), (1, 641, 13), (1, 3, 0), (1, 3, -1), (1, 3, 12),
                (1, 3, 1024), (1, 3, 1027), (160, 441, 354), (2 ** 30, 2 ** 30, 3)):
        assert f(*bad) == 0, bad
    # the rates of the issue to 16 kHz under both presets have a kernel; the banks have the sizes of its table
    from speaker_embedding_ge2e_loss_amd import functional as GF
    for sr in RATES:
        for name in ("kaiser_best", "kaiser_fast"):
            b = audio.resample_bank(sr, 16000, name)
            assert GF.resample_supported(b.up, b.down, 2 * b.lead + 1), (sr, name)
    sizes = {sr: (b.up, b.down, 2 * b.lead + 1) for sr in (48000, 44100, 22050, 11025) for b in [audio.resample_bank(sr, 16000)]}
    assert sizes == {48000: (1, 3, 385), 44100: (160, 441, 355), 22050: (320, 441, 179), 11025: (640, 441, 129)}
    assert not GF.resample_supported(147, 641, 13) and not GF.resample_supported(1, 3, 14)


def test_pack_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_resample_pack
    ok = dict(taps=16, L=160, M=441, lead=5, packed=48, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("taps", "packed"):
        assert call(**{k: None}) == ERR_NULL, k
    for kw in (dict(L=0), dict(L=-2), dict(M=0), dict(M=-441), dict(lead=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(L=641), dict(M=641), dict(lead=513), dict(lead=2 ** 30), dict(lead=2 ** 31 - 1)):
        assert call(**kw) == ERR_IMPL, kw
    assert call(packed=40) == ERR_ALIGN and call(packed=52) == ERR_ALIGN
    assert call(taps=20, packed=40) == ERR_ALIGN                      # (only packed is read sixteen bytes at a time)
    # the order: NULL, shape, implementation, alignment
    assert call(packed=None, L=0) == ERR_NULL and call(taps=None, L=641, packed=40) == ERR_NULL
    assert call(L=0, M=641) == ERR_SHAPE and call(lead=-1, packed=40) == ERR_SHAPE
    assert call(L=641, packed=40) == ERR_IMPL


def test_resample_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_resample
    ok = dict(packed=16, wav=36, in_start=64, in_len=72, out_start=80, U=2, total_out=40, L=160, M=441, lead=5, out=96,
              stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("packed", "wav", "in_start", "in_len", "out_start", "out"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("U", "L", "M", "total_out"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -3}) == ERR_SHAPE, k
    assert call(lead=-1) == ERR_SHAPE
    for kw in (dict(L=641), dict(M=641), dict(lead=513), dict(lead=2 ** 31 - 1), dict(total_out=2 ** 62)):
        assert call(**kw) == ERR_IMPL, kw
    for kw in (dict(packed=24), dict(packed=20), dict(out=104), dict(out=100), dict(wav=38), dict(wav=33)):
        assert call(**kw) == ERR_ALIGN, kw
    # the order: NULL, shape, implementation, alignment
    assert call(out=None, U=0) == ERR_NULL and call(wav=None, L=641) == ERR_NULL and call(packed=None, out=100) == ERR_NULL
    assert call(M=0, L=641) == ERR_SHAPE and call(total_out=0, out=100) == ERR_SHAPE and call(lead=-1, L=641, wav=33) == ERR_SHAPE
    assert call(L=641, out=100) == ERR_IMPL and call(lead=600, packed=24) == ERR_IMPL


def test_volume_gain_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_volume_gain
    ok = dict(wav=36, utt_start=64, utt_len=72, U=2, target=-30.0, increase_only=1, gain_out=100, workspace=256, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("wav", "utt_start", "utt_len", "gain_out", "workspace"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(U=0) == ERR_SHAPE and call(U=-1) == ERR_SHAPE
    for kw in (dict(workspace=264), dict(workspace=260), dict(wav=38), dict(gain_out=101)):
        assert call(**kw) == ERR_ALIGN, kw
    assert call(wav=None, U=0) == ERR_NULL and call(U=0, wav=38) == ERR_SHAPE
    w = lib.ge2e_volume_gain_workspace_bytes
    assert w(1000, 3) == 3 * 128 * 8 and w(0, 1) == 128 * 8 and w(2 ** 40, 1) == 128 * 8
    assert w(1000, 0) == 0 and w(-1, 3) == 0


def test_resample_plan_names_the_instantiation_the_tile_and_the_grid(lib):
    assert _lib.resample_plan(1, 100000, 1, 3, 192) == ["resample<lds,8>/2048/49"]          # 48 kHz -> 16 kHz, kaiser_best
    assert _lib.resample_plan(3, 5000, 160, 441, 177) == ["resample<lds,2>/2560/4"]          # 44.1 kHz -> 16 kHz
    assert _lib.resample_plan(1, 2047, 2, 1, 64) == ["resample<lds,8>/2048/1"]               # 8 kHz -> 16 kHz
    assert _lib.resample_plan(2, 1024, 1, 640, 1) == ["resample<global,4>/1024/3"]           # a span LDS does not hold
    assert _lib.resample_plan(1, 2 ** 40, 1, 1, 0) == ["resample<lds,8>/2048/%d" % (2 ** 29 + 1)]
    assert lib.ge2e_resample_plan(1, 100000, 1, 3, 192, None, 0) == len("resample<lds,8>/2048/49")   # measures
    assert lib.ge2e_resample_plan(0, 100, 1, 3, 192, None, 0) == ERR_SHAPE
    assert lib.ge2e_resample_plan(1, 100, 641, 3, 192, None, 0) == ERR_IMPL
    assert lib.ge2e_resample_plan(1, 0, 641, 3, 192, None, 0) == ERR_SHAPE                   # shape before implementation
    with pytest.raises(ValueError):
        _lib.resample_plan(1, 100, 1, 3, 513)
    # every supported ratio of the issue's rates: a tile is a multiple of L and its LDS span within 40 KB
    for sr in RATES:
        for name in ("kaiser_best", "kaiser_fast"):
            b = audio.resample_bank(sr, 16000, name)
            kind, tile, grid = re.fullmatch(r"resample<(\w+),(\d)>/(\d+)/(\d+)", _lib.resample_plan(2, 10 ** 6, b.up, b.down, b.lead)[0]).group(1, 3, 4)
            assert kind == "lds" and int(tile) % b.up == 0 and int(grid) == 10 ** 6 // int(tile) + 2, (sr, name)


def test_layout_and_lengths_against_the_ceil_formula():
    from fractions import Fraction
    from math import ceil
    from speaker_embedding_ge2e_loss_amd import functional as GF
    lengths = list(range(0, 70)) + [159, 160, 161, 440, 441, 442, 16000, 44100, 48001, 2 ** 33 + 1]
    for L, M in ((1, 1), (1, 3), (2, 1), (2, 3), (3, 2), (160, 441), (320, 441), (640, 441), (1, 6), (2, 3)):
        want = [ceil(Fraction(n * L, M)) for n in lengths]
        assert [audio.resampled_length(n, L, M) for n in lengths] == want == [rr.out_length(n, L, M) for n in lengths]
        lay = GF.resample_layout(lengths, L, M, device="cpu")
        assert lay.out_lengths == want and lay.out_start == [0] + np.cumsum(np.array(want, dtype=object)).tolist()
        assert lay.in_len.tolist() == lengths and lay.in_start.tolist() == [0] + np.cumsum(np.array(lengths, dtype=object)).tolist()[:-1]
        assert lay.out_start_dev.tolist() == lay.out_start and (lay.up, lay.down) == (L, M)
    lay = GF.resample_layout(torch.tensor([3, 0, 5]), 1, 3, device="cpu")
    assert lay.out_start == [0, 1, 1, 3] and lay.in_start.tolist() == [0, 3, 3]
    for bad in (dict(lengths=[], up=1, down=3), dict(lengths=[-1], up=1, down=3), dict(lengths=[5], up=0, down=3),
                dict(lengths=[5], up=1, down=0)):
        with pytest.raises(ValueError):
            GF.resample_layout(device="cpu", **bad)
    fe = audio.MelFrontEnd()
    assert fe.resampled_lengths([48000, 7], 48000) == [16000, 3] and fe.resampled_lengths([44100, 1], 44100) == [16000, 1]
    assert fe.resampled_lengths([123], None) == [123] and fe.resampled_lengths([123], 16000) == [123]


def test_volume_gain_reads_any_layout_through_one_accessor():
    """The three layout types hand out the same utterance starts and lengths (what volume_gain's kernel reads, whichever
    layout it is given); the torch route of volume_gain takes ``lengths`` and ignores a layout, so with each of them it
    returns audio.volume_gain's values."""
    from speaker_embedding_ge2e_loss_amd import functional as GF
    lengths = [700, 300, 1500, 260]
    layouts = [GF.melspec_layout(lengths, hop=160, n_fft=512, device="cpu"), GF.resample_layout(lengths, 160, 441, device="cpu"),
               GF.vad_layout(lengths, 480, device="cpu")]
    wav = torch.as_tensor(0.05 * np.random.default_rng(3).standard_normal(sum(lengths)).astype(np.float32))
    want = audio.volume_gain(wav, lengths)
    for lay in layouts:
        starts, lens, ls = GF._utterances(lay)
        assert starts.tolist() == [0, 700, 1000, 2500] and lens.tolist() == lengths == ls
        assert starts.dtype == lens.dtype == torch.int64 and starts.device == lens.device == torch.device("cpu")
        GF._check_fits(starts, ls, wav)
        assert torch.equal(GF.volume_gain(wav, lengths, native=False, layout=lay), want)
        with pytest.raises(ValueError):
            GF._check_fits(starts, ls, wav[:-1])
    with pytest.raises(TypeError):
        GF._utterances((layouts[0][0], layouts[0][1]))


@pytest.mark.parametrize("name", ["kaiser_best", "kaiser_fast"])
def test_the_bank_is_the_formula_and_its_phases_sum_to_one(name):
    worst = 0.0
    for sr in RATES + (16000,):
        b = audio.resample_bank(sr, 16000, name)
        L, M = rr.ratio(sr, 16000)
        lead, taps = rr.bank(L, M, *rr.PRESETS[name])
        assert (b.up, b.down, b.lead) == (L, M, lead) and b.taps.dtype == torch.float64 and tuple(b.taps.shape) == (L, 2 * lead + 1)
        assert np.abs(b.taps.numpy() - taps).max() <= 1e-14, (sr, np.abs(b.taps.numpy() - taps).max())
        assert audio.resample_bank(sr, 16000, rr.PRESETS[name]).taps.equal(b.taps)
        worst = max(worst, np.abs(taps.sum(axis=1) - 1.0).max())
        assert np.abs(b.taps.numpy().sum(axis=1) - 1.0).max() <= 1e-4, sr
    print(f"{name}: the tap sums of a phase are within {worst:.2e} of 1")
    with pytest.raises(ValueError):
        audio.resample_bank(48000, 16000, "sinc_best")
    with pytest.raises(ValueError):
        audio.resample_bank(0, 16000)


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
@pytest.mark.parametrize("name,bound", [("kaiser_best", 1e-7), ("kaiser_fast", 1e-4)])
def test_the_oracle_resamples_a_sine(sr, name, bound):
    b = audio.resample_bank(sr, 16000, name)
    x = np.sin(2 * np.pi * 440.0 * np.arange(int(0.1 * sr)) / sr)
    y, _ = rr.resample_ref(x, b.taps.numpy(), b.up, b.down, b.lead)
    assert len(y) == 1600
    edge = int(np.ceil(b.lead * b.up / b.down)) + 1                          # outputs whose window leaves the signal
    want = np.sin(2 * np.pi * 440.0 * np.arange(1600) / 16000.0)
    err = np.abs(y - want)[edge:-edge].max()
    print(f"{sr} -> 16000 {name}: mid-signal error {err:.2e}")
    assert 1600 - 2 * edge > 800 and err < bound, (sr, name, err)


@pytest.mark.parametrize("L,M", [(1, 3), (160, 441), (2, 1), (2, 3)])
def test_the_oracle_is_upfirdn(L, M):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(L * 1000 + M)
    lead = 2 * M                                                              # a multiple of M: the shift is a whole number
    W = 2 * lead + 1
    taps = rng.standard_normal((L, W))
    x = rng.standard_normal(300)
    h = np.zeros(L * W)
    for p in range(L):
        h[p + np.arange(W) * L] = taps[p]
    full = signal.upfirdn(h, x, L, M)
    shift = lead * L // M
    assert (lead * L) % M == 0
    y, _ = rr.resample_ref(x, taps, L, M, lead)
    assert len(y) == rr.out_length(300, L, M) and shift + len(y) <= len(full)
    assert np.abs(full[shift:shift + len(y)] - y).max() <= 1e-13


def test_the_gain_oracle_is_audio_volume_gain():
    rng = np.random.default_rng(3)
    for n, amp in ((1, 0.5), (2049, 0.01), (5000, 3.0)):
        x = (amp * rng.standard_normal(n)).astype(np.float32)
        for inc in (True, False):
            got = audio.volume_gain(torch.from_numpy(x), target_dbfs=-30.0, increase_only=inc).numpy()[0]
            assert got in rr.float32_neighbours(rr.gain_ref(x, -30.0, inc)), (n, amp, inc)
    assert rr.gain_ref(np.zeros(5)) == np.inf and np.isnan(rr.gain_ref(np.zeros(0)))
    assert rr.gain_ref(np.full(10, 2.0)) == 1.0 and rr.gain_ref(np.full(10, 2.0), increase_only=False) < 0.02
