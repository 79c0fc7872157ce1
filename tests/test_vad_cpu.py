"""CPU: the host side of the silence-trimming stage -- ge2e_vad_workspace_bytes / ge2e_vad_flags / ge2e_vad_mask /
ge2e_vad_trim / ge2e_vad_plan: declared, exported and bound, every error code and the order of the checks, the workspace
size, the plan -- and tests/vad_ref.py, the oracle of the GPU tests: its mask against scipy's binary_dilation and a
restatement of the reference's moving_average, its trimming against what the reference itself returned
(tests/golden/callers/vad.npz), its detector on synthetic bursts, its quantiser at the edges."""
import ctypes
import os
import re

import numpy as np
import pytest

import vad_ref as vr
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, audio, build

SYMS = ("ge2e_vad_workspace_bytes", "ge2e_vad_flags", "ge2e_vad_mask", "ge2e_vad_trim", "ge2e_vad_plan")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_IMPL, ERR_ALIGN = -1, -2, -3, -5, -6
I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "callers", "vad.npz")


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_vad_workspace_bytes"] == (ctypes.c_size_t, [LL, I])
    assert _lib.PROTOTYPES["ge2e_vad_flags"] == (I, [P] * 5 + [I, LL, I, I, LL, LL, P, P, P])
    assert _lib.PROTOTYPES["ge2e_vad_mask"] == (I, [P, P, I, LL, I, I, I, P, P, P])
    assert _lib.PROTOTYPES["ge2e_vad_trim"] == (I, [P] * 5 + [I, LL, I, P, P])
    assert _lib.PROTOTYPES["ge2e_vad_plan"] == (I, [I, LL, I, I, I, I, ctypes.c_char_p, ctypes.c_size_t])
    assert not any(a.startswith("vad") for a in _lib.plan_atoms())
    from speaker_embedding_ge2e_loss_amd import functional as GF
    for f in ("vad_supported", "vad_layout", "vad_flags", "vad_mask", "trim_silences"):
        assert callable(getattr(GF, f))
    for f in ("preprocess", "spectrogram"):
        assert callable(getattr(audio.MelFrontEnd, f))


def test_workspace_is_the_int64_energies(lib):
    w = lib.ge2e_vad_workspace_bytes
    assert w(0, 1) == 0 and w(1, 1) == 8 and w(120000, 360) == 960000 and w(2 ** 31 - 1, 1) == 8 * (2 ** 31 - 1)
    assert w(-1, 1) == 0 and w(10, 0) == 0 and w(10, -2) == 0


def test_flags_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_vad_flags
    ok = dict(wav=36, utt_start=64, utt_len=72, gain=100, win_start=80, U=2, total=40, S=480, span=100, ratio=2033,
              min_energy=1000, flags=33, ws=256, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("wav", "utt_start", "utt_len", "win_start", "flags"):
        assert call(**{k: None}) == ERR_NULL, k
    for kw in (dict(U=0), dict(U=-1), dict(S=0), dict(S=-480), dict(total=-1), dict(span=-1), dict(ratio=-1), dict(min_energy=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(S=1), dict(S=4097), dict(S=2 ** 31 - 1), dict(span=1025), dict(total=2 ** 31), dict(total=2 ** 62)):
        assert call(**kw) == ERR_IMPL, kw
    for kw in (dict(ws=None), dict(ws=264), dict(ws=260)):
        assert call(**kw) == ERR_WORKSPACE, kw
    for kw in (dict(wav=38), dict(wav=33), dict(gain=101)):
        assert call(**kw) == ERR_ALIGN, kw
    # the order: NULL, shape, implementation, workspace, alignment
    assert call(wav=None, U=0) == ERR_NULL and call(flags=None, S=1, ws=None) == ERR_NULL
    assert call(U=0, S=4097) == ERR_SHAPE and call(span=-1, S=1) == ERR_SHAPE and call(total=-1, ws=None, wav=38) == ERR_SHAPE
    assert call(S=1, ws=None) == ERR_IMPL and call(span=1025, wav=38) == ERR_IMPL
    assert call(ws=None, wav=38) == ERR_WORKSPACE and call(ws=264, gain=101) == ERR_WORKSPACE
    # supported at the limits, gain optional, and nothing to launch: OK without a GPU
    assert call(total=0) == 0 and call(total=0, gain=None, S=2, span=0, ratio=0, min_energy=0) == 0
    assert call(total=0, S=4096, span=1024, ratio=2 ** 63 - 1, min_energy=2 ** 62) == 0


def test_mask_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_vad_mask
    ok = dict(flags=33, win_start=80, U=2, total=40, S=480, A=8, silence=6, dst=100, out_len=256, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("flags", "win_start", "dst", "out_len"):
        assert call(**{k: None}) == ERR_NULL, k
    for kw in (dict(U=0), dict(S=0), dict(total=-1), dict(A=0), dict(A=-8), dict(silence=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(S=1), dict(S=4097), dict(A=65), dict(silence=64), dict(total=2 ** 31)):
        assert call(**kw) == ERR_IMPL, kw
    for kw in (dict(dst=102), dict(dst=101), dict(out_len=260), dict(out_len=257)):
        assert call(**kw) == ERR_ALIGN, kw
    assert call(dst=None, U=0) == ERR_NULL and call(A=0, S=4097) == ERR_SHAPE and call(U=0, A=65, dst=102) == ERR_SHAPE
    assert call(A=65, dst=102) == ERR_IMPL and call(silence=64, out_len=260) == ERR_IMPL


def test_trim_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_vad_trim
    ok = dict(wav=36, utt_start=64, win_start=80, dst=100, out_start=128, U=2, total=40, S=480, out=260, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("wav", "utt_start", "win_start", "dst", "out_start", "out"):
        assert call(**{k: None}) == ERR_NULL, k
    for kw in (dict(U=0), dict(S=0), dict(S=-1), dict(total=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(S=1), dict(S=4097), dict(total=2 ** 31)):
        assert call(**kw) == ERR_IMPL, kw
    for kw in (dict(wav=38), dict(out=261), dict(out=262), dict(dst=101)):
        assert call(**kw) == ERR_ALIGN, kw
    assert call(out=None, U=0) == ERR_NULL and call(U=0, S=4097, out=261) == ERR_SHAPE and call(S=1, out=261) == ERR_IMPL
    assert call(total=0) == 0 and call(total=0, S=2) == 0 and call(total=0, S=4096) == 0


def test_plan_names_the_instantiations_the_chunk_and_the_grids(lib):
    plan = lambda *a: _lib._plan(lib.ge2e_vad_plan, *a)  # noqa: E731
    assert plan(360, 120000, 480, 100, 8, 6) == ["vad_energy<64>/16/7500", "vad_flag/256/469", "vad_mask/4096/360",
                                                 "vad_trim<64>/16/7500"]
    assert plan(3, 1000, 30, 0, 1, 0) == ["vad_energy<8>/128/8", "vad_flag/256/4", "vad_mask/4096/3", "vad_trim<8>/128/8"]
    assert plan(1, 1, 64, 1024, 64, 63)[0] == "vad_energy<64>/16/1" and plan(1, 1, 63, 0, 1, 0)[0] == "vad_energy<8>/128/1"
    assert plan(1, 2 ** 31 - 1, 2, 0, 1, 0)[2:] == ["vad_mask/4096/1", "vad_trim<8>/128/%d" % 2 ** 24]
    assert plan(5, 0, 480, 100, 8, 6) == []
    f = lib.ge2e_vad_plan
    assert f(1, 1000, 30, 0, 1, 0, None, 0) == len("vad_energy<8>/128/8,vad_flag/256/4,vad_mask/4096/1,vad_trim<8>/128/8")
    for bad in ((0, 10, 480, 100, 8, 6), (1, -1, 480, 100, 8, 6), (1, 10, 0, 100, 8, 6), (1, 10, 480, -1, 8, 6),
                (1, 10, 480, 100, 0, 6), (1, 10, 480, 100, 8, -1), (1, 10, 4097, 100, 0, 6)):
        assert f(*bad, None, 0) == ERR_SHAPE, bad
    for bad in ((1, 10, 1, 100, 8, 6), (1, 10, 4097, 100, 8, 6), (1, 10, 480, 1025, 8, 6), (1, 10, 480, 100, 65, 6),
                (1, 10, 480, 100, 8, 64), (1, 2 ** 31, 480, 100, 8, 6)):
        assert f(*bad, None, 0) == ERR_IMPL, bad
    with pytest.raises(ValueError):
        plan(1, 10, 1, 100, 8, 6)


def test_layout_and_detector_parameters():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    lay = GF.vad_layout([1000, 0, 479, 480, 961], 480, device="cpu")
    assert lay.win_start == [0, 2, 2, 2, 3, 5] and lay.win_start_dev.tolist() == lay.win_start and lay.total_windows == 5
    assert lay.utt_start.tolist() == [0, 1000, 1000, 1479, 1959] and lay.utt_len.tolist() == [1000, 0, 479, 480, 961]
    assert lay.window == 480
    for bad in (dict(lengths=[], window=480), dict(lengths=[-1], window=480), dict(lengths=[5], window=0)):
        with pytest.raises(ValueError):
            GF.vad_layout(device="cpu", **bad)
    assert GF.vad_detector_params(480, 9.0, -60.0) == (vr.ratio_q8(9.0), vr.min_energy(480, -60.0)) == (2033, 247375017)      # 480^2 32.767^2
    assert GF.vad_supported(480, 100, 8, 6) and GF.vad_supported(2, 0, 1, 0) and GF.vad_supported(4096, 1024, 64, 63)
    for bad in ((1, 0, 1, 0), (4097, 0, 1, 0), (480, 1025, 1, 0), (480, 0, 65, 0), (480, 0, 1, 64)):
        assert not GF.vad_supported(*bad), bad
    fe = audio.MelFrontEnd()
    assert (fe.vad_window, fe.vad_moving_average_width, fe.vad_max_silence_length) == (480, 8, 6)
    assert (fe.vad_floor_span, fe.vad_ratio_db, fe.vad_min_level_dbfs) == (100, 9.0, -60.0)
    from types import SimpleNamespace as NS
    a = NS(sampling_rate=8000, n_fft=512, hop_length=128, mel_n_channels=40, mel_window_step=10, partials_n_frames=20)
    fe = audio.MelFrontEnd.from_hp(NS(audio=a, vad=NS(rate_partial_slices=1.3, min_coverage=0.75, vad_window_length=20,
                                                      vad_moving_average_width=5, vad_max_silence_length=3)))
    assert (fe.vad_window, fe.vad_moving_average_width, fe.vad_max_silence_length, fe.vad_floor_span) == (160, 5, 3, 100)
    fe = audio.MelFrontEnd.from_hp(NS(audio=a, vad=NS(rate_partial_slices=1.3, min_coverage=0.75)))
    assert (fe.vad_window_length, fe.vad_moving_average_width, fe.vad_max_silence_length) == (30, 8, 6)


def reference_moving_average_mask(flags, width):
    """The reference's moving_average and rounding (s0:135-142), restated."""
    padded = np.concatenate((np.zeros((width - 1) // 2), flags, np.zeros(width // 2)))
    ret = np.cumsum(padded, dtype=float)
    ret[width:] = ret[width:] - ret[:-width]
    return np.round(ret[width - 1:] / width).astype(bool)


@pytest.mark.parametrize("density", [0.0, 0.1, 0.5, 0.9, 1.0])
def test_the_oracle_mask_is_moving_average_and_binary_dilation(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 10))
    for A in list(range(1, 12)) + [64]:
        for silence in list(range(0, 9)) + [63]:
            W = int(rng.integers(1, 90))
            flags = (rng.random(W) < density).astype(np.uint8)
            want = ndimage.binary_dilation(reference_moving_average_mask(flags, A), np.ones(silence + 1))
            got = vr.mask(flags, A, silence)
            assert got.dtype == bool and np.array_equal(got, want), (A, silence, flags.tolist())
    assert vr.mask(np.zeros(0, np.uint8), 8, 6).shape == (0,)


def test_the_oracle_trims_as_the_reference_did():
    g = np.load(GOLDEN)
    names = sorted(k[:-4] for k in g.files if k.endswith("_wav"))
    assert names == ["v0", "v1", "v2", "v3", "v4"]
    kept = []
    for name in names:
        sr, ms, A, silence = (int(v) for v in g[name + "_cfg"])
        S = ms * sr // 1000
        wav, flags, want = g[name + "_wav"], g[name + "_flags"], g[name + "_trimmed"]
        assert S == 30 and len(flags) == len(wav) // S and (len(wav) % S > 0) == (name != "v3")
        got, _, keep = vr.trim_silences(wav, S, A=A, max_silence=silence, voice_flags=flags)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        dst, count = vr.ranks(keep)
        assert count * S == len(want) and np.array_equal(dst[keep], np.arange(count)) and (dst[~keep] == -1).all()
        kept.append(len(want))
    assert kept[4] == 0 and all(0 < k < len(g[n + "_wav"]) for k, n in zip(kept[:4], names))


SEEDS = (0, 1, 2, 3, 4)


def clear_windows(spans, n_windows, S):
    """Per window: 1 wholly inside a burst, 0 wholly outside every burst, -1 across an edge."""
    label = np.zeros(n_windows, dtype=np.int64)
    for w in range(n_windows):
        a, b = w * S, (w + 1) * S
        for s0, s1 in spans:
            if a >= s0 and b <= s1:
                label[w] = 1
            elif a < s1 and b > s0:
                label[w] = -1
    return label


@pytest.mark.parametrize("snr_db", [30, 20])
def test_the_detector_is_right_on_the_synthetic_bursts(snr_db):
    """vad_ref.bursts(seed, snr): eight seconds at 16 kHz, three bursts of a 19-harmonic tone (120 Hz, vibrato, a 4 Hz
    envelope) over white noise, seeds 0 .. 4; the defaults S = 480, span 100, 9 dB, -60 dBFS.  Every window that lies wholly
    inside or wholly outside a burst must get the right flag."""
    checked = 0
    for seed in SEEDS:
        x, spans = vr.bursts(seed, snr_db)
        flags = vr.flags(x, 480)
        label = clear_windows(spans, len(flags), 480)
        clear = label >= 0
        wrong = np.flatnonzero(clear & (flags != label))
        assert wrong.size == 0, (seed, snr_db, wrong.tolist())
        checked += int(clear.sum())
        # and the trimming built on it shortens the recording but keeps every burst whole
        _, _, keep = vr.trim_silences(x, 480)
        assert keep[label == 1].all() and 0 < keep.sum() < len(keep)
    assert checked >= 1300


def test_the_quantiser_at_its_edges():
    f32 = np.float32
    exact = vr.exact_halves(list(range(-40, 40)) + [1000, 1001, -1000, -1001, 32766, 32767, -32768, -32769])
    assert len(exact) >= 20 and {k % 2 for _, k in exact} == {0, 1}
    for x, k in exact:                                                        # the scaled value is exactly k + 1/2
        want = k if k % 2 == 0 else k + 1                                     # halves go to the even neighbour
        assert vr.quantise([x])[0] == min(max(want, -32768), 32767), (x, k)
    for x, k in vr.exact_halves(range(-20, 20), gain=1.7):
        assert vr.quantise([x], np.float32(1.7))[0] == (k if k % 2 == 0 else k + 1)
    x = np.array([1.0, -1.0, 1.00002, -1.00002, -1.00004, 3.0, -3.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0,
                  1e-45, -1e-45, 1e-39, 1.5e-5, 1.6e-5, 4.6e-5], dtype=np.float32)
    want = [32767, -32767, 32767, -32768, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0, 0, 0, 0, 0, 0, 1, 2]
    assert vr.quantise(x).tolist() == want
    assert vr.quantise(x, gain=np.float32(np.inf)).tolist()[:2] == [32767, -32768] and vr.quantise([0.0], gain=np.inf)[0] == 0
    # two roundings: a gain whose product with x rounds before the scale is applied
    x, g = f32(0.1), f32(3.3)
    assert vr.quantise([x], g)[0] == int(np.rint(f32(f32(x * g) * f32(32767.0))))
    # energies: DC does not count, the remainder is not looked at, the bound of the header holds
    assert vr.energies(np.full(100, 0.25, np.float32), 30).tolist() == [0, 0, 0]
    alt = np.tile(np.array([2.0, -2.0], np.float32), 2048)
    assert vr.energies(alt, 4096).tolist() == [4096 * 2048 * (32767 ** 2 + 32768 ** 2) - 2048 ** 2]
    assert 2 ** 53 < vr.energies(alt, 4096)[0] < 2 ** 54
    assert vr.energies(np.array([1, -1, np.nan], np.float32), 2).tolist() == [2 * 2 * 32767 ** 2]
