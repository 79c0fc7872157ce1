"""GPU: the silence-trimming stage (ge2e_vad_flags / ge2e_vad_mask / ge2e_vad_trim, functional.vad_flags / vad_mask /
trim_silences, MelFrontEnd(trim_silences=...), SpeakerEncoder.embed_audio(trim_silences=...)) against tests/vad_ref.py.
The C ABI is called with raw pointers on guarded buffers (tests/guarded.py): the waveforms between NaN guards with a NaN
sample behind every utterance and NaN in the samples past every utterance's last whole window, the outputs poisoned between
guards, the energies' workspace between byte guards.

Everything is integer arithmetic or a copy of bits, so everything is compared for equality."""
import os
import re

import numpy as np
import pytest
import torch

import encoder_ref as enc
import vad_ref as vr
from capi import GF, lib, ok  # noqa: F401
from guarded import SENTINEL, Buf, IntBuf, Workspace, _Guarded, dev, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "callers", "vad.npz")
NAN = np.float32(np.nan)


class ByteBuf(_Guarded):
    """uint8 between guards of 0xA5; outputs hold 0xA5 as poison (a flag is 0 or 1)."""
    FILL, DTYPE, is_fill = 0xA5, torch.uint8, staticmethod(lambda t: t == 0xA5)


def plan(lib, U, total, S, span=0, A=1, silence=0):
    from speaker_embedding_ge2e_loss_amd import _lib
    names = _lib._plan(lib.ge2e_vad_plan, U, total, S, span, A, silence)
    p = {}
    for n in names:
        m = re.fullmatch(r"(vad_\w+?)(?:<(\d+)>)?/(\d+)/(\d+)", n)
        p[m.group(1)] = (int(m.group(2) or 0), int(m.group(3)), int(m.group(4)))
    return p


class Batch:
    """Utterances in one guarded waveform buffer: one NaN sample behind each, NaN past each one's last whole window."""

    def __init__(self, utts, S, offset=1, gains=None):
        self.S, self.utts = S, [np.asarray(x, dtype=np.float32) for x in utts]
        parts, starts, at = [], [], 0
        for x in self.utts:
            y = x.copy()
            y[len(y) // S * S:] = NAN
            starts.append(at)
            parts += [y, np.array([NAN], np.float32)]
            at += len(y) + 1
        self.flat = np.concatenate(parts)
        self.starts, self.lens = starts, [len(x) for x in self.utts]
        self.windows = [n // S for n in self.lens]
        self.win_start = [0] + np.cumsum(self.windows).tolist()
        self.total, self.U = self.win_start[-1], len(utts)
        self.wav = Buf((len(self.flat),), self.flat, offset=offset)
        self.d_start = IntBuf((self.U,), starts, dtype=torch.int64)
        self.d_len = IntBuf((self.U,), self.lens, dtype=torch.int64)
        self.d_win = IntBuf((self.U + 1,), self.win_start, dtype=torch.int64)
        self.gains = None if gains is None else np.asarray(gains, dtype=np.float32)
        self.d_gain = None if gains is None else Buf((self.U,), self.gains)

    def gain(self, u):
        return np.float32(1.0) if self.gains is None else self.gains[u]

    def inputs_intact(self):
        return all(b.guards_intact() for b in (self.wav, self.d_start, self.d_len, self.d_win))

    def flags(self, lib, span, ratio, floor_energy):
        """ge2e_vad_flags -> (flags, energies), guards checked."""
        ws = Workspace(lib.ge2e_vad_workspace_bytes(self.total, self.U))
        out = ByteBuf((self.total + 1,))                         # one spare element: an address where there is no window
        ok(lib.ge2e_vad_flags(self.wav.ptr, self.d_start.ptr, self.d_len.ptr, None if self.d_gain is None else self.d_gain.ptr,
                              self.d_win.ptr, self.U, self.total, self.S, span, ratio, floor_energy, out.ptr, ws.ptr, None),
           "ge2e_vad_flags")
        flags = out._fetch("flags")
        assert flags[self.total] == 0xA5 and not (flags[:self.total] == 0xA5).any(), "flags: poison left, or one flag too many"
        flags = flags[:self.total]
        ws.check("ge2e_vad_flags")
        assert self.inputs_intact()
        return flags, ws.t.view(torch.int64).cpu().numpy()

    def ref_energies(self):
        return [vr.energies(x, self.S, self.gain(u)) for u, x in enumerate(self.utts)]

    def ref_flags(self, span, ratio, floor_energy):
        return [vr.flags_from_energies(e, span, ratio, floor_energy) for e in self.ref_energies()]

    def mask(self, lib, flags, A, silence):
        """ge2e_vad_mask on the given flags -> (dst, out_len)."""
        f = ByteBuf((self.total + 1,), np.append(flags, 1).astype(np.uint8))
        dst, out_len = IntBuf((self.total + 1,)), IntBuf((self.U,), dtype=torch.int64)
        ok(lib.ge2e_vad_mask(f.ptr, self.d_win.ptr, self.U, self.total, self.S, A, silence, dst.ptr, out_len.ptr, None),
           "ge2e_vad_mask")
        d, n = dst.get("dst", written=False), out_len.get("out_len")
        assert f.guards_intact() and self.inputs_intact()
        assert d[self.total] == SENTINEL and not (d[:self.total] == SENTINEL).any(), "dst: poison left, or one rank too many"
        return d[:self.total], n

    def ref_mask(self, flags, A, silence):
        dsts, lens, keeps = [], [], []
        for a, b in zip(self.win_start, self.win_start[1:]):
            keep = vr.mask(flags[a:b], A, silence)
            d, c = vr.ranks(keep)
            dsts.append(d), lens.append(c * self.S), keeps.append(keep)
        return np.concatenate(dsts) if dsts else np.zeros(0, np.int32), lens, keeps

    def trim(self, lib, dst, out_len, in_slot=False):
        """ge2e_vad_trim -> the uint32 bits of the output buffer (SENTINEL where nothing was written) and out_start."""
        if in_slot:
            out_start, size = list(self.starts), len(self.flat)
        else:
            out_start, size = [0] + np.cumsum(out_len).tolist()[:-1], int(np.sum(out_len))
        d_dst = IntBuf((self.total + 1,), np.append(dst, 0))
        d_out_start = IntBuf((self.U,), out_start, dtype=torch.int64)
        # float32 storage seen as bits: NaN payloads are data here; one spare element, so that an empty output has an address
        out = IntBuf((size + 1,))
        ok(lib.ge2e_vad_trim(self.wav.ptr, self.d_start.ptr, self.d_win.ptr, d_dst.ptr, d_out_start.ptr, self.U, self.total,
                             self.S, out.ptr, None), "ge2e_vad_trim")
        bits = out.get("trim", written=False)
        assert d_dst.guards_intact() and d_out_start.guards_intact() and self.inputs_intact()
        assert bits[size] == SENTINEL, "an element past the output was written"
        return bits[:size].view(np.uint32), out_start

    def ref_trim(self, keeps):
        return [vr.trim(x, self.S, k) for x, k in zip(self.utts, keeps)]


def signal(n, seed, S):
    """Noise whose level changes from window to window (silence, quiet, loud), so that the flags are mixed."""
    rng = np.random.default_rng(seed)
    level = np.repeat(rng.choice([0.0, 1e-4, 2e-3, 0.05, 0.4], n // S + 1), S)[:n]
    return (rng.standard_normal(n) * level + 0.01).astype(np.float32)


def window_counts(lib, S):
    """W_u of a batch: 0, 1, 2 and at, one below and one above every tile the plan names for this S."""
    p = plan(lib, 1, 1000, S)
    tiles = sorted({p["vad_energy"][1], p["vad_flag"][1], p["vad_trim"][1]})
    assert tiles in ([16, 256], [128, 256])
    return [0, 1, 2] + [t + d for t in tiles for d in (-1, 0, 1)]


SPECIALS = [np.inf, -np.inf, np.nan, 1.5, -1.5, 1.00002, -1.00004, 1e-45, -0.0, 3e38]


@pytest.mark.parametrize("with_gain", [False, True])
@pytest.mark.parametrize("S", [2, 30, 480, 481, 4096])
def test_energies_and_flags(lib, S, with_gain):
    counts = window_counts(lib, S)
    rng = np.random.default_rng(S + with_gain)
    gains = [np.float32(g) for g in rng.choice([0.5, 1.0, 1.7, 3.3], len(counts))] if with_gain else None
    utts = []
    for u, W in enumerate(counts):
        n = W * S + (u * 7 + 1) % S                          # a remainder behind the last window, odd offsets in the buffer
        x = signal(n, 100 * S + u, S)
        g = 1.0 if gains is None else gains[u]
        halves = vr.exact_halves(range(-6, 7), g)
        assert halves
        for j in rng.integers(0, max(W * S, 1), min(W * S, 24)):    # exact halves, saturating, NaN and inf samples
            x[j] = halves[j % len(halves)][0] if j % 2 else SPECIALS[j % len(SPECIALS)]
        utts.append(x)
    b = Batch(utts, S, offset=1, gains=gains)
    assert b.windows == counts and any(s % 2 for s in b.starts[1:])
    ratio, floor_energy = vr.ratio_q8(3.0), vr.min_energy(S, -50.0)
    flags, energies = b.flags(lib, 3, ratio, floor_energy)
    want_e = np.concatenate(b.ref_energies())
    assert energies.dtype == np.int64 and np.array_equal(energies, want_e)
    want = np.concatenate(b.ref_flags(3, ratio, floor_energy))
    assert np.array_equal(flags, want)
    assert 0 < want.sum() < len(want)


def test_the_floor_span_and_the_utterance_boundary(lib):
    S = 30
    rng = np.random.default_rng(5)
    steady = (0.2 * rng.standard_normal(40 * S)).astype(np.float32)              # loud all along: no window above its floor
    silent = (1e-4 * rng.standard_normal(40 * S)).astype(np.float32)
    mixed = signal(1500 * S + 11, 9, S)
    b = Batch([steady, silent, mixed, steady[:20 * S], silent[:S]], S)
    ratio, floor_energy = vr.ratio_q8(9.0), vr.min_energy(S, -60.0)
    for span in (0, 1, 50, 100, 1023, 1024):
        flags, _ = b.flags(lib, span, ratio, floor_energy)
        want = b.ref_flags(span, ratio, floor_energy)
        assert np.array_equal(flags, np.concatenate(want)), span
        # the loud utterances lie next to silent ones; a floor that looked across would flag all of their windows
        assert want[0].sum() == 0 and want[3].sum() == 0 and want[1].sum() == 0
        assert (span == 0) == (want[2].sum() == 0)


def test_comparisons_at_exact_equality(lib):
    """S = 2, windows (k, -k) / 32767: e = 4 k^2.  With the floor at k = 10, k = 30 gives e 256 == floor 2304."""
    ks = [10, 30, 31, 29, 10, 30, 12]
    x = np.array([v for k in ks for v in (k / 32767.0, -k / 32767.0)], dtype=np.float32)
    b = Batch([x], 2, offset=0)
    e = b.ref_energies()[0]
    assert e.tolist() == [4 * k * k for k in ks]
    for ratio, floor_energy, want in ((2304, 0, [0, 0, 1, 0, 0, 0, 0]), (2303, 0, [0, 1, 1, 0, 0, 1, 0]),
                                      (0, 3600, [0, 1, 1, 0, 0, 1, 0]), (0, 3601, [0, 0, 1, 0, 0, 0, 0]),
                                      (256, 0, [0, 1, 1, 1, 0, 1, 1]), (255, 400, [1] * 7), (0, 0, [1] * 7)):
        flags, energies = b.flags(lib, 100, ratio, floor_energy)
        assert energies.tolist() == e.tolist()
        assert flags.tolist() == want == vr.flags_from_energies(e, 100, ratio, floor_energy).tolist(), (ratio, floor_energy)
    zero = Batch([np.zeros(8, np.float32)], 2, offset=0)                        # e = 0: never above 0 times anything
    assert zero.flags(lib, 1, 0, 0)[0].tolist() == [0] * 4


def test_energies_near_2_to_54_and_the_largest_ratio(lib):
    """The 128-bit comparison: floor times ratio_q8 passes 2^64 (at ratio_q8 = 4096 its low 64 bits would compare wrongly)."""
    S = 4096
    alt = np.tile(np.array([1.0, -1.0], np.float32), S // 2)
    x = np.concatenate([2.0 * alt, 0.9 * alt, 2.0 * alt, 0.5 * alt, np.zeros(S, np.float32), 0.9 * alt])
    b = Batch([x, 0.9 * alt], S, offset=1)
    e = b.ref_energies()
    assert 2 ** 53 < e[0][0] < 2 ** 54 and e[0][4] == 0 and 2 ** 52 < e[0][1]
    seen = set()
    for span in (1, 2):
        for ratio in (300, 1024, 4096, 2 ** 11 * 3, 2 ** 40, 2 ** 62, 2 ** 63 - 1):
            flags, energies = b.flags(lib, span, ratio, 1)
            assert np.array_equal(energies, np.concatenate(e))
            want = np.concatenate(b.ref_flags(span, ratio, 1))
            assert np.array_equal(flags, want), (span, ratio)
            seen.add(tuple(want.tolist()))
            f0 = int(min(e[0][0], e[0][1]))
            if f0 * ratio >= 2 ** 64:
                assert want[0] == 0 and want[6] == 0
    assert len(seen) >= 3


AS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 64]
NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 64]


@pytest.mark.parametrize("di,density", list(enumerate([0.0, 0.1, 0.5, 0.9, 1.0])))
def test_the_mask_and_the_ranks(lib, di, density):
    S = 2
    chunk = plan(lib, 1, 1000, S)["vad_mask"][1]
    assert chunk == 4096
    counts = [0, 1, chunk - 1, 0, chunk, chunk + 1, 2 * chunk + 1, 0]
    b = Batch([np.zeros(W * S + 1, np.float32) for W in counts], S)
    rng = np.random.default_rng(di)
    # runs of flags: at density 0.5 single flags, pairs and longer runs all occur
    flags = np.repeat(rng.random(b.total) < density, rng.integers(1, 4, b.total))[:b.total].astype(np.uint8)
    for i, A in enumerate(AS):
        n = NS[(i + 2 * di) % len(NS)]
        dst, out_len = b.mask(lib, flags, A, n - 1)
        want_dst, want_len, keeps = b.ref_mask(flags, A, n - 1)
        assert out_len.tolist() == want_len, (A, n)
        assert dst.dtype == np.int32 and np.array_equal(dst, want_dst), (A, n)
        if density == 0.0:
            assert sum(want_len) == 0
        if density == 1.0 and A == 1:                          # (a wide average drops a short utterance even so)
            assert want_len == [W * S for W in counts]
    # any non-zero byte is a voiced window
    dst, out_len = b.mask(lib, flags * 37, 8, 6)
    assert np.array_equal(dst, b.ref_mask(flags, 8, 6)[0])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("S", [2, 30, 64, 480, 481])
def test_trim_moves_the_bits_of_the_kept_windows(lib, S, offset):
    p = plan(lib, 1, 1000, S)["vad_trim"]
    assert p[:2] == ((64, 16) if S >= 64 else (8, 128))
    rng = np.random.default_rng(S + offset)
    counts = [p[1] + 1, 0, 3, p[1] - 1, 1]
    utts = []
    for u, W in enumerate(counts):
        n = W * S + (3 * u + 2) % S
        bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)   # any bits: -0.0, denormals, NaN payloads
        bits[bits == np.uint32(SENTINEL & 0xFFFFFFFF)] = 0
        bits[:min(n, 3)] = [0x80000000, 0x7FC12345, 0xFFFFFFFF][:min(n, 3)]
        utts.append(bits.view(np.float32))
    b = Batch(utts, S, offset=offset)
    poison = np.uint32(SENTINEL & 0xFFFFFFFF)
    for density in (0.5, 1.0, 0.0):
        flags = (rng.random(b.total) < density).astype(np.uint8)
        dst, out_len, keeps = b.ref_mask(flags, 1, 0)
        want = [w.view(np.uint32) for w in b.ref_trim(keeps)]
        assert [len(w) for w in want] == out_len
        got, _ = b.trim(lib, dst, out_len)                                      # dense: exactly sum(out_len) elements
        assert np.array_equal(got, np.concatenate(want)), density
        got, out_start = b.trim(lib, dst, out_len, in_slot=True)                # in-slot: every utterance at its own start
        expect = np.full(len(b.flat), poison, dtype=np.uint32)
        for s, w in zip(out_start, want):
            expect[s:s + len(w)] = w
        assert np.array_equal(got, expect), density
        assert int((got != poison).sum()) == sum(out_len)
    assert sum(b.ref_mask(np.ones(b.total, np.uint8), 1, 0)[1]) == b.total * S


def pipeline(lib, b, span=3, A=3, silence=2):
    ratio, floor_energy = vr.ratio_q8(3.0), vr.min_energy(b.S, -50.0)
    flags, energies = b.flags(lib, span, ratio, floor_energy)
    dst, out_len = b.mask(lib, flags, A, silence)
    bits, _ = b.trim(lib, dst, out_len.tolist())
    return flags, energies, dst, out_len, bits


def test_determinism_and_independence_of_the_batch(lib):
    S = 30
    utts = [signal(n, 40 + i, S) for i, n in enumerate((300 * S + 7, 5, 17 * S, 4200 * S + 29, S))]
    b = Batch(utts, S)
    first = pipeline(lib, b)
    again = pipeline(lib, b)
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    want_flags = b.ref_flags(3, vr.ratio_q8(3.0), vr.min_energy(S, -50.0))
    assert np.array_equal(first[0], np.concatenate(want_flags)) and 0 < first[0].sum() < b.total
    at = 0
    for u, x in enumerate(utts):                                               # every utterance alone: the same results
        alone = pipeline(lib, Batch([x], S, offset=u % 2))
        a, e = b.win_start[u], b.win_start[u + 1]
        assert np.array_equal(alone[0], first[0][a:e]) and np.array_equal(alone[1], first[1][a:e])
        assert np.array_equal(alone[2], first[2][a:e]) and alone[3][0] == first[3][u]
        assert np.array_equal(alone[4], first[4][at:at + int(first[3][u])])
        at += int(first[3][u])
    assert at == len(first[4])


@pytest.mark.parametrize("S,lens,gains", [(480, [1000, 0, 479, 480, 961], [1.0, 2.0, 0.5, 0.25, 1.5]),
                                          (30, [0, 4000, 0, 95, 0], None)])
def test_empty_utterances_first_in_runs_and_near_the_end(lib, S, lens, gains):
    """Utterances without a window share their win_start with the next one: first, in a run, between two others and last.
    A window must find the LAST utterance that starts at or before it.  Every stage equals vad_ref to the bit, utterance by
    utterance, and equals the same calls on each non-empty utterance alone; the mask and the trim run twice, on the
    detector's flags and with every window voiced (width 1, no dilation), so that the trim looks up every window."""
    utts = [signal(n, 90 + i, S) for i, n in enumerate(lens)]
    span, ratio, floor_energy = 3, vr.ratio_q8(3.0), vr.min_energy(S, -50.0)

    def stages(b):
        flags, energies = b.flags(lib, span, ratio, floor_energy)
        out = [flags, energies[:b.total]]
        for f, A, silence in ((flags, 3, 2), (np.ones(b.total, np.uint8), 1, 0)):
            dst, out_len = b.mask(lib, f, A, silence)
            out += [dst, out_len, b.trim(lib, dst, out_len.tolist())[0]]
        return out

    b = Batch(utts, S, gains=gains)
    got = stages(b)
    want_flags = np.concatenate(b.ref_flags(span, ratio, floor_energy))
    assert np.array_equal(got[0], want_flags) and np.array_equal(got[1], np.concatenate(b.ref_energies()))
    for k, f, A, silence in ((2, want_flags, 3, 2), (5, np.ones(b.total, np.uint8), 1, 0)):
        dst, kept, keeps = b.ref_mask(f, A, silence)
        assert np.array_equal(got[k], dst) and got[k + 1].tolist() == kept
        assert np.array_equal(got[k + 2], np.concatenate(b.ref_trim(keeps)).view(np.uint32))
    assert got[6].tolist() == [w * S for w in b.windows] and b.total > 0
    at = {4: 0, 7: 0}
    for u, x in enumerate(utts):
        if len(x) == 0:
            continue
        alone = stages(Batch([x], S, offset=u % 2, gains=None if gains is None else [gains[u]]))
        a, e = b.win_start[u], b.win_start[u + 1]
        for k in (0, 1, 2, 5):
            assert np.array_equal(alone[k], got[k][a:e]), (u, k)
        for k in (4, 7):
            n = int(got[k - 1][u])
            assert alone[k - 1][0] == n and np.array_equal(alone[k], got[k][at[k]:at[k] + n]), (u, k)
            at[k] += n
    assert at == {4: len(got[4]), 7: len(got[7])}


# ---- functional and the pipeline ---------------------------------------------------------------------------------------------
def host_trim(wavs, S, gains=None, A=8, silence=6, **detector):
    return [vr.trim_silences(w, S, 1.0 if gains is None else gains[u], A, silence, **detector)[0] for u, w in enumerate(wavs)]


def test_functional_trim_silences_native_torch_and_oracle(GF):
    S = 30
    wavs = [signal(n, 70 + i, S) for i, n in enumerate((200 * S + 3, 0, 29, 31 * S, 4100 * S + 1))]
    lengths = [len(w) for w in wavs]
    flat = torch.as_tensor(np.concatenate(wavs)).to(dev())
    gain = torch.tensor([1.0, 2.0, 1.0, 0.25, 1.5], device=dev())
    for g in (None, gain):
        gains = None if g is None else g.cpu().numpy()
        kw = dict(window=S, floor_span=5, ratio_db=3.0, min_level_dbfs=-50.0, avg_width=3, max_silence=2)
        want = host_trim(wavs, S, gains, 3, 2, span=5, ratio=vr.ratio_q8(3.0), floor_energy=vr.min_energy(S, -50.0))
        lay = GF.vad_layout(lengths, S, device=dev())
        flags = {}
        for native in (True, False, None):
            out, out_lengths = GF.trim_silences(flat, lengths, gain=g, native=native, **kw)
            assert out_lengths == [len(w) for w in want] and isinstance(out_lengths, list)
            assert same_bits(out.cpu().numpy(), np.concatenate(want))
            flags[native] = GF.vad_flags(flat, lengths, g, window=S, floor_span=5, ratio_db=3.0, min_level_dbfs=-50.0,
                                         layout=lay, native=native)
            dst, out_len = GF.vad_mask(flags[native], lay, 3, 2, native=native)
            assert out_len.tolist() == out_lengths and dst.dtype == torch.int32 and out_len.dtype == torch.int64
        assert torch.equal(flags[True], flags[False]) and 0 < int(flags[True].sum()) < lay.total_windows
        assert 0 < sum(len(w) for w in want) < sum(lengths)
    # parameters the kernels do not take: the torch route where native is None, an error where it is True
    out, out_lengths = GF.trim_silences(flat, lengths, window=S, floor_span=1100, avg_width=65, max_silence=70)
    want = host_trim(wavs, S, None, 65, 70, span=1100)
    assert out_lengths == [len(w) for w in want] and same_bits(out.cpu().numpy(), np.concatenate(want))
    with pytest.raises(RuntimeError):
        GF.trim_silences(flat, lengths, window=S, floor_span=1100, native=True)
    # nothing to trim: no window in any utterance
    out, out_lengths = GF.trim_silences(flat[:40], [20, 20], window=S)
    assert out.numel() == 0 and out_lengths == [0, 0]
    # the one change-over by size: the mask of a very long utterance comes from torch's ops where native is None; same ranks
    lay = GF.vad_layout([2 * (GF.VAD_MASK_TORCH_FROM + 1), 10], 2, device=dev())
    f = (torch.rand(lay.total_windows, device=dev()) < 0.5).to(torch.uint8)
    auto, kernel = GF.vad_mask(f, lay, 3, 2), GF.vad_mask(f, lay, 3, 2, native=True)
    assert torch.equal(auto[0], kernel[0]) and torch.equal(auto[1], kernel[1]) and int(kernel[1].sum()) > 0


def test_voice_flags_from_the_reference_give_its_trimmed_waveform(GF):
    g = np.load(GOLDEN)
    for name in ("v0", "v1", "v2", "v3", "v4"):
        sr, ms, A, silence = (int(v) for v in g[name + "_cfg"])
        wav = torch.as_tensor(g[name + "_wav"]).to(dev())
        for native in (True, False):
            out, out_lengths = GF.trim_silences(wav, voice_flags=g[name + "_flags"], window=ms * sr // 1000, avg_width=A,
                                                max_silence=silence, native=native)
            assert out_lengths == [len(g[name + "_trimmed"])] and same_bits(out.cpu().numpy(), g[name + "_trimmed"]), name
    # three of them in one call, under other widths
    names = ("v0", "v3", "v4")
    flat = torch.as_tensor(np.concatenate([g[n + "_wav"] for n in names])).to(dev())
    out, out_lengths = GF.trim_silences(flat, [len(g[n + "_wav"]) for n in names], window=30, avg_width=1, max_silence=1,
                                        voice_flags=np.concatenate([g[n + "_flags"] for n in names]))
    want = [vr.trim_silences(g[n + "_wav"], 30, A=1, max_silence=1, voice_flags=g[n + "_flags"])[0] for n in names]
    assert out_lengths == [len(w) for w in want] and same_bits(out.cpu().numpy(), np.concatenate(want))
    assert same_bits(want[1], g["v3_trimmed"])
    with pytest.raises(ValueError):
        GF.trim_silences(flat, [len(g[n + "_wav"]) for n in names], window=30, voice_flags=g["v0_flags"])


def front_end():
    from speaker_embedding_ge2e_loss_amd.audio import MelFrontEnd
    return MelFrontEnd(16000, 512, 160, 40, 90.0, 7600.0, 10, 20, 10.0, 0.75, vad_floor_span=20)


def recordings():
    out = []
    for seed, seconds in ((0, 1.6), (1, 0.9), (2, 2.2)):
        x, _ = vr.bursts(seed, 30, seconds=8.0)
        out.append(np.ascontiguousarray(np.float32(0.05) * x[int(0.5 * 16000):int((0.5 + seconds) * 16000)]))   # quiet: a gain above 1
    return out


def test_frames_after_trimming_are_the_frames_of_the_trimmed_waveforms(GF):
    from speaker_embedding_ge2e_loss_amd import audio
    fe, host = front_end(), recordings()
    wavs = [torch.as_tensor(w).to(dev()) for w in host]
    before = fe.frames(wavs, normalize_volume=True, pad_to_partials=True)
    for norm in (False, True):
        gain = audio.volume_gain(torch.cat(wavs), [w.numel() for w in wavs], fe.target_dbfs) if norm else None
        trimmed = host_trim(host, 480, None if gain is None else gain.cpu().numpy(), span=20)
        assert all(0 < len(t) < len(w) for t, w in zip(trimmed, host))
        flat, lengths, g = fe.preprocess(wavs, norm, trim_silences=True)
        assert lengths == [len(t) for t in trimmed] and same_bits(flat.cpu().numpy(), np.concatenate(trimmed))
        assert (g is None) == (gain is None) and (g is None or torch.equal(g, gain))
        for pad in (False, True):
            got, fs = fe.frames(wavs, norm, pad_to_partials=pad, trim_silences=True)
            want, fs2 = fe.spectrogram(torch.as_tensor(np.concatenate(trimmed)).to(dev()), lengths, gain, pad_to_partials=pad)
            assert fs == fs2 and torch.equal(got, want)
        parts = fe.partials(wavs, norm, trim_silences=True)
        rows, owner = fe.partial_rows(lengths, fs)
        assert [p.shape[0] for p in parts] == [owner.count(u) for u in range(3)] and all(p.shape[0] >= 1 for p in parts)
        assert torch.equal(parts[1][0], got[rows[owner.index(1)]:rows[owner.index(1)] + 20])
    # voice_flags alone imply the trimming; without either nothing changes by a bit
    n_windows = sum(len(w) // 480 for w in host)
    every = np.ones(n_windows, np.uint8)
    got, fs = fe.frames(wavs, voice_flags=every, pad_to_partials=True)
    want, fs2 = fe.frames([w[:w.numel() // 480 * 480] for w in wavs], pad_to_partials=True)
    assert fs == fs2 and torch.equal(got, want)
    after = fe.frames(wavs, normalize_volume=True, pad_to_partials=True, trim_silences=False)
    assert before[1] == after[1] and torch.equal(before[0], after[0])


def module_with(ps, n_mels, H, L, D):
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    m = SpeakerEncoder(n_mels, H, L, D)
    with torch.no_grad():
        for l in range(L):
            for n, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ps[4 * l:4 * l + 4]):
                getattr(m.LSTM_stack, f"{n}_l{l}").copy_(torch.as_tensor(p))
        m.projection.weight.copy_(torch.as_tensor(ps[-2]))
        m.projection.bias.copy_(torch.as_tensor(ps[-1]))
    return m.to(dev()).eval()


def test_embed_audio_after_trimming_and_an_utterance_of_silence(GF):
    n_mels, H, L, D = 40, 128, 2, 64
    fe, host = front_end(), recordings()
    host.append(np.zeros(4000, np.float32))                                   # digital silence: trimmed to nothing
    wavs = [torch.as_tensor(w).to(dev()) for w in host]
    m = module_with(enc.random_params(n_mels, H, L, D, seed=22), n_mels, H, L, D)
    trimmed = host_trim(host, 480, span=20)
    assert len(trimmed[3]) == 0 and all(len(t) for t in trimmed[:3])
    got = m.embed_audio(wavs, fe, trim_silences=True)
    want = m.embed_audio([torch.as_tensor(t).to(dev()) for t in trimmed], fe)
    assert got.shape == (4, D) and bool(torch.isfinite(got).all()) and same_bits(got.cpu().numpy(), want.cpu().numpy())
    assert not same_bits(got.cpu().numpy(), m.embed_audio(wavs, fe).cpu().numpy())
    # the silent utterance alone: one partial of silence with pad_to_partials, a ValueError naming it without
    parts = fe.partials(wavs[3], trim_silences=True)
    assert parts[0].shape == (1, 20, n_mels) and torch.equal(parts[0], fe.partials(torch.zeros(0, device=dev()))[0])
    frames, fs = fe.frames(wavs, pad_to_partials=True, trim_silences=True)
    assert fs[4] - fs[3] == fe.slices(0).padded_length // 160 + 1
    with pytest.raises(ValueError, match="utterance 3"):
        fe.frames(wavs, trim_silences=True)
