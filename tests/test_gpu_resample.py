"""GPU: the resampling stage (ge2e_resample_pack / ge2e_resample / ge2e_volume_gain, functional.resample,
functional.volume_gain, MelFrontEnd(source_rate=...), SpeakerEncoder.embed_audio(source_rate=...)) against
tests/resample_ref.py in float64.  The C ABI is called with raw pointers on guarded buffers (tests/guarded.py): the
waveforms between NaN guards with NaN written into the samples behind every utterance, the outputs NaN-poisoned between
guards, the gain's workspace between byte guards.

The accuracy bound is derived, not measured: the oracle runs on the float32-rounded taps and samples, and an output may
differ from it by at most (W + 1) 2^-24 sum_k |taps x| -- the bound of a W-term fp32 dot product with fused products,
accumulated in ANY order.  Single taps are held to float32 equality (a unit impulse picks them out one by one).
The gain: the arithmetic is double on both sides, so only the final rounding can differ; the result must be the float32
rounding of the oracle's or one of its two neighbours.

Measured on an MI355X, the worst output as a fraction of its bound: (1, 1) 0.310, (1, 3) 0.181, (2, 1) 0.310, (2, 3) 0.279,
(3, 2) 0.307, (160, 441) 0.176, (640, 441) 0.398 with two zero crossings (W 5 .. 13); 44 100 -> 16 000 on 2 000 samples:
kaiser_best (W 355) 0.025, kaiser_fast (W 91) 0.054.  The other instantiations, synthetic banks: resample<lds,4> at (1, 6),
W 769: 0.003; resample<lds,1> at (1, 32), W 13: 0.114; resample<global,4> at (1, 64), W 13: 0.186.
"""
import functools

import numpy as np
import pytest
import torch

import encoder_ref as enc
import resample_ref as rr
from capi import GF, lib, ok  # noqa: F401
from guarded import Buf, Workspace, dev, same_bits

pytestmark = pytest.mark.gpu
GAP = 5                          # NaN samples behind every utterance in the wav buffer
SMALL = (2, 0.9475937167399596, 14.769656459379492)      # two zero crossings: a narrow bank
RATIOS = [(1, 1), (1, 3), (2, 1), (2, 3), (3, 2), (160, 441), (640, 441)]


def noise(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def bank32(L, M, flt=SMALL):
    """(lead, taps) of the project's bank for M -> L, rounded once to float32 as resample_pack holds it."""
    from speaker_embedding_ge2e_loss_amd import audio
    b = audio.resample_bank(M, L, flt)
    assert (b.up, b.down) == (L, M)
    taps = b.taps.numpy().astype(np.float32)
    taps.setflags(write=False)
    return b.lead, taps


_TABLES = {}


def tables(taps, L, M, lead):
    """functional.resample_pack, once per distinct bank."""
    from speaker_embedding_ge2e_loss_amd import functional
    key = (L, M, lead, taps.tobytes())
    if key not in _TABLES:
        _TABLES[key] = functional.resample_pack(torch.tensor(taps).to(dev()), L, M, lead)
    return _TABLES[key]


def tile_of(L, M, lead):
    from speaker_embedding_ge2e_loss_amd import _lib
    return int(_lib.resample_plan(1, 1, L, M, lead)[0].split("/")[1])


def out_starts(lens, L, M):
    os = [0]
    for n in lens:
        os.append(os[-1] + rr.out_length(n, L, M))
    return os


def res_abi(lib, taps, L, M, lead, utts, finite=True):
    """ge2e_resample through raw pointers on guarded buffers -> the list of float32 outputs, one array per utterance.  In
    the wav buffer every utterance is followed by GAP NaN samples."""
    lens = [len(u) for u in utts]
    starts, at, parts = [], 0, []
    for u in utts:
        starts.append(at)
        parts += [u, np.full(GAP, np.nan, dtype=np.float32)]
        at += len(u) + GAP
    wav = Buf((at,), data=np.concatenate(parts))
    os = out_starts(lens, L, M)
    idx = torch.as_tensor(np.array(starts + lens + os, dtype=np.int64)).to(dev())
    U = len(utts)
    t = tables(taps, L, M, lead)
    assert t.packed is not None
    out = Buf((os[-1],))
    p8 = idx.data_ptr()
    ok(lib.ge2e_resample(t.packed.data_ptr(), wav.ptr, p8, p8 + 8 * U, p8 + 16 * U, U, os[-1], L, M, lead, out.ptr, None),
       "ge2e_resample")
    got = out.get("ge2e_resample", finite=finite)
    assert wav.guards_intact()
    return [got[a:b] for a, b in zip(os, os[1:])]


def within_bound(what, got, x, taps, L, M, lead):
    y64, mag = rr.resample_ref(x, taps, L, M, lead)
    W = 2 * lead + 1
    assert got.shape == y64.shape, (what, got.shape, y64.shape)
    if len(y64) == 0:
        return 0.0
    bound = (W + 1) * 2.0 ** -24 * mag
    diff = np.abs(got.astype(np.float64) - y64)
    worst = float((diff / np.where(bound > 0, bound, 1.0)).max())
    assert (diff <= bound).all(), (what, int(np.argmax(diff - bound)), worst)
    return worst


@pytest.mark.parametrize("L,M", RATIOS)
def test_against_the_oracle(lib, L, M):
    lead, taps = bank32(L, M)
    utts = [noise(237, 1), noise(1000, 2, amp=1.0), noise(64, 3)]
    got = res_abi(lib, taps, L, M, lead, utts)
    worst = max(within_bound((L, M, i), g, u, taps, L, M, lead) for i, (g, u) in enumerate(zip(got, utts)))
    print(f"({L}, {M}), W {2 * lead + 1}: the worst output is at {worst:.3f} of the bound")


@pytest.mark.parametrize("name", ["kaiser_best", "kaiser_fast"])
def test_the_presets_at_44100(lib, name):
    L, M = rr.ratio(44100, 16000)
    lead, taps = bank32(L, M, name)
    assert (L, M, 2 * lead + 1) == (160, 441, {"kaiser_best": 355, "kaiser_fast": 91}[name])
    x = noise(2000, 4, amp=0.5)
    got, = res_abi(lib, taps, L, M, lead, [x])
    print(f"{name}: the worst output is at {within_bound(name, got, x, taps, L, M, lead):.3f} of the bound")


def test_every_tap_exactly(lib):
    """441 utterances, a unit impulse at sample 100 + j in utterance j: over one period of M every phase and every k is
    picked out, as float32 equality."""
    L, M = 160, 441
    lead, taps = bank32(L, M)
    W, n_in = 2 * lead + 1, 1000
    utts = []
    for j in range(M):
        x = np.zeros(n_in, dtype=np.float32)
        x[100 + j] = 1.0
        utts.append(x)
    got = res_abi(lib, taps, L, M, lead, utts)
    idx, phase = rr.indices(n_in, L, M, lead, W)              # sample of tap k of output n
    seen = np.zeros((L, W), dtype=bool)
    for j, g in enumerate(got):
        hit = idx == 100 + j                                   # at most one k per output
        want = np.where(hit.any(axis=1), taps[phase, hit.argmax(axis=1)], np.float32(0.0))
        assert np.array_equal(g, want), (j, int(np.argmax(g != want)))
        seen[phase[hit.any(axis=1)], hit.argmax(axis=1)[hit.any(axis=1)]] = True
    assert seen.all()


def test_identity_copies_bit_for_bit(lib):
    taps = np.ones((1, 1), dtype=np.float32)
    utts = [noise(1, 5), noise(2047, 6), noise(2048, 7), noise(4100, 8)]
    utts[1][3] = -0.0
    utts[3][17] = np.float32(1e-42)                            # a denormal stays one
    for g, u in zip(res_abi(lib, taps, 1, 1, 0, utts), utts):
        assert same_bits(g, u)


@pytest.mark.parametrize("L,M", [(1, 3), (160, 441), (2, 1)])
def test_edges_of_lengths_and_tiles(lib, L, M):
    lead, taps = bank32(L, M)
    tile = tile_of(L, M, lead)
    # the lengths whose output counts are the tile - 1, + 0 and + 1 (when up-sampling: the counts there are next to them)
    at_tile = sorted({(tile + d) * M // L for d in (-1, 0, 1)} | {-(-(tile + d) * M // L) for d in (-1, 0, 1)})
    counts = {rr.out_length(n, L, M) for n in at_tile}
    assert tile in counts and min(counts) < tile < max(counts) and (L > M or {tile - 1, tile + 1} <= counts)
    lens = [0, 1, lead - 1, lead, lead + 1, 0] + at_tile + [0, 37]
    utts = [noise(n, 20 + i, amp=1.0) for i, n in enumerate(lens)]
    got = res_abi(lib, taps, L, M, lead, utts)
    assert [len(g) for g in got] == [rr.out_length(n, L, M) for n in lens] and len(got[0]) == len(got[5]) == 0
    for i, (g, u) in enumerate(zip(got, utts)):
        within_bound((L, M, lens[i]), g, u, taps, L, M, lead)
    # an utterance of length 0 between two others leaves both as they are alone
    a, b = utts[1], utts[-1]
    three = res_abi(lib, taps, L, M, lead, [a, np.zeros(0, dtype=np.float32), b])
    assert len(three[1]) == 0 and same_bits(three[0], res_abi(lib, taps, L, M, lead, [a])[0])
    assert same_bits(three[2], res_abi(lib, taps, L, M, lead, [b])[0])


@pytest.mark.parametrize("L,M", [(1, 3), (160, 441), (3, 2)])
def test_neighbours_do_not_leak_in(lib, L, M):
    lead, taps = bank32(L, M)
    x = noise(700, 30, amp=1.0)
    nan = np.full(300, np.nan, dtype=np.float32)
    alone, = res_abi(lib, taps, L, M, lead, [x])
    got = res_abi(lib, taps, L, M, lead, [nan, x, nan], finite=False)
    assert same_bits(got[1], alone) and np.isfinite(alone).all()
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all()


@pytest.mark.parametrize("L,M,bad", [(1, 3, (0,)), (1, 3, (350,)), (160, 441, (699,)), (160, 441, (3, 400)), (2, 1, (123,))])
def test_a_nan_sample_poisons_exactly_its_windows(lib, L, M, bad):
    lead, taps = bank32(L, M)
    x = noise(700, 31, amp=1.0)
    clean, = res_abi(lib, taps, L, M, lead, [x])
    dirty = x.copy()
    dirty[list(bad)] = np.nan
    got, = res_abi(lib, taps, L, M, lead, [dirty], finite=False)
    hit = np.zeros(len(clean), dtype=bool)
    for j in bad:
        hit |= rr.windows_holding(700, L, M, lead, j)
    assert 1 <= hit.sum() < len(clean) // 2
    assert np.isnan(got[hit]).all() and same_bits(got[~hit], clean[~hit])


def test_rows_do_not_depend_on_their_batch_and_calls_repeat(lib):
    for L, M in ((1, 3), (160, 441)):
        lead, taps = bank32(L, M)
        tile = tile_of(L, M, lead)
        a, b, c = noise(900, 32), noise(tile * M // L + 500, 33), noise(333, 34)       # b spans two tiles
        alone, = res_abi(lib, taps, L, M, lead, [b])
        batch = res_abi(lib, taps, L, M, lead, [a, b, c])
        assert len(alone) > tile and same_bits(batch[1], alone)
        again = res_abi(lib, taps, L, M, lead, [a, b, c])
        assert all(same_bits(g, h) for g, h in zip(batch, again))


@pytest.mark.parametrize("L,M", [(160, 441), (1, 3), (2, 1)])
def test_empty_utterances_first_in_a_run_and_last_but_one(lib, L, M):
    """Empty utterances own one block each and share their out_start with the next utterance: first, in a run of two and
    last but one.  A block must find its own utterance whatever stands around it: every utterance of the batched call is
    held to resample_ref by the oracle's bound (a float64 oracle: the bound, not equality, is its comparison) and equals,
    to the bit, the same entry on that utterance alone."""
    lead, taps = bank32(L, M, "kaiser_fast")
    lens = [0, 5, 0, 0, 900, 0, 1]
    utts = [noise(n, 50 + i, amp=1.0) for i, n in enumerate(lens)]
    got = res_abi(lib, taps, L, M, lead, utts)
    assert [len(g) for g in got] == [rr.out_length(n, L, M) for n in lens]
    for i, (g, u) in enumerate(zip(got, utts)):
        within_bound((L, M, i), g, u, taps, L, M, lead)
        if len(u):
            assert same_bits(g, res_abi(lib, taps, L, M, lead, [u])[0]), i


# ---- the instantiations the shapes above do not reach -------------------------------------------------------------------------
# The ratios above run resample<lds,8> and, at (160, 441), resample<lds,2>.  (L, M, lead) for the other three: four outputs a
# thread (96 kHz -> 16 kHz under kaiser_best has this shape: W 769), one output a thread, and a span LDS does not hold, read
# from global memory.  Synthetic banks: the kernel takes any taps.
OTHER = {"lds,4": (1, 6, 384), "lds,1": (1, 32, 6), "global,4": (1, 64, 6)}


@functools.lru_cache(maxsize=None)
def synthetic_bank(L, M, lead):
    W = 2 * lead + 1
    taps = (np.random.default_rng(100 * M + lead).standard_normal((L, W)) / np.sqrt(W)).astype(np.float32)
    taps.setflags(write=False)
    return taps


@pytest.mark.parametrize("name", list(OTHER))
def test_the_other_instantiations_against_the_oracle(lib, name):
    from speaker_embedding_ge2e_loss_amd import _lib
    L, M, lead = OTHER[name]
    taps = synthetic_bank(L, M, lead)
    assert _lib.resample_plan(1, 1, L, M, lead)[0].startswith(f"resample<{name}>/")
    tile = tile_of(L, M, lead)
    # two tiles and a bit, the tile exactly, one sample, nothing, a short one
    lens = [tile * M // L + 37, tile * M // L, 1, 0, 300]
    utts = [noise(n, 80 + i, amp=1.0) for i, n in enumerate(lens)]
    got = res_abi(lib, taps, L, M, lead, utts)
    assert len(got[0]) > tile and len(got[1]) == tile
    worst = max(within_bound((name, n), g, u, taps, L, M, lead) for n, g, u in zip(lens, got, utts))
    print(f"{name}: ({L}, {M}), W {2 * lead + 1}: the worst output is at {worst:.3f} of the bound")
    # an utterance does not depend on its batch, and calls repeat
    assert same_bits(res_abi(lib, taps, L, M, lead, [utts[0]])[0], got[0])
    assert all(same_bits(g, h) for g, h in zip(got, res_abi(lib, taps, L, M, lead, utts)))


@pytest.mark.parametrize("name", list(OTHER))
def test_the_other_instantiations_tap_by_tap(lib, name):
    """A unit impulse in each of M utterances, over one period of M around the end of the first tile: every tap as float32
    equality, through windows that lie in the first tile, in the second and across both."""
    L, M, lead = OTHER[name]
    taps = synthetic_bank(L, M, lead)
    W, tile = 2 * lead + 1, tile_of(L, M, lead)
    n_in = tile * M // L + 2 * lead + 2 * M
    j0 = tile * M // L - M                                     # i0 of the first tile's last output: its window and the next one's
    utts = []
    for j in range(M):
        x = np.zeros(n_in, dtype=np.float32)
        x[j0 + j] = 1.0
        utts.append(x)
    got = res_abi(lib, taps, L, M, lead, utts)
    idx, phase = rr.indices(n_in, L, M, lead, W)
    seen = np.zeros((L, W), dtype=bool)
    tiles_hit = set()
    for j, g in enumerate(got):
        hit = idx == j0 + j
        rows = hit.any(axis=1)
        want = np.where(rows, taps[phase, hit.argmax(axis=1)], np.float32(0.0))
        assert np.array_equal(g, want), (name, j, int(np.argmax(g != want)))
        seen[phase[rows], hit.argmax(axis=1)[rows]] = True
        tiles_hit |= set((np.nonzero(rows)[0] // tile).tolist())
    assert seen.all() and tiles_hit == {0, 1}


@pytest.mark.parametrize("name", list(OTHER))
def test_the_other_instantiations_poison_exactly_their_windows(lib, name):
    L, M, lead = OTHER[name]
    taps = synthetic_bank(L, M, lead)
    tile = tile_of(L, M, lead)
    n_in = tile * M // L + 40 * M
    x = noise(n_in, 90, amp=1.0)
    bad = (0, tile * M // L - 1, n_in - M)                                     # the start, the tiles' seam, the last output's centre
    clean = res_abi(lib, taps, L, M, lead, [x, x[:100]])
    dirty = x.copy()
    dirty[list(bad)] = np.nan
    nan = np.full(64, np.nan, dtype=np.float32)
    got = res_abi(lib, taps, L, M, lead, [nan, dirty, nan, x[:100]], finite=False)
    hit = np.zeros(len(clean[0]), dtype=bool)
    for j in bad:
        hit |= rr.windows_holding(n_in, L, M, lead, j)
    assert 3 <= hit.sum() < len(hit)
    assert np.isnan(got[1][hit]).all() and same_bits(got[1][~hit], clean[0][~hit])
    assert same_bits(got[3], clean[1])                                          # the NaN neighbours do not leak in


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_functional_resample_is_the_abi_call(GF, lib):
    for L, M in ((1, 3), (160, 441)):
        lead, taps = bank32(L, M)
        utts = [noise(900, 35, amp=1.0), noise(0, 36), noise(1700, 37, amp=1.0)]
        lens = [len(u) for u in utts]
        wav = torch.as_tensor(np.concatenate(utts)).to(dev())
        t = tables(taps, L, M, lead)
        want = res_abi(lib, taps, L, M, lead, utts)
        got, out_lens = GF.resample(t, wav, lens)
        assert out_lens == [len(w) for w in want] and same_bits(got.cpu().numpy(), np.concatenate(want))
        assert torch.equal(GF.resample(t, wav, torch.tensor(lens), native=True)[0], got)
        one, n1 = GF.resample(t, wav[:900])                                     # a 1-D tensor without lengths: one utterance
        assert n1 == [len(want[0])] and same_bits(one.cpu().numpy(), want[0])
        # the torch route on the same device, within the same bound
        slow, slow_lens = GF.resample(t, wav, lens, native=False)
        assert slow_lens == out_lens
        at = 0
        for u, n in zip(utts, out_lens):
            within_bound(("torch route", L, M), slow[at:at + n].cpu().numpy(), u, taps, L, M, lead)
            at += n
        with pytest.raises(ValueError):
            GF.resample(t, wav, [len(wav) + 1])
        with pytest.raises(ValueError):
            GF.resample(t, wav, lens, layout=GF.resample_layout(lens, L + 1, M, device=dev()))


def test_an_unsupported_width_takes_the_torch_route(GF):
    L, M, lead = 1, 3, 513                                                      # W = 1027: no kernel
    assert not GF.resample_supported(L, M, 2 * lead + 1)
    taps = (np.random.default_rng(38).standard_normal((L, 2 * lead + 1)) / 30).astype(np.float32)
    t = GF.resample_pack(torch.as_tensor(taps).to(dev()), L, M, lead)
    assert t.packed is None and (t.up, t.down, t.lead, t.width) == (L, M, lead, 2 * lead + 1)
    x = noise(2500, 39, amp=1.0)
    wav = torch.as_tensor(x).to(dev())
    got, lens = GF.resample(t, wav)
    assert lens == [rr.out_length(2500, L, M)]
    within_bound("W 1027", got.cpu().numpy(), x, taps, L, M, lead)
    with pytest.raises(RuntimeError):
        GF.resample(t, wav, native=True)


# ---- the gain ---------------------------------------------------------------------------------------------------------------
def gain_abi(lib, utts, target=-30.0, increase_only=True, finite=True):
    """ge2e_volume_gain through raw pointers on guarded buffers -> (U,) float32."""
    lens = [len(u) for u in utts]
    starts, at, parts = [], 0, []
    for u in utts:
        starts.append(at)
        parts += [u, np.full(GAP, np.nan, dtype=np.float32)]
        at += len(u) + GAP
    wav = Buf((at,), data=np.concatenate(parts))
    U = len(utts)
    idx = torch.as_tensor(np.array(starts + lens, dtype=np.int64)).to(dev())
    out = Buf((U,))
    ws = Workspace(lib.ge2e_volume_gain_workspace_bytes(at, U))
    p8 = idx.data_ptr()
    ok(lib.ge2e_volume_gain(wav.ptr, p8, p8 + 8 * U, U, target, int(increase_only), out.ptr, ws.ptr, None), "ge2e_volume_gain")
    got = out.get("ge2e_volume_gain", finite=finite)
    ws.check("ge2e_volume_gain")
    assert wav.guards_intact()
    return got


def test_gain_against_the_oracle(lib):
    tile, slices = 2048, 128
    lens = [1, 2, tile - 1, tile, tile + 1, 5000, slices * tile + 5]            # the last: every slice, the first one twice
    utts = [noise(n, 40 + i, amp=10.0 ** -(i % 4)) for i, n in enumerate(lens)]
    for target, inc in ((-30.0, True), (-30.0, False), (-27.5, True)):
        got = gain_abi(lib, utts, target, inc)
        for g, u in zip(got, utts):
            want = rr.gain_ref(u, target, inc)
            assert g in rr.float32_neighbours(want), (len(u), target, inc, g, want)
    # increase_only, on both sides of the target
    loud, quiet = noise(3000, 50, amp=1.0), noise(3000, 51, amp=1e-4)
    inc, both = gain_abi(lib, [loud, quiet], increase_only=True), gain_abi(lib, [loud, quiet], increase_only=False)
    assert inc[0] == 1.0 and both[0] < 0.05 and inc[1] == both[1] and inc[1] > 100.0


def test_gain_of_silence_and_of_nothing(lib):
    got = gain_abi(lib, [np.zeros(3000, dtype=np.float32), noise(100, 52), np.zeros(0, dtype=np.float32)], finite=False)
    assert got[0] == np.inf and np.isnan(got[2]) and got[1] in rr.float32_neighbours(rr.gain_ref(noise(100, 52)))
    got = gain_abi(lib, [np.zeros(3000, dtype=np.float32)], increase_only=False, finite=False)
    assert got[0] == np.inf


def test_gain_does_not_depend_on_the_batch_and_calls_repeat(lib):
    a, b, c = noise(700, 53), noise(128 * 2048 + 4097, 54, amp=0.01), noise(2049, 55, amp=1e-3)
    alone = gain_abi(lib, [b])
    batch = gain_abi(lib, [a, b, c])
    assert same_bits(batch[1:2], alone) and same_bits(batch, gain_abi(lib, [a, b, c]))
    assert same_bits(gain_abi(lib, [c, a, b])[2:3], alone)


def test_functional_volume_gain_is_the_abi_call(GF, lib):
    utts = [noise(1500, 56), noise(0, 57), noise(4100, 58, amp=1e-3)]
    lens = [len(u) for u in utts]
    wav = torch.as_tensor(np.concatenate(utts)).to(dev())
    want = gain_abi(lib, utts, -25.0, True, finite=False)
    got = GF.volume_gain(wav, lens, target_dbfs=-25.0)
    assert same_bits(got.cpu().numpy(), want)
    assert same_bits(GF.volume_gain(wav[:1500]).cpu().numpy(), gain_abi(lib, utts[:1]))
    from speaker_embedding_ge2e_loss_amd import audio
    slow = GF.volume_gain(wav, lens, target_dbfs=-25.0, native=False)
    assert same_bits(slow.cpu().numpy(), audio.volume_gain(wav, lens, -25.0, True).cpu().numpy())
    assert np.allclose(slow.cpu().numpy()[[0, 2]], want[[0, 2]], rtol=1e-6)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------
def front_end():
    from speaker_embedding_ge2e_loss_amd.audio import MelFrontEnd
    return MelFrontEnd(16000, 512, 160, 40, 90.0, 7600.0, 10, 20, 10.0, 0.75)


def recordings():
    return [torch.as_tensor(noise(n, 60 + i, amp=0.01 * (i + 1))).to(dev()) for i, n in enumerate((7500, 12000, 19500))]


def test_frames_at_a_source_rate_is_resample_then_melspec(GF):
    fe, wavs = front_end(), recordings()
    t = fe.resampler(48000, dev())
    assert t is fe.resampler(48000, "cuda") and t is not fe.resampler(48000, dev(), "kaiser_fast")
    assert (t.up, t.down, t.width) == (1, 3, 385) and t.packed is not None
    flat, lens = GF.resample(t, torch.cat(wavs), [w.numel() for w in wavs])
    assert lens == [2500, 4000, 6500]
    got, fs = fe.frames(wavs, source_rate=48000)
    want, fs2 = GF.melspec(fe.tables(dev()), flat, lens, hop=160)
    assert fs == fs2 and torch.equal(got, want) and bool(torch.isfinite(got).all())
    # with the gain and the pad to the partial slices: both from the resampled signal
    got, fs = fe.frames(wavs, normalize_volume=True, pad_to_partials=True, source_rate=48000)
    gain = GF.volume_gain(flat, lens, fe.target_dbfs)
    assert bool((gain > 1).all())
    want, fs2 = GF.melspec(fe.tables(dev()), flat, lens, hop=160, padded_lengths=[fe.slices(n).padded_length for n in lens], gain=gain)
    assert fs == fs2 and torch.equal(got, want)
    part = fe.partials(wavs, source_rate=48000)
    assert [p.shape[0] for p in part] == [len(fe.slices(n).mel_starts) for n in lens] == [1, 2, 3]
    # the other preset is another signal
    assert not torch.equal(fe.frames(wavs, source_rate=48000, resample_filter="kaiser_fast")[0], fe.frames(wavs, source_rate=48000)[0])


def test_frames_without_a_source_rate_is_todays_call(GF):
    from speaker_embedding_ge2e_loss_amd import audio
    fe, wavs = front_end(), recordings()
    lens = [w.numel() for w in wavs]
    flat = torch.cat(wavs)
    want, fs = GF.melspec(fe.tables(dev()), flat, lens, hop=160, padded_lengths=[fe.slices(n).padded_length for n in lens],
                          gain=audio.volume_gain(flat, lens, fe.target_dbfs, increase_only=True))
    for rate in (None, 16000):
        got, fs2 = fe.frames(wavs, normalize_volume=True, pad_to_partials=True, source_rate=rate)
        assert fs == fs2 and torch.equal(got, want)
    assert not fe._resamplers


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


def test_embed_audio_at_a_source_rate(GF):
    n_mels, H, L, D = 40, 128, 2, 64
    fe, wavs = front_end(), recordings()
    m = module_with(enc.random_params(n_mels, H, L, D, seed=21), n_mels, H, L, D)
    got = m.embed_audio(wavs, fe, normalize_volume=True, source_rate=48000)
    assert got.shape == (3, D) and bool(torch.isfinite(got).all())
    assert np.allclose(got.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)
    # the d-vectors of the resampled recordings handed in at the model's rate (their gain from the torch route, which may
    # round the other way): close, and without the gain the very same bits
    flat, lens = GF.resample(fe.resampler(48000, dev()), torch.cat(wavs), [w.numel() for w in wavs])
    at16 = list(torch.split(flat, lens))
    assert same_bits(m.embed_audio(wavs, fe, source_rate=48000).cpu().numpy(), m.embed_audio(at16, fe).cpu().numpy())
    assert np.abs(got.cpu().numpy() - m.embed_audio(at16, fe, normalize_volume=True).cpu().numpy()).max() < 1e-4


def test_resample_and_gain_are_captured_in_a_graph(GF):
    L, M = 160, 441
    lead, taps = bank32(L, M)
    t = tables(taps, L, M, lead)
    lens = [1500, 0, 2600]
    x = torch.as_tensor(np.concatenate([noise(1500, 70), noise(2600, 71, amp=1e-3)])).to(dev())
    x2 = torch.flip(x, dims=(0,)) * 0.5
    lay = GF.resample_layout(lens, L, M, device=dev())
    lay_out = GF.resample_layout(lay.out_lengths, 1, 1, device=dev())           # where the resampled utterances lie
    eager = []
    for w in (x, x2):
        y, _ = GF.resample(t, w, lens)
        eager.append((y.clone(), GF.volume_gain(y, lay.out_lengths).clone()))
    torch.cuda.synchronize()
    static_x = x.clone()
    static_y = torch.full((lay.out_start[-1],), float("nan"), device=dev())
    static_g = torch.full((3,), float("nan"), device=dev())
    ws = GF.volume_gain_workspace(static_y.numel(), 3, dev())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        GF.resample(t, static_x, layout=lay, out=static_y)
        GF.volume_gain(static_y, layout=lay_out, out=static_g, workspace=ws)
    for w, (want_y, want_g) in zip((x, x2), eager):
        static_y.fill_(float("nan"))
        static_g.fill_(float("nan"))
        static_x.copy_(w)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, want_y)
        assert same_bits(static_g.cpu().numpy(), want_g.cpu().numpy())           # (a NaN for the empty utterance)
