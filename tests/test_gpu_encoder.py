"""GPU: the native encoder (ge2e_encoder_pack / ge2e_encode, functional.encode, SpeakerEncoder.embed / embed_utterances)
against tests/encoder_ref.py in float64.  The C ABI is called with raw pointers on guarded buffers (tests/guarded.py): the
mels between NaN guards, the output NaN-poisoned between guards.

The accuracy gate is calibrated on the reference, never on the code under test: err_ref is the relative Frobenius error of
torch's CPU float32 nn.LSTM + Linear path against encoder_ref in float64 on the case's own inputs, and the native output
must satisfy err <= 4 err_ref + 2^-22 (encoder_ref.gate).  The 4: a hand-written fp32 LSTM in another summation order gave
0.57 .. 1.12 of err_ref, and the device's expf / tanhf are 1-2 ulp; the floor is two ulps of a unit-vector component.
check_rows holds the worst ROW to the same rule -- row-wise relative 2-norm errors, 4 x the yardstick's worst row plus the
same floor -- so that one bad row among R is not diluted by sqrt(R); the yardstick's worst row is 1.3 .. 1.4 times its batch
error.  The shape, edge and poison cases come from tests/encoder_cases.py, which tests/test_encoder_cases.py holds to what
they are there for on the float64 reference alone.

Measured on an MI355X, the worst row's err / the yardstick's worst row (the gate allows 4 plus the floor; normalised / raw):
(H, L) grid at (R, T, n_mels, D) = (17, 5, 20, 24): (128, 1) 2.00 / 1.98, (128, 2) 1.67 / 1.74, (128, 3) 2.02 / 2.08,
(128, 4) 2.37 / 2.50, (256, 1) 2.22 / 2.18, (256, 2) 2.19 / 2.25, (256, 3) 2.39 / 2.72, (256, 4) 2.42 / 2.59.
n_mels edges (three rows of two frames, errors near 3e-7, so the floor carries a third of the gate): H = 128: 1: 2.51 / 3.33,
3: 2.22 / 4.59 (3.6e-7 under a gate of 5.5e-7), 4: 2.52 / 2.74, 15: 2.25 / 2.27, 16: 2.85 / 3.82, 17: 2.65 / 2.39,
255: 1.45 / 1.60, 256: 1.02 / 1.14; H = 256: 17: 3.30 / 3.33, 256: 1.46 / 1.26.
D edges: H = 128: 1: exact / 1.02, 15: 2.37 / 2.87, 16: 2.35 / 2.84, 17: 2.16 / 2.34, 127: 2.77 / 2.85, 128: 2.65 / 2.75,
129: 3.00 / 3.26, 255: 2.12 / 2.92, 256: 2.88 / 3.29; H = 256: 129: 3.04 / 3.46, 256: 2.52 / 2.68.
A row holding one +-Inf: 1.15 .. 3.70; windows in place at (256, 4): 2.42; through a guarded pack: 1.85.  The earlier
cases row by row: 1.11 .. 2.90, and t1 (one row, one frame) 4.02 at 1.6e-7 under a gate of 4.0e-7."""
import functools
import os

import numpy as np
import pytest
import torch

import encoder_cases as ec
import encoder_ref as enc
from capi import GF, lib, ok  # noqa: F401
from guarded import Buf, dev, same_bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "callers")

# name -> (R, T, n_mels, H, L, D, weight scale, input scale)
CASES = {
    "t1":            (1, 1, 12, 128, 1, 16, 1.0, 1.0),       # T = 1: no recurrence, zero initial state
    "t1_four":       (3, 1, 12, 128, 4, 37, 1.0, 1.0),       # four layers at T = 1
    "mels13":        (5, 3, 13, 128, 2, 64, 1.0, 1.0),       # n_mels not a multiple of 4
    "rows31":        (31, 2, 40, 128, 2, 64, 1.0, 1.0),      # just below the tile
    "rows32":        (32, 2, 40, 128, 2, 64, 1.0, 1.0),      # the tile
    "rows33":        (33, 2, 40, 128, 2, 64, 1.0, 1.0),      # just above it
    "reference":     (33, 160, 80, 256, 3, 256, 1.0, 1.0),   # the reference's model at its real length, with a tail tile
    "saturated":     (17, 160, 80, 256, 3, 256, 4.0, 1.0),   # weights x 4: saturated gates
    "far_out":       (33, 40, 40, 128, 2, 64, 1.0, 30.0),    # inputs x 30: pre-activations far beyond +-100
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Parameters, inputs, the float64 reference and err_ref of a case; computed once, shared, never changed."""
    R, T, n_mels, H, L, D, wscale, xscale = CASES[name]
    seed = sorted(CASES).index(name)
    ps = enc.random_params(n_mels, H, L, D, seed=100 + seed, scale=wscale)
    x = (np.random.default_rng(200 + seed).uniform(0.0, 0.96, (R, T, n_mels)) * xscale).astype(np.float32)
    return ec.finish(dict(shape=(R, T, n_mels, H, L, D), params=ps, x=x))


@functools.lru_cache(maxsize=None)
def fixture_case():
    w = np.load(os.path.join(GOLD, "encoder_weights.npz"))
    z = np.load(os.path.join(GOLD, "encoder.npz"))
    n_mels, H, L, D = (int(v) for v in z["cfg"][:4])
    ps = [w[f"LSTM_stack.{n}_l{l}"] for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    ps += [w["projection.weight"], w["projection.bias"]]
    x = z["mels"].astype(np.float32)                                           # the cast of s2:28
    c = ec.finish(dict(shape=(x.shape[0], x.shape[1], n_mels, H, L, D), params=ps, x=x))
    c["mels64"], c["out64"] = z["mels"], z["out64"]
    return c


@functools.lru_cache(maxsize=None)
def packed_for(name):
    c = fixture_case() if name == "fixture" else case(name)
    _, _, n_mels, H, L, D = c["shape"]
    from speaker_embedding_ge2e_loss_amd import functional
    return functional.encoder_pack(torch.as_tensor(enc.flat(c["params"])).to(dev()), n_mels, H, L, D)


def encode_abi(lib, packed, x, shape, normalize=True, row_start=None, R=None):
    """ge2e_encode through raw pointers on guarded buffers -> (R, D) float32 numpy; `x` dense (R, T, n_mels) or, with
    row_start, flat (frames, n_mels)."""
    _, T, n_mels, H, L, D = shape
    R = shape[0] if R is None else R
    mel = Buf(x.shape, data=x)
    out = Buf((R, D))
    rs = None
    if row_start is not None:
        rs = torch.as_tensor(np.asarray(row_start, dtype=np.int64)).to(dev())
    ok(lib.ge2e_encode(packed.data_ptr(), mel.ptr, None if rs is None else rs.data_ptr(), R, T, n_mels, H, L, D,
                       int(normalize), out.ptr, None), "ge2e_encode")
    got = out.get("ge2e_encode", finite=False)
    assert mel.guards_intact()
    return got


@functools.lru_cache(maxsize=None)
def native(name):
    """The native output of a case, computed once (the bitwise tests compare against it)."""
    from speaker_embedding_ge2e_loss_amd import _lib
    c = fixture_case() if name == "fixture" else case(name)
    got = encode_abi(_lib.load(), packed_for(name), c["x"], c["shape"])
    got.setflags(write=False)
    return got


def check_gate(what, got, ref, err_ref):
    assert np.isfinite(got).all(), f"{what}: NaN or inf in the output"
    err = enc.rel_err(got, ref)
    print(f"{what}: err {err:.3e}, err_ref {err_ref:.3e}, gate {enc.gate(err_ref):.3e}")
    assert err <= enc.gate(err_ref), (what, err, err_ref)


def check_rows(what, got, ref, ref32):
    """The same gate row by row: the worst row's relative error against 4 x the yardstick's worst row plus the floor (one
    bad row among R is diluted by sqrt(R) in check_gate's batch norm)."""
    assert np.isfinite(got).all(), f"{what}: NaN or inf in the output"
    err, err_ref = ec.row_errs(got, ref).max(), ec.row_errs(ref32, ref).max()
    ratio = f"{err / err_ref:.2f}" if err_ref > 0 else "-"
    print(f"{what}: worst row err {err:.3e}, err_ref {err_ref:.3e}, ratio {ratio}, gate {enc.gate(err_ref):.3e}")
    assert err <= enc.gate(err_ref), (what, err, err_ref)


@pytest.mark.parametrize("name", list(CASES))
def test_encode_against_float64(lib, name):
    c = case(name)
    check_gate(name, native(name), c["ref"], c["err_ref"])
    check_rows(name, native(name), c["ref"], c["ref32"])
    if name in ("t1", "reference", "saturated"):
        assert np.abs(np.linalg.norm(native(name).astype(np.float64), axis=1) - 1).max() < 1e-6


def test_encode_the_reference_encoders_fixture(lib):
    c = fixture_case()
    got = native("fixture")
    check_gate("fixture", got, c["ref"], c["err_ref"])
    check_gate("fixture against the reference's own float64 output", got, c["out64"], c["err_ref"])


def test_raw_projection_and_the_zero_row(lib):
    for name in ("mels13", "rows33"):
        c = case(name)
        got = encode_abi(lib, packed_for(name), c["x"], c["shape"], normalize=False)
        check_gate(name + " raw", got, c["raw"], c["err_ref_raw"])
    # a projection that is exactly zero: NaN when normalised (s2:34 divides without an epsilon), +0 raw
    c = case("mels13")
    R, T, n_mels, H, L, D = c["shape"]
    ps = [p.copy() for p in c["params"]]
    ps[-2][:] = 0
    ps[-1][:] = 0
    from speaker_embedding_ge2e_loss_amd import functional
    packed = functional.encoder_pack(torch.as_tensor(enc.flat(ps)).to(dev()), n_mels, H, L, D)
    assert np.isnan(encode_abi(lib, packed, c["x"], c["shape"])).all()
    assert not encode_abi(lib, packed, c["x"], c["shape"], normalize=False).any()


def test_rows_do_not_depend_on_their_batch(lib):
    c = case("reference")
    full = native("reference")
    R, T, n_mels, H, L, D = c["shape"]
    alone = encode_abi(lib, packed_for("reference"), c["x"][5:7], (2, T, n_mels, H, L, D))
    assert same_bits(alone, full[5:7])
    last = encode_abi(lib, packed_for("reference"), c["x"][32:33], (1, T, n_mels, H, L, D))    # the tail tile's only row
    assert same_bits(last, full[32:33])


def test_rows_do_not_depend_on_the_tile_count_and_calls_repeat(lib):
    c = case("far_out")
    _, T, n_mels, H, L, D = c["shape"]
    x = np.concatenate([c["x"], c["x"][::-1] * 0.01])[:64]
    shape = (64, T, n_mels, H, L, D)
    one = encode_abi(lib, packed_for("far_out"), x, shape)
    again = encode_abi(lib, packed_for("far_out"), x, shape)
    assert same_bits(one, again)
    halves = [encode_abi(lib, packed_for("far_out"), x[i:i + 32], (32, T, n_mels, H, L, D)) for i in (0, 32)]
    assert same_bits(one, np.concatenate(halves))
    assert same_bits(one[:33], native("far_out"))


@pytest.mark.parametrize("T,hop,n_mels", [(160, 80, 40), (160, 7, 40), (20, 7, 13)])
def test_windows_addressed_in_place(lib, T, hop, n_mels):
    H, L, D = 128, 2, 64
    n = 5
    frames = T + (n - 1) * hop
    ps = enc.random_params(n_mels, H, L, D, seed=300 + hop + n_mels)
    from speaker_embedding_ge2e_loss_amd import functional
    packed = functional.encoder_pack(torch.as_tensor(enc.flat(ps)).to(dev()), n_mels, H, L, D)
    flat = np.full((frames + 9, n_mels), np.nan, dtype=np.float32)           # frames past the last window: NaN
    flat[:frames] = np.random.default_rng(hop).uniform(0, 0.96, (frames, n_mels))
    starts = [i * hop for i in range(n)]
    dense = np.stack([flat[s:s + T] for s in starts])
    shape = (n, T, n_mels, H, L, D)
    want = encode_abi(lib, packed, dense, shape)
    got = encode_abi(lib, packed, flat, shape, row_start=starts, R=n)
    assert np.isfinite(got).all() and same_bits(got, want)
    ref = enc.encode_ref(ps, dense.astype(np.float64))
    check_gate(f"windows T {T} hop {hop}", got, ref, enc.rel_err(enc.torch_encode(ps, dense, torch.float32), ref))
    # the windows in another order, one of them twice
    order = [3, 0, 0, 4]
    got = encode_abi(lib, packed, flat, shape, row_start=[starts[i] for i in order], R=len(order))
    assert same_bits(got, want[order])


# ---- tests/encoder_cases.py: every (H, L), the n_mels and D edges, poisoned rows, the pack kernel on its own --------------------
def pack(ps, shape):
    from speaker_embedding_ge2e_loss_amd import functional
    n_mels, H, L, D = shape[-4:]
    return functional.encoder_pack(torch.as_tensor(enc.flat(ps)).to(dev()), n_mels, H, L, D)


@functools.lru_cache(maxsize=None)
def ec_packed(name):
    c = ec.case(name)
    return pack(c["params"], c["shape"])


@functools.lru_cache(maxsize=None)
def ec_native(name, normalize=True):
    """The native output of a case of encoder_cases, computed once (the poison tests compare bits against it)."""
    from speaker_embedding_ge2e_loss_amd import _lib
    c = ec.case(name)
    got = encode_abi(_lib.load(), ec_packed(name), c["x"], c["shape"], normalize=normalize)
    got.setflags(write=False)
    return got


def check_both_outputs(lib, name):
    """The normalised and the raw output of a case of encoder_cases under both gates -> (normalised, raw)."""
    c = ec.case(name)
    outs = []
    for normalize, ref, ref32, err_ref in ((True, "ref", "ref32", "err_ref"), (False, "raw", "raw32", "err_ref_raw")):
        got = encode_abi(lib, ec_packed(name), c["x"], c["shape"], normalize=normalize)
        what = name + ("" if normalize else " raw")
        check_gate(what, got, c[ref], c[err_ref])
        check_rows(what, got, c[ref], c[ref32])
        outs.append(got)
    return outs


@pytest.mark.parametrize("name", list(ec.GRID))
def test_every_hidden_size_and_depth_with_a_recurrence(lib, name):
    got, _ = check_both_outputs(lib, name)
    if name == "h256_l4":            # 128 KiB of dynamic LDS: the second call launches from the cached launch state
        c = ec.case(name)
        assert 4 * c["shape"][4] * 32 * c["shape"][3] == 128 * 1024
        assert same_bits(got, encode_abi(lib, ec_packed(name), c["x"], c["shape"]))


@pytest.mark.parametrize("name", list(ec.N_MELS_EDGES))
def test_n_mels_edges(lib, name):
    check_both_outputs(lib, name)


@pytest.mark.parametrize("name", list(ec.D_EDGES))
def test_d_edges(lib, name):
    got, _ = check_both_outputs(lib, name)
    if ec.case(name)["shape"][5] == 1:   # y / sqrtf(y y) is exact: +-1.0 with the sign of the float64 projection
        assert same_bits(got, np.sign(ec.case(name)["raw"]).astype(np.float32)), got.ravel()


@pytest.mark.parametrize("value", list(ec.POISON_VALUES))
@pytest.mark.parametrize("at", ec.POISON_AT)
@pytest.mark.parametrize("name", list(ec.POISON_SHAPES))
def test_one_rows_poison_stays_in_that_row(lib, name, at, value):
    c = ec.poisoned(name, at, value)
    row = at[0]
    others = np.arange(c["shape"][0]) != row
    for normalize, ref, ref32 in ((True, "ref", "ref32"), (False, "raw", "raw32")):
        got = encode_abi(lib, ec_packed(name), c["x"], c["shape"], normalize=normalize)
        assert same_bits(got[others], ec_native(name, normalize)[others]), (name, at, value, normalize)
        if value == "nan":
            assert np.isnan(got[row]).all()
        else:
            # one +-Inf saturates the gates of one step and the row stays finite, in float64 and in torch's float32 path
            # alike (tests/test_encoder_cases.py holds both to that for every case here: no accuracy check is dropped)
            assert np.isfinite(got[row]).all(), (name, at, value, normalize)
            check_rows(f"{name} {value} at {at}{'' if normalize else ' raw'}", got[row:row + 1], c[ref][row:row + 1],
                       c[ref32][row:row + 1])


def test_windows_addressed_in_place_at_four_layers_of_256(lib):
    n_mels, H, L, D, T, hop, n = 20, 256, 4, 24, 5, 1, 5
    frames = T + (n - 1) * hop
    ps = enc.random_params(n_mels, H, L, D, seed=320)
    packed = pack(ps, (n_mels, H, L, D))
    flat = np.full((frames + 9, n_mels), np.nan, dtype=np.float32)           # frames past the last window: NaN
    flat[:frames] = np.random.default_rng(321).uniform(0, 0.96, (frames, n_mels))
    starts = [i * hop for i in range(n)]
    dense = np.stack([flat[s:s + T] for s in starts])
    shape = (n, T, n_mels, H, L, D)
    want = encode_abi(lib, packed, dense, shape)
    got = encode_abi(lib, packed, flat, shape, row_start=starts, R=n)
    assert np.isfinite(got).all() and same_bits(got, want)
    ref = enc.encode_ref(ps, dense.astype(np.float64))
    ref32 = enc.torch_encode(ps, dense, torch.float32)
    check_gate("windows at (256, 4)", got, ref, enc.rel_err(ref32, ref))
    check_rows("windows at (256, 4)", got, ref, ref32)


@pytest.mark.parametrize("shape", ec.PACK_SHAPES)
def test_pack_on_its_own(lib, GF, shape):
    n_mels, H, L, D = shape
    n_packed = ec.packed_floats(*shape)
    assert lib.ge2e_encoder_packed_bytes(*shape) == 4 * n_packed

    def run(ps):
        flat = Buf((GF.encoder_flat_numel(*shape),), data=enc.flat(ps))          # a read past either end is a NaN
        packed = Buf((n_packed,))                                                # NaN poison: every byte is written
        ok(lib.ge2e_encoder_pack(flat.ptr, n_mels, H, L, D, packed.ptr, None), "ge2e_encoder_pack")
        got = packed.get("ge2e_encoder_pack")
        assert flat.guards_intact()
        return packed, got

    # whatever the order inside a tile: the values are the weights, the bias sums and the projection biases, each once,
    # and everything else is +0.0
    ps, expected = ec.integer_params(*shape)
    _, got = run(ps)
    assert np.array_equal(np.sort(got[got != 0]), expected)
    assert int((got.view(np.uint32) == 0).sum()) == n_packed - expected.size
    if shape == ec.PACK_SHAPES[0]:       # ... and the order is the one ge2e_encode reads
        c = ec.build((5, 3) + shape, seed=4000)
        packed, _ = run(c["params"])
        out = encode_abi(lib, packed.t, c["x"], c["shape"])
        assert packed.guards_intact()
        check_gate("through a guarded pack", out, c["ref"], c["err_ref"])
        check_rows("through a guarded pack", out, c["ref"], c["ref32"])


def module_with(ps, shape):
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    _, _, n_mels, H, L, D = shape
    m = SpeakerEncoder(n_mels, H, L, D)
    with torch.no_grad():
        for l in range(L):
            for n, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ps[4 * l:4 * l + 4]):
                getattr(m.LSTM_stack, f"{n}_l{l}").copy_(torch.as_tensor(p))
        m.projection.weight.copy_(torch.as_tensor(ps[-2]))
        m.projection.bias.copy_(torch.as_tensor(ps[-1]))
    return m.to(dev()).eval()


def test_module_embed(GF):
    c = case("rows33")
    R, T, n_mels, H, L, D = c["shape"]
    m = module_with(c["params"], c["shape"])
    x = torch.as_tensor(c["x"]).to(dev())
    e = m.embed(x, native=True)
    assert not e.requires_grad and same_bits(e.cpu().numpy(), native("rows33"))
    # native=None: the kernel from NATIVE_MIN_ROWS windows on (the same bits, row for row), torch's route below
    from speaker_embedding_ge2e_loss_amd import encoder as E
    big = x.repeat(E.NATIVE_MIN_ROWS // R + 1, 1, 1)
    assert E.NATIVE_MIN_ROWS <= big.shape[0] < E.NATIVE_MIN_ROWS + R
    e = m.embed(big)
    assert not e.requires_grad and same_bits(e[:R].cpu().numpy(), native("rows33")) and torch.equal(e[-R:], e[:R])
    with torch.no_grad():
        assert torch.equal(m.embed(x), m(x))
    assert same_bits(GF.encode(m.packed_weights(), x, hidden=H, layers=L, dim=D).cpu().numpy(), native("rows33"))
    assert m.packed_weights() is m.packed_weights()                            # cached
    check_gate("embed(normalize=False)", m.embed(x, native=True, normalize=False).cpu().numpy(), c["raw"], c["err_ref_raw"])
    check_gate("embed(float64 mels)", m.embed(x.double(), native=True).cpu().numpy(), c["ref"], c["err_ref"])
    check_gate("embed(native=False)", m.embed(x, native=False).cpu().numpy(), c["ref"], c["err_ref"])
    # an in-place parameter update (an optimiser step): the weights are packed again
    before = m.packed_weights()
    with torch.no_grad():
        m.projection.weight.mul_(-1.0)
        m.LSTM_stack.bias_ih_l0.add_(0.25)
    ps = [p.copy() for p in c["params"]]
    ps[-2] *= -1.0
    ps[2] += np.float32(0.25)
    e2 = m.embed(x, native=True).cpu().numpy()
    assert m.packed_weights() is not before and not same_bits(e2, native("rows33"))
    ref = enc.encode_ref(ps, c["x"].astype(np.float64))
    check_gate("embed after the update", e2, ref, enc.rel_err(enc.torch_encode(ps, c["x"], torch.float32), ref))
    # load_state_dict repacks too
    m.load_state_dict(module_with(c["params"], c["shape"]).state_dict())
    assert same_bits(m.embed(x, native=True).cpu().numpy(), native("rows33"))


def test_module_embed_without_a_kernel(GF):
    shape = (6, 4, 12, 64, 2, 16)
    ps = enc.random_params(12, 64, 2, 16, seed=7)
    m = module_with(ps, shape)
    x = torch.as_tensor(np.random.default_rng(8).uniform(0, 0.96, shape[:3]).astype(np.float32)).to(dev())
    assert not GF.encode_supported(12, 64, 2, 16) and GF.encode_supported(12, 128, 2, 16) and not m.native_supported()
    with pytest.raises(RuntimeError):
        m.embed(x, native=True)
    with torch.no_grad():
        want = m(x)
    got = m.embed(x)
    assert not got.requires_grad and torch.equal(got, want)
    with pytest.raises(RuntimeError):
        m.embed_utterances([x[0].repeat(50, 1)])
    with pytest.raises(ValueError):
        GF.encode(torch.zeros(16, device=dev()), x, hidden=64, layers=2, dim=16)


def test_embed_utterances(GF):
    n_mels, H, L, D = 40, 128, 2, 64
    window, hop = 32, 16
    ps = enc.random_params(n_mels, H, L, D, seed=11)
    m = module_with(ps, (0, 0, n_mels, H, L, D))
    rng = np.random.default_rng(12)
    mels = [rng.uniform(0, 0.96, (F, n_mels)) for F in (32, 75, 130)]         # 1, 3 and 7 windows; float64 as on disk
    got = m.embed_utterances([torch.as_tensor(s) for s in mels], window=window, hop=hop).cpu().numpy()
    assert got.shape == (3, D)
    want, lib32 = [], []
    for s in mels:
        s32 = s.astype(np.float32)
        wins = np.stack([s32[i:i + window] for i in range(0, s.shape[0] - window + 1, hop)])
        for acc, e in ((want, enc.encode_ref(ps, wins.astype(np.float64))), (lib32, enc.torch_encode(ps, wins, torch.float32))):
            mean = e.mean(axis=0)
            acc.append(mean / np.linalg.norm(mean))
    assert [len(range(0, s.shape[0] - window + 1, hop)) for s in mels] == [1, 3, 7]
    check_gate("embed_utterances", got, np.stack(want), enc.rel_err(np.stack(lib32), np.stack(want)))
    with pytest.raises(ValueError):
        m.embed_utterances([torch.as_tensor(mels[1]), torch.as_tensor(mels[0][:31])], window=window, hop=hop)


def test_encode_is_captured_in_a_graph(GF):
    c = case("rows33")
    R, T, n_mels, H, L, D = c["shape"]
    packed = packed_for("rows33")
    x = torch.as_tensor(c["x"]).to(dev())
    x2 = torch.flip(x, dims=(0,)) * 0.5
    eager = [GF.encode(packed, t, hidden=H, layers=L, dim=D).clone() for t in (x, x2)]
    torch.cuda.synchronize()
    static_x = x.clone()
    static_out = torch.full((R, D), float("nan"), device=dev())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        GF.encode(packed, static_x, hidden=H, layers=L, dim=D, out=static_out)
    for t, want in zip((x, x2), eager):
        static_out.fill_(float("nan"))
        static_x.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
    assert same_bits(eager[0].cpu().numpy(), native("rows33"))
