"""CPU: the host side of the native encoder -- ge2e_encoder_packed_bytes / ge2e_encoder_pack / ge2e_encode /
ge2e_encode_plan: declared, exported and bound, the packed size, every error code and the order of the checks, the plan --
and tests/encoder_ref.py, the float64 reference of the GPU tests, held to torch's own modules in float64 and to the
reference encoder's float64 output in tests/golden/callers/encoder.npz."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import encoder_ref as enc
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_encoder_packed_bytes", "ge2e_encoder_pack", "ge2e_encode", "ge2e_encode_plan")
ERR_NULL, ERR_SHAPE, ERR_IMPL, ERR_ALIGN = -1, -2, -5, -6
I, P = ctypes.c_int, ctypes.c_void_p
GOLD = os.path.join(os.path.dirname(__file__), "golden", "callers")


def fixture_params():
    w = np.load(os.path.join(GOLD, "encoder_weights.npz"))
    z = np.load(os.path.join(GOLD, "encoder.npz"))
    L = int(z["cfg"][2])
    ps = [w[f"LSTM_stack.{n}_l{l}"] for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return ps + [w["projection.weight"], w["projection.bias"]], z


@pytest.mark.parametrize("shape", [(3, 1, 5, 4, 1, 3), (4, 7, 6, 8, 2, 5), (2, 5, 3, 8, 3, 4)])
def test_encoder_ref_is_torchs_lstm_and_linear_in_float64(shape):
    R, T, n_mels, H, L, D = shape
    ps = enc.random_params(n_mels, H, L, D, seed=sum(shape), scale=2.0)
    x = np.random.default_rng(1).standard_normal((R, T, n_mels))
    for normalize in (True, False):
        got, want = enc.encode_ref(ps, x, normalize), enc.torch_encode(ps, x, torch.float64, normalize)
        assert np.abs(got - want).max() <= 1e-12, (shape, normalize)


def test_encoder_ref_reproduces_the_reference_encoders_float64_output():
    ps, z = fixture_params()
    n_mels, H, L, D = (int(v) for v in z["cfg"][:4])
    assert ps[0].shape == (4 * H, n_mels) and ps[-2].shape == (D, H) and len(ps) == 4 * L + 2
    assert z["mels"].dtype == np.float64 and 0.0 <= z["mels"].min() and z["mels"].max() < 0.96
    assert any(np.abs(p).max() > 0 for p in ps[2::4])                      # the biases are not the zeros s2:18-22 leaves
    # the reference's forward casts the mels to float32 (s2:28); its double copy was driven on the float64 mels
    assert np.abs(enc.encode_ref(ps, z["mels"]) - z["out64"]).max() <= 1e-12
    assert enc.rel_err(z["out32"], z["out64"]) < 1e-6


def test_sigmoid_is_finite_and_right_far_out():
    z = np.array([-1000.0, -100.0, 0.0, 100.0, 1000.0])
    s = enc.sigmoid(z)
    assert s[0] == 0.0 and 0 < s[1] < 1e-43 and s[2] == 0.5 and s[3] == 1.0 and s[4] == 1.0


def test_a_zero_projection_is_nan_when_normalised():
    ps = enc.random_params(4, 8, 1, 3, seed=2)
    ps[-2][:] = 0
    ps[-1][:] = 0
    x = np.ones((2, 3, 4))
    assert np.isnan(enc.encode_ref(ps, x)).all() and not enc.encode_ref(ps, x, normalize=False).any()


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_encoder_packed_bytes"] == (ctypes.c_size_t, [I] * 4)
    assert _lib.PROTOTYPES["ge2e_encoder_pack"] == (I, [P, I, I, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_encode"] == (I, [P, P, P, I, I, I, I, I, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_encode_plan"] == (I, [I] * 6 + [ctypes.c_char_p, ctypes.c_size_t])
    atoms = _lib.plan_atoms()
    assert len(atoms) == 94 and not any(a.startswith("encode") for a in atoms)


def pad16(n):
    return (n + 15) // 16 * 16


def test_packed_bytes(lib):
    f = lib.ge2e_encoder_packed_bytes
    for n_mels, H, L, D in ((80, 256, 3, 256), (80, 128, 2, 64), (1, 128, 1, 1), (13, 128, 4, 37), (256, 256, 4, 256)):
        want = (pad16(n_mels) + H) * 4 * H + 4 * H + (L - 1) * (2 * H * 4 * H + 4 * H) + H * pad16(D) + pad16(D)
        assert f(n_mels, H, L, D) == 4 * want, (n_mels, H, L, D)
        assert f(n_mels, H, L, D) % 64 == 0
    for bad in ((80, 64, 3, 256), (80, 512, 3, 256), (80, 192, 1, 8), (80, 256, 0, 256), (80, 256, 5, 256), (0, 256, 3, 256),
                (257, 256, 3, 256), (80, 256, 3, 0), (80, 256, 3, 257), (-80, 256, 3, 256), (80, -256, 3, 256)):
        assert f(*bad) == 0, bad


def test_pack_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_encoder_pack
    ok = dict(flat=16, n_mels=80, H=256, L=3, D=256, packed=32, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("flat", "packed"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("n_mels", "L", "D"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    for kw in (dict(H=64), dict(H=0), dict(H=257), dict(L=5), dict(n_mels=257), dict(D=257)):
        assert call(**kw) == ERR_IMPL, kw
    assert call(packed=40) == ERR_ALIGN and call(packed=36) == ERR_ALIGN
    assert call(flat=20, packed=40) == ERR_ALIGN             # (flat_params is read four bytes at a time: only packed counts)
    # the order: NULL, shape, implementation, alignment
    assert call(packed=None, L=0) == ERR_NULL and call(flat=None, H=64, packed=40) == ERR_NULL
    assert call(D=0, H=64) == ERR_SHAPE and call(n_mels=0, packed=40) == ERR_SHAPE
    assert call(H=64, packed=40) == ERR_IMPL and call(L=5, packed=36) == ERR_IMPL


def test_encode_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_encode
    ok = dict(packed=16, mel=32, row_start=None, R=40, T=160, n_mels=80, H=256, L=3, D=256, normalize=1, out=48, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("packed", "mel", "out"):
        assert call(**{k: None}) == ERR_NULL, k
    for k in ("R", "T", "n_mels", "D", "L"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -3}) == ERR_SHAPE, k
    for kw in (dict(H=64), dict(H=0), dict(H=-256), dict(H=192), dict(H=512), dict(L=5), dict(n_mels=257), dict(D=257)):
        assert call(**kw) == ERR_IMPL, kw
    for k in ("packed", "mel", "out"):
        assert call(**{k: 24}) == ERR_ALIGN and call(**{k: 20}) == ERR_ALIGN, k
    # the order: NULL, shape, implementation, alignment
    assert call(out=None, R=0) == ERR_NULL and call(mel=None, H=64) == ERR_NULL and call(packed=None, out=24) == ERR_NULL
    assert call(T=0, H=64) == ERR_SHAPE and call(L=0, mel=24) == ERR_SHAPE and call(R=-1, L=5, out=20) == ERR_SHAPE
    assert call(H=128 + 1, out=24) == ERR_IMPL and call(D=300, packed=24) == ERR_IMPL


def test_encode_plan_names_the_instantiation_and_the_grid(lib):
    assert _lib.encode_plan(8192, 160, 80, 256, 3, 256) == ["encode<256>/256"]
    assert _lib.encode_plan(640, 160, 80, 256, 3, 256) == ["encode<256>/20"]
    assert _lib.encode_plan(33, 2, 40, 128, 2, 64) == ["encode<128>/2"]
    assert _lib.encode_plan(32, 2, 40, 128, 2, 64) == ["encode<128>/1"]
    assert _lib.encode_plan(1, 1, 12, 128, 1, 16) == ["encode<128>/1"]
    assert lib.ge2e_encode_plan(8192, 160, 80, 256, 3, 256, None, 0) == len("encode<256>/256")   # measures
    assert lib.ge2e_encode_plan(0, 160, 80, 256, 3, 256, None, 0) == ERR_SHAPE
    assert lib.ge2e_encode_plan(4, 160, 80, 64, 3, 256, None, 0) == ERR_IMPL
    assert lib.ge2e_encode_plan(4, 0, 80, 64, 3, 256, None, 0) == ERR_SHAPE                      # shape before implementation
    with pytest.raises(ValueError):
        _lib.encode_plan(4, 160, 80, 64, 3, 256)
