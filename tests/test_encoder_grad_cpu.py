"""CPU: tests/encoder_grad_ref.py, the float64 reference of the encoder's backward, held to torch's float64 autograd; and
the host side of the training entry points -- ge2e_encoder_packed_bwd_bytes / ge2e_encoder_pack_bwd /
ge2e_encode_train_tape_bytes / ge2e_encode_train / ge2e_encode_bwd_workspace_bytes / ge2e_encode_bwd and the two plans:
declared, exported and bound, the sizes against their formulas, every error code and the order of the checks, the plan
strings.  Nothing here launches: every refused call returns before the GPU is looked at."""
import ctypes
import re

import numpy as np
import pytest
import torch

import encoder_grad_ref as gref
import encoder_ref as enc
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_encoder_packed_bwd_bytes", "ge2e_encoder_pack_bwd", "ge2e_encode_train_tape_bytes", "ge2e_encode_train",
        "ge2e_encode_bwd_workspace_bytes", "ge2e_encode_bwd", "ge2e_encode_train_plan", "ge2e_encode_bwd_plan")
ERR_NULL, ERR_SHAPE, ERR_IMPL, ERR_ALIGN = -1, -2, -5, -6
I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


@pytest.mark.parametrize("shape", [(3, 1, 5, 4, 1, 3), (4, 7, 6, 8, 2, 5), (2, 5, 3, 8, 3, 4), (3, 4, 2, 4, 4, 1)])
@pytest.mark.parametrize("normalize", [True, False])
def test_grad_ref_is_torchs_float64_autograd(shape, normalize):
    R, T, n_mels, H, L, D = shape                 # (D = 1 normalised: both sides are rounding noise around zero)
    ps = enc.random_params(n_mels, H, L, D, seed=sum(shape), scale=2.0)
    rng = np.random.default_rng(7)
    x, g = rng.standard_normal((R, T, n_mels)), rng.standard_normal((R, D))
    got, want = gref.encode_grads(ps, x, g, normalize), gref.torch_grads(ps, x, g, torch.float64, normalize)
    assert len(got) == len(want) == 4 * L + 2
    for name, a, b in zip(gref.names(ps), got, want):
        assert a.shape == b.shape, name
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (shape, normalize, name)


def test_grad_ref_edges():
    # T = 1: no recurrence, every weight_hh gradient is exactly zero
    ps = enc.random_params(5, 8, 3, 4, seed=11)
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((3, 1, 5)), rng.standard_normal((3, 4))
    grads, dzs = gref.encode_grads(ps, x, g, with_dz=True)
    assert all(not grads[4 * l + 1].any() for l in range(3)) and all(grads[4 * l].any() for l in range(3))
    assert all(dz.shape == (3, 1, 32) for dz in dzs)
    # D = 1 normalised: y / |y| is a sign, its gradient zero everywhere
    ps = enc.random_params(5, 8, 2, 1, seed=12)
    x, g = rng.standard_normal((3, 4, 5)), rng.standard_normal((3, 1))
    assert all(np.abs(a).max() <= 1e-15 for a in gref.encode_grads(ps, x, g))
    assert any(np.abs(a).max() > 1e-3 for a in gref.encode_grads(ps, x, g, normalize=False))
    # a row with a zero upstream gradient has zero dz
    ps = enc.random_params(5, 8, 2, 4, seed=13)
    x, g = rng.standard_normal((4, 3, 5)), rng.standard_normal((4, 4))
    g[2] = 0
    _, dzs = gref.encode_grads(ps, x, g, with_dz=True)
    assert all(not dz[2].any() and dz[1].any() for dz in dzs)
    # split_flat inverts encoder_ref.flat
    back = gref.split_flat(enc.flat(ps), ps)
    assert all(np.array_equal(a, b) for a, b in zip(back, ps))


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["ge2e_encoder_packed_bwd_bytes"] == (Z, [I] * 4)
    assert _lib.PROTOTYPES["ge2e_encoder_pack_bwd"] == (I, [P, I, I, I, I, P, P])
    assert _lib.PROTOTYPES["ge2e_encode_train_tape_bytes"] == (Z, [I] * 6)
    assert _lib.PROTOTYPES["ge2e_encode_train"] == (I, [P, P, P, I, I, I, I, I, I, I, P, P, P])
    assert _lib.PROTOTYPES["ge2e_encode_bwd_workspace_bytes"] == (Z, [I] * 6)
    assert _lib.PROTOTYPES["ge2e_encode_bwd"] == (I, [P, P, P, I, I, I, I, I, I, I, P, P, P, P, P])
    for s in ("ge2e_encode_train_plan", "ge2e_encode_bwd_plan"):
        assert _lib.PROTOTYPES[s] == (I, [I] * 6 + [ctypes.c_char_p, Z])
    assert not any(a.startswith("encode") for a in _lib.plan_atoms())


def pad16(n):
    return (n + 15) // 16 * 16


def round64(n):
    return (n + 63) // 64 * 64


def slices(K):
    s = min((K + 511) // 512, 32)
    length = ((K + s - 1) // s + 3) // 4 * 4
    return (K + length - 1) // length


def flat_numel(n_mels, H, L, D):
    return 4 * H * (n_mels + H + 2) + (L - 1) * 4 * H * (2 * H + 2) + D * H + D


SHAPES = ((8192, 160, 80, 256, 3, 256), (33, 2, 40, 128, 2, 64), (1, 1, 1, 128, 1, 1), (17, 5, 20, 256, 4, 24),
          (73, 7, 13, 128, 1, 37))
BAD = ((4, 5, 80, 64, 3, 256), (4, 5, 80, 192, 1, 8), (4, 5, 80, 256, 5, 256), (4, 5, 257, 256, 3, 256),
       (4, 5, 80, 256, 3, 257), (0, 5, 80, 256, 3, 256), (4, 0, 80, 256, 3, 256), (4, 5, 80, 256, 0, 256))


def test_size_queries_match_their_formulas(lib):
    for R, T, n_mels, H, L, D in SHAPES:
        assert lib.ge2e_encode_train_tape_bytes(R, T, n_mels, H, L, D) == 4 * (6 * L * T * R * H + R * D)
        assert lib.ge2e_encoder_packed_bwd_bytes(n_mels, H, L, D) == 4 * (4 * H * H + (L - 1) * 4 * H * 2 * H + pad16(D) * H)
        want = round64(L * T * R * 4 * H) + round64(R * D) + slices(R * T) * round64(flat_numel(n_mels, H, L, D))
        assert lib.ge2e_encode_bwd_workspace_bytes(R, T, n_mels, H, L, D) == 4 * want, (R, T, n_mels, H, L, D)
    # the slice length: 512 pairs up to 32 slices, equal parts of a multiple of 4 beyond
    assert [slices(K) for K in (1, 511, 512, 513, 1024, 1025, 16384, 16385, 8192 * 160)] == [1, 1, 1, 2, 2, 3, 32, 32, 32]
    for bad in BAD:
        assert lib.ge2e_encode_train_tape_bytes(*bad) == 0 and lib.ge2e_encode_bwd_workspace_bytes(*bad) == 0, bad
    for bad in ((80, 64, 3, 256), (80, 256, 0, 256), (80, 256, 5, 256), (0, 256, 3, 256), (80, 256, 3, 257)):
        assert lib.ge2e_encoder_packed_bwd_bytes(*bad) == 0, bad


def test_pack_bwd_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_encoder_pack_bwd
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
    assert call(packed=40) == ERR_ALIGN and call(flat=20, packed=36) == ERR_ALIGN
    assert call(packed=None, L=0) == ERR_NULL and call(D=0, H=64) == ERR_SHAPE and call(H=64, packed=40) == ERR_IMPL


def check_order(f, ok, pointers, dims):
    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in pointers:
        assert call(**{k: None}) == ERR_NULL, k
    for k in dims:
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -3}) == ERR_SHAPE, k
    for kw in (dict(H=64), dict(H=0), dict(H=-256), dict(H=192), dict(H=512), dict(L=5), dict(n_mels=257), dict(D=257)):
        assert call(**kw) == ERR_IMPL, kw
    for k in pointers:
        assert call(**{k: 24}) == ERR_ALIGN and call(**{k: 20}) == ERR_ALIGN, k
    # the order: NULL, shape, implementation, alignment
    first, last = pointers[0], pointers[-1]
    assert call(**{last: None}, R=0) == ERR_NULL and call(**{first: None}, H=64) == ERR_NULL
    assert call(**{first: None, last: 24}) == ERR_NULL
    assert call(T=0, H=64) == ERR_SHAPE and call(L=0, **{first: 24}) == ERR_SHAPE and call(R=-1, L=5, **{last: 20}) == ERR_SHAPE
    assert call(H=129, **{last: 24}) == ERR_IMPL and call(D=300, **{first: 24}) == ERR_IMPL


def test_encode_train_argument_validation_returns_codes_without_gpu(lib):
    ok = dict(packed=16, mel=32, row_start=None, R=40, T=160, n_mels=80, H=256, L=3, D=256, normalize=1, out=48, tape=64,
              stream=None)
    check_order(lib.ge2e_encode_train, ok, ("packed", "mel", "out", "tape"), ("R", "T", "n_mels", "D", "L"))


def test_encode_bwd_argument_validation_returns_codes_without_gpu(lib):
    ok = dict(packed_bwd=16, mel=32, row_start=None, R=40, T=160, n_mels=80, H=256, L=3, D=256, normalize=1, tape=64, d_out=48,
              d_flat=80, workspace=256, stream=None)
    check_order(lib.ge2e_encode_bwd, ok, ("packed_bwd", "mel", "tape", "d_out", "d_flat", "workspace"),
                ("R", "T", "n_mels", "D", "L"))


def test_plans_name_the_instantiations_and_the_grids(lib):
    assert _lib.encode_train_plan(8192, 160, 80, 256, 3, 256) == ["encode_train<256>/256"]
    assert _lib.encode_train_plan(33, 2, 40, 128, 2, 64) == ["encode_train<128>/2"]
    # the reference model: 512 tiles of 16 rows; layer 0 [1024][80 + 256] = 6 x 16 blocks, the others [1024][512], the
    # projection [256][256]; 32 slices of R T pairs and 16 of R
    assert _lib.encode_bwd_plan(8192, 160, 80, 256, 3, 256) == [
        "encode_bwd<256>/512", "encode_wgrad/6x16x32", "encode_wgrad/8x16x32", "encode_wgrad/8x16x32", "encode_wgrad/4x4x16",
        "encode_reduce/4096"]
    assert _lib.encode_bwd_plan(33, 2, 40, 128, 2, 64) == [
        "encode_bwd<128>/3", "encode_wgrad/3x8x1", "encode_wgrad/4x8x1", "encode_wgrad/2x1x1", "encode_reduce/889"]
    assert _lib.encode_bwd_plan(16, 33, 1, 128, 1, 1)[:3] == ["encode_bwd<128>/1", "encode_wgrad/3x8x2", "encode_wgrad/2x1x1"]
    n = len("encode_bwd<128>/1,encode_wgrad/3x8x2,encode_wgrad/2x1x1,encode_reduce/263")
    assert lib.ge2e_encode_bwd_plan(16, 33, 1, 128, 1, 1, None, 0) == n                           # measures
    for plan in (lib.ge2e_encode_train_plan, lib.ge2e_encode_bwd_plan):
        assert plan(0, 160, 80, 256, 3, 256, None, 0) == ERR_SHAPE
        assert plan(4, 160, 80, 64, 3, 256, None, 0) == ERR_IMPL
        assert plan(4, 0, 80, 64, 3, 256, None, 0) == ERR_SHAPE                                   # shape before implementation
    with pytest.raises(ValueError):
        _lib.encode_bwd_plan(4, 160, 80, 64, 3, 256)
