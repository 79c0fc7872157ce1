"""CPU: the ragged loss's reference helper (tests/ragged_ref.py) against the dense oracle, and the host side of
ge2e_loss_fwd_bwd_ragged / ge2e_workspace_bytes_ragged / functional.ragged_offsets: declared, exported and bound, a sane
workspace size, every error code and the order of the checks -- all before anything is launched."""
import ctypes
import re

import numpy as np
import pytest
import torch

from capi import built_lib as lib  # noqa: F401
from capi import header_text
import ragged_ref as rr
from oracle import ge2e_oracle as orc
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_workspace_bytes_ragged", "ge2e_loss_fwd_bwd_ragged")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_VARIANT, ERR_ALIGN = -1, -2, -3, -4, -6


# (contrast with one speaker has no other speaker to take the max over: the definition -- and every kernel -- says 0 for
# that term, numpy's argmax over an all-masked row in the closed form says column 0, so that pair is not a common ground)
DENSE = [(s, v) for s in ((4, 5, 16), (7, 3, 36), (1, 3, 8), (5, 2, 1)) for v in ("softmax", "contrast")
         if not (s[0] == 1 and v == "contrast")]


@pytest.mark.parametrize("shape,variant", DENSE, ids=lambda x: x if isinstance(x, str) else "x".join(map(str, x)))
def test_reference_helper_is_the_dense_loss_at_equal_counts(shape, variant):
    """Two independent fp64 formulations (per-speaker slices + autograd here, the matmul closed form there) of the same
    function: they agree to rounding (measured: loss 6e-16, dE 1e-15, dw and db 2e-16 relative), held to 1e-12."""
    N, M, D = shape
    E = rr.ragged_inputs([M] * N, D, seed=N * 100 + M * 10 + D)
    for w, b in ((10.0, -5.0), (-3.0, 0.5)):
        ref = orc.closed_form(E.reshape(N, M, D), w, b, variant=variant)
        got = rr.ragged_loss(E, [M] * N, w, b, variant=variant)
        rows = N * M
        assert abs(got["loss"] - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
        assert np.abs(got["per"] - ref["per"].reshape(rows)).max() <= 1e-12 * max(1.0, np.abs(ref["per"]).max())
        assert np.abs(got["dE"] - ref["dE"].reshape(rows, D)).max() <= 1e-12 * max(1.0, np.abs(ref["dE"]).max())
        assert abs(got["dw"] - ref["dw"]) <= 1e-12 * rows and abs(got["db"] - ref["db"]) <= 1e-12 * rows


def test_header_library_and_binding_have_both_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    # additions only: the ABI version every existing caller checks does not move
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text
    res, args = _lib.PROTOTYPES["ge2e_loss_fwd_bwd_ragged"]
    assert res is ctypes.c_int and args.count(ctypes.c_float) == 2 and ctypes.c_double not in args and len(args) == 19
    res, args = _lib.PROTOTYPES["ge2e_workspace_bytes_ragged"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int] * 5


def test_workspace_bytes_positive_aligned_and_monotone(lib):
    f = lib.ge2e_workspace_bytes_ragged
    base = (3, 7, 2100, 36)          # B, N, R, D with R >= 2 (N + 700)
    for variant in (0, 1):
        for axis in range(4):
            prev = 0
            for step in (0, 1, 2, 5, 30, 700):
                shape = list(base)
                shape[axis] += step
                B, N, R, D = shape
                cur = f(*shape, variant)
                assert cur > 0 and cur % 256 == 0 and cur >= prev, (shape, cur, prev)
                # the kernel's own intermediates at least: four [N][D] planes and the [R][N] matrix per workgroup slice
                assert cur >= min(B, 512) * 4 * (4 * N * D + R * N), (shape, cur)
                prev = cur
    # one slice per workgroup of the grid, and the grid stops at 512
    assert f(512, 7, 40, 36, 0) == f(5000, 7, 40, 36, 0) > f(511, 7, 40, 36, 0)
    assert f(600, 4, 9, 8, 0) >= 512 * 4 * (4 * 4 * 8 + 9 * 4)
    assert f(1, 1, 2, 1, 0) > 0                                   # the smallest legal shape
    assert f(1, 4, 7, 8, 0) == 0 and f(1, 4, 8, 8, 0) > 0         # R < 2 N
    for bad in ((0, 4, 20, 8), (1, 0, 20, 8), (1, 4, 20, 0), (1, 4, 0, 8), (-1, 4, 20, 8), (1, 4, -20, 8)):
        assert f(*bad, 0) == 0, bad


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_loss_fwd_bwd_ragged
    big = 1 << 40
    ok = dict(E=16, off=16, B=1, N=4, R=20, D=8, w=16, b=16, eps_cos=1e-8, eps=1e-6, variant=0, loss=16, per=None, dE=None,
              dw=None, db=None, ws=256, ws_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    assert call(E=None) == ERR_NULL and call(off=None) == ERR_NULL
    assert call(loss=None) == ERR_NULL
    assert call(w=None) == ERR_NULL and call(b=None) == ERR_NULL
    assert call(dE=32) == ERR_NULL and call(dE=32, dw=16) == ERR_NULL and call(dE=32, db=16) == ERR_NULL
    assert call(R=7) == ERR_SHAPE                                # fewer than two rows per speaker
    assert call(B=0) == ERR_SHAPE and call(N=0) == ERR_SHAPE and call(D=0) == ERR_SHAPE and call(R=0) == ERR_SHAPE
    assert call(variant=7) == ERR_VARIANT and call(variant=-1) == ERR_VARIANT
    need = lib.ge2e_workspace_bytes_ragged(1, 4, 20, 8, 0)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE             # short
    assert call(ws=None, ws_bytes=0) == ERR_WORKSPACE           # missing
    assert call(ws=264) == ERR_WORKSPACE                         # not 256-byte aligned
    assert call(E=24) == ERR_ALIGN
    assert call(dE=40, dw=16, db=16) == ERR_ALIGN
    # the order of the checks is ge2e_loss_fwd_bwd_f64's: NULL, shape, variant, workspace, alignment
    assert call(off=None, R=7) == ERR_NULL and call(R=7, variant=7) == ERR_SHAPE
    assert call(variant=7, ws=None) == ERR_VARIANT and call(ws=None, E=24) == ERR_WORKSPACE


def test_ragged_offsets():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    off = GF.ragged_offsets([2, 17, 3, 65, 2], 89)
    assert off.dtype == torch.int32 and not off.is_cuda and off.tolist() == [0, 2, 19, 22, 87, 89]
    off = GF.ragged_offsets(torch.tensor([[2, 4], [3, 3], [4, 2]]), 6)
    assert off.dtype == torch.int32 and off.tolist() == [[0, 2, 6], [0, 3, 6], [0, 4, 6]]
    assert GF.ragged_offsets(np.array([5], dtype=np.int16), 5).tolist() == [0, 5]
    assert GF.ragged_offsets(torch.tensor([3, 2], dtype=torch.int32), 5).tolist() == [0, 3, 5]
    with pytest.raises(ValueError, match="at least 2"):
        GF.ragged_offsets([3, 1, 4], 8)
    with pytest.raises(ValueError, match="at least 2"):
        GF.ragged_offsets([[2, 2], [3, 1]], 4)
    with pytest.raises(ValueError, match="sum"):
        GF.ragged_offsets([3, 2, 4], 10)
    with pytest.raises(ValueError, match="sum"):
        GF.ragged_offsets([[2, 4], [3, 4]], 6)
    with pytest.raises(ValueError, match="N >= 1"):
        GF.ragged_offsets([], 0)
    with pytest.raises(ValueError, match="N >= 1"):
        GF.ragged_offsets(torch.zeros(2, 0, dtype=torch.int64), 0)
    with pytest.raises(TypeError):
        GF.ragged_offsets([2.5, 2.5], 5)
