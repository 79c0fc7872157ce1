"""CPU: the double-precision entry point of the C ABI (ge2e_loss_fwd_bwd_f64 / ge2e_workspace_bytes_f64) is declared,
exported and bound, sizes its workspace sanely and rejects bad arguments on the host, before anything is launched."""
import ctypes
import re


from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_workspace_bytes_f64", "ge2e_loss_fwd_bwd_f64")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_VARIANT, ERR_ALIGN = -1, -2, -3, -4, -6


def test_header_library_and_binding_have_both_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    # additions only: the ABI version every existing caller checks does not move
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text
    res, args = _lib.PROTOTYPES["ge2e_loss_fwd_bwd_f64"]
    assert res is ctypes.c_int and args.count(ctypes.c_double) == 2 and ctypes.c_float not in args and len(args) == 18


def test_workspace_bytes_positive_and_monotone(lib):
    f = lib.ge2e_workspace_bytes_f64
    base = (3, 7, 3, 36)
    for variant in (0, 1):
        assert f(*base, variant) > 0
        # the kernel's own intermediates at least: four [N][D] planes and the [NM][N] matrix, in doubles
        B, N, M, D = base
        assert f(*base, variant) >= B * (4 * N * D + N * M * N) * 8
        for axis in range(4):
            prev = 0
            for step in (0, 1, 2, 5, 30, 700):
                shape = list(base)
                shape[axis] += step
                cur = f(*shape, variant)
                assert cur > 0 and cur >= prev, (shape, cur, prev)
                prev = cur
    assert f(1, 1, 2, 1, 0) > 0                                  # the smallest legal shape
    assert f(1, 4, 1, 8, 0) == 0 and f(0, 4, 5, 8, 0) == 0      # bad shape -> 0, like ge2e_workspace_bytes
    assert f(1, 4, 5, 8, 0) % 256 == 0


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_loss_fwd_bwd_f64
    big = 1 << 40
    ok = dict(E=16, B=1, N=4, M=5, D=8, w=16, b=16, eps_cos=1e-8, eps=1e-6, variant=0, loss=16, per=None, dE=None,
              dw=None, db=None, ws=256, ws_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    assert call(E=None) == ERR_NULL
    assert call(loss=None) == ERR_NULL
    assert call(w=None) == ERR_NULL and call(b=None) == ERR_NULL
    assert call(dE=32) == ERR_NULL                               # dE without dw / db
    assert call(M=1) == ERR_SHAPE                                # M = 1 divides by zero in the reference (s3:110-111)
    assert call(B=0) == ERR_SHAPE and call(N=0) == ERR_SHAPE and call(D=0) == ERR_SHAPE
    assert call(variant=7) == ERR_VARIANT and call(variant=-1) == ERR_VARIANT
    need = lib.ge2e_workspace_bytes_f64(1, 4, 5, 8, 0)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE             # short
    assert call(ws=None, ws_bytes=0) == ERR_WORKSPACE           # missing
    assert call(ws=264) == ERR_WORKSPACE                         # not 256-byte aligned
    assert call(E=24) == ERR_ALIGN
    assert call(dE=40, dw=16, db=16) == ERR_ALIGN
    # the order of the checks is ge2e_loss_fwd_bwd's: NULL before shape before variant before workspace
    assert call(E=None, M=1) == ERR_NULL and call(M=1, variant=7) == ERR_SHAPE and call(variant=7, ws=None) == ERR_VARIANT
