"""CPU: the host side of the labelled ragged loss -- ge2e_label_index / ge2e_label_index_workspace_bytes /
ge2e_loss_fwd_bwd_labeled / ge2e_workspace_bytes_labeled and functional.dense_labels: declared, exported and bound, a sane
workspace size, every error code and the order of the checks, the handling of host labels -- all before anything is
launched."""
import ctypes
import re

import numpy as np
import pytest
import torch

from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_label_index_workspace_bytes", "ge2e_label_index", "ge2e_workspace_bytes_labeled", "ge2e_loss_fwd_bwd_labeled")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_VARIANT, ERR_ALIGN = -1, -2, -3, -4, -6
GRID = 512           # the ragged kernel's grid cap: one workspace slice per workgroup


def test_header_library_and_binding_have_the_four_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    # additions only: the ABI version every existing caller checks does not move
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text
    res, args = _lib.PROTOTYPES["ge2e_loss_fwd_bwd_labeled"]
    assert (res, args) == _lib.PROTOTYPES["ge2e_loss_fwd_bwd_ragged"]        # labels stand where the offsets stood
    assert _lib.PROTOTYPES["ge2e_workspace_bytes_labeled"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert _lib.PROTOTYPES["ge2e_label_index_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    res, args = _lib.PROTOTYPES["ge2e_label_index"]
    assert res is ctypes.c_int and len(args) == 9 and args[1:4] == [ctypes.c_int] * 3 and args[7] is ctypes.c_size_t


def test_workspace_bytes_labeled(lib):
    f, ragged = lib.ge2e_workspace_bytes_labeled, lib.ge2e_workspace_bytes_ragged
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
                # the ragged workspace, and offsets [B][N+1] and order [B][R] for every batch
                assert cur >= ragged(*shape, variant) + 4 * B * (N + 1 + R), (shape, cur)
                prev = cur
    # monotone in B up to the grid cap (and beyond it: the two tables keep growing with B, the slices do not)
    prev = 0
    for B in (1, 2, 3, 64, 511, GRID, GRID + 1, 5000):
        cur = f(B, 7, 40, 36, 0)
        assert cur > prev and cur >= ragged(B, 7, 40, 36, 0) + 4 * B * (7 + 1 + 40), (B, cur, prev)
        prev = cur
    # more speakers than the index kernel keeps in LDS: its counters are part of the workspace, one slice per workgroup
    for B in (1, 3, GRID + 3):
        extra = lib.ge2e_label_index_workspace_bytes(B, 1100, 2200)
        assert extra >= 4 * min(B, GRID) * 1100 and extra % 256 == 0
        assert f(B, 1100, 2200, 4, 0) >= ragged(B, 1100, 2200, 4, 0) + 4 * B * (1100 + 1 + 2200) + extra
    assert lib.ge2e_label_index_workspace_bytes(3, 67, 300) % 256 == 0       # may be 0
    assert f(1, 1, 2, 1, 0) > 0                                   # the smallest legal shape
    assert f(1, 4, 7, 8, 0) == 0 and f(1, 4, 8, 8, 0) > 0         # R < 2 N
    for bad in ((0, 4, 20, 8), (1, 0, 20, 8), (1, 4, 20, 0), (1, 4, 0, 8), (-1, 4, 20, 8), (1, 4, -20, 8)):
        assert f(*bad, 0) == 0, bad
    for bad in ((0, 4, 20), (1, 0, 20), (1, 4, 0), (-1, 4, 20)):
        assert lib.ge2e_label_index_workspace_bytes(*bad) == 0, bad


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_loss_fwd_bwd_labeled
    big = 1 << 40
    ok = dict(E=16, labels=16, B=1, N=4, R=20, D=8, w=16, b=16, eps_cos=1e-8, eps=1e-6, variant=0, loss=16, per=None, dE=None,
              dw=None, db=None, ws=256, ws_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    assert call(E=None) == ERR_NULL and call(labels=None) == ERR_NULL
    assert call(loss=None) == ERR_NULL
    assert call(w=None) == ERR_NULL and call(b=None) == ERR_NULL
    assert call(dE=32) == ERR_NULL and call(dE=32, dw=16) == ERR_NULL and call(dE=32, db=16) == ERR_NULL
    assert call(R=7) == ERR_SHAPE                                # fewer than two rows per speaker
    assert call(B=0) == ERR_SHAPE and call(N=0) == ERR_SHAPE and call(D=0) == ERR_SHAPE and call(R=0) == ERR_SHAPE
    assert call(variant=7) == ERR_VARIANT and call(variant=-1) == ERR_VARIANT
    need = lib.ge2e_workspace_bytes_labeled(1, 4, 20, 8, 0)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE             # short
    assert call(ws_bytes=lib.ge2e_workspace_bytes_ragged(1, 4, 20, 8, 0)) == ERR_WORKSPACE      # the ragged entry's size
    assert call(ws=None, ws_bytes=0) == ERR_WORKSPACE           # missing
    assert call(ws=264) == ERR_WORKSPACE                         # not 256-byte aligned
    assert call(E=24) == ERR_ALIGN
    assert call(dE=40, dw=16, db=16) == ERR_ALIGN
    # the order of the checks is the ragged entry's: NULL, shape, variant, workspace, alignment
    assert call(labels=None, R=7) == ERR_NULL and call(R=7, variant=7) == ERR_SHAPE
    assert call(variant=7, ws=None) == ERR_VARIANT and call(ws=None, E=24) == ERR_WORKSPACE

    g = lib.ge2e_label_index
    oki = dict(labels=16, B=1, N=1100, R=2200, offsets=16, order=16, ws=256, ws_bytes=big, stream=None)

    def calli(**kw):
        a = dict(oki, **kw)
        return g(*[a[k] for k in oki])

    assert calli(labels=None) == ERR_NULL and calli(offsets=None) == ERR_NULL and calli(order=None) == ERR_NULL
    assert calli(B=0) == ERR_SHAPE and calli(N=0) == ERR_SHAPE and calli(R=0) == ERR_SHAPE
    needi = lib.ge2e_label_index_workspace_bytes(1, 1100, 2200)
    assert needi > 0
    assert calli(ws_bytes=needi - 1) == ERR_WORKSPACE and calli(ws=None, ws_bytes=0) == ERR_WORKSPACE
    assert calli(ws=264) == ERR_WORKSPACE
    assert calli(order=None, N=0) == ERR_NULL and calli(N=0, ws=None) == ERR_SHAPE


def test_host_labels():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    ids, n = GF.dense_labels([7, 7, -3, 42, -3, 42, 42])
    assert ids.dtype == torch.int32 and not ids.is_cuda and ids.tolist() == [1, 1, 0, 2, 0, 2, 2] and n == 3
    # every batch by its own ascending ids
    ids, n = GF.dense_labels(torch.tensor([[500, 500, -9, -9, 3, 3], [1, 0, 2, 2, 0, 1]]))
    assert ids.tolist() == [[2, 2, 0, 0, 1, 1], [1, 0, 2, 2, 0, 1]] and n == 3
    ids, n = GF.dense_labels(np.array([5, 5, 5], dtype=np.int16))
    assert ids.tolist() == [0, 0, 0] and n == 1
    big = 2 ** 40
    assert GF.dense_labels([big, -big, big, -big])[0].tolist() == [1, 0, 1, 0]
    # dense ids are what numpy says
    rng = np.random.default_rng(5)
    raw = np.repeat(rng.choice(10 ** 6, size=37, replace=False) - 5 * 10 ** 5, 3)
    rng.shuffle(raw)
    ids, n = GF.dense_labels(raw)
    uniq, inv = np.unique(raw, return_inverse=True)
    assert n == 37 and np.array_equal(ids.numpy(), inv)
    with pytest.raises(ValueError, match=r"speaker 42\b.*at least 2"):
        GF.dense_labels([7, 7, 42, -3, -3])
    with pytest.raises(ValueError, match=r"speaker -3 of batch 1"):
        GF.dense_labels([[7, 7, 8, 8], [7, 7, 7, -3]])
    with pytest.raises(ValueError, match="same number of distinct speakers"):
        GF.dense_labels([[1, 1, 2, 2], [1, 1, 1, 1]])
    with pytest.raises(ValueError, match="integers"):
        GF.dense_labels([1.0, 1.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="integers"):
        GF.dense_labels(torch.tensor([True, True]))
    with pytest.raises(ValueError):
        GF.dense_labels([])
    with pytest.raises(ValueError):
        GF.dense_labels(torch.zeros(2, 2, 2, dtype=torch.int64))


def test_device_labels_need_num_speakers():
    """As far as a machine without a GPU can say: the check comes before anything touches the device (a tensor on the
    `meta` device stands in for one that is not on the host)."""
    from speaker_embedding_ge2e_loss_amd import functional as GF
    lab = torch.zeros(8, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="num_speakers"):
        GF._labels_on_device(lab, None, 1, 8, torch.device("meta"))
    with pytest.raises(TypeError, match="int32 or torch.int64"):
        GF._labels_on_device(lab.to(torch.float32), 2, 1, 8, torch.device("meta"))
    with pytest.raises(RuntimeError, match="one device"):
        GF._labels_on_device(lab, 2, 1, 8, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="rows"):
        GF._labels_on_device(lab, 5, 1, 8, torch.device("meta"))
    # host labels of another length than the rows; the module refuses labels together with counts
    with pytest.raises(ValueError, match=r"\(R,\) or \(B, R\)"):
        GF._labels_on_device([4, 4, 9, 9], None, 1, 6, torch.device("cpu"))
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    with pytest.raises(ValueError, match="not both"):
        GE2ELoss(HParams("cpu"))(torch.zeros(4, 2), counts=[2, 2], labels=[0, 0, 1, 1])
    with pytest.raises(ValueError, match='impl="auto"'):
        GE2ELoss(HParams("cpu"), impl="generic")(torch.zeros(4, 2), labels=[0, 0, 1, 1])
