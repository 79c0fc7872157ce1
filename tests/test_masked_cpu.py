"""CPU: the host side of the masked labelled loss -- ge2e_label_index_masked / ge2e_label_index_masked_workspace_bytes /
ge2e_loss_fwd_bwd_labeled_masked / ge2e_workspace_bytes_labeled_masked, functional.dense_labels(masked=True) and the checks
the Python layer makes before it touches a device: declared, exported and bound, a sane workspace size (slices laid out for
the speakers the rows can hold, not for the bound), every error code and the order of the checks, the handling of host
labels.  tests/masked_ref.py, the reference of the GPU tests, is held to hand-made examples here."""
import ctypes
import re

import numpy as np
import pytest
import torch

from capi import built_lib as lib  # noqa: F401
from capi import header_text
import masked_ref as mr
import ragged_ref as rr
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_label_index_masked_workspace_bytes", "ge2e_label_index_masked", "ge2e_workspace_bytes_labeled_masked",
        "ge2e_loss_fwd_bwd_labeled_masked")
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
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    # the labelled entry's arguments with `active` in front of the workspace
    res, args = _lib.PROTOTYPES["ge2e_loss_fwd_bwd_labeled_masked"]
    lres, largs = _lib.PROTOTYPES["ge2e_loss_fwd_bwd_labeled"]
    assert res is lres and args == largs[:-3] + [ctypes.c_void_p] + largs[-3:]
    assert _lib.PROTOTYPES["ge2e_workspace_bytes_labeled_masked"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert _lib.PROTOTYPES["ge2e_label_index_masked_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    res, args = _lib.PROTOTYPES["ge2e_label_index_masked"]
    assert res is ctypes.c_int and len(args) == 11 and args[1:4] == [ctypes.c_int] * 3 and args[9] is ctypes.c_size_t


def bound(lib, B, N, R, D, v):
    """What the workspace must stay below: the ragged slices for the speakers R rows can hold, the four tables, the index
    kernel's counters, and alignment."""
    NA = max(1, min(N, R // 2))
    return lib.ge2e_workspace_bytes_ragged(B, NA, max(R, 2 * NA, 2), D, v) + 4 * B * (2 * N + R + 3) + 4 * min(B, GRID) * N + 2048


def test_workspace_bytes_labeled_masked(lib):
    f = lib.ge2e_workspace_bytes_labeled_masked
    base = (3, 7, 2100, 36)
    for variant in (0, 1):
        for axis in range(4):
            prev = 0
            for step in (0, 1, 2, 5, 30, 700, 3000):
                shape = list(base)
                shape[axis] += step
                B, N, R, D = shape
                cur = f(*shape, variant)
                assert cur > 0 and cur % 256 == 0 and cur >= prev, (shape, cur, prev)
                # offsets [B][N+1], order [B][R], speakers [B][N] and active [B][2] for every batch
                assert 4 * B * (2 * N + R + 3) < cur < bound(lib, *shape, variant), (shape, cur)
                prev = cur
    prev = 0
    for B in (1, 2, 3, 64, 511, GRID, GRID + 1, 5000):
        cur = f(B, 7, 40, 36, 0)
        assert cur > prev and cur < bound(lib, B, 7, 40, 36, 0), (B, cur, prev)
        prev = cur
    # the slices are laid out for the speakers the rows can hold, not for the bound
    for shape in ((1, 5000, 64, 256), (3, 1251, 640, 256), (1, 4, 1, 1), (GRID + 3, 1100, 30, 4), (2, 1, 1, 1), (1, 3, 9, 2)):
        for variant in (0, 1):
            cur = f(*shape, variant)
            assert 0 < cur < bound(lib, *shape, variant) and cur % 256 == 0, (shape, cur)
    assert f(1, 5000, 64, 256, 0) < lib.ge2e_workspace_bytes_ragged(1, 100, 200, 256, 0)
    # more speakers than the index kernel keeps in LDS: its counters are part of the workspace, one slice per workgroup
    for B in (1, 3, GRID + 3):
        extra = lib.ge2e_label_index_masked_workspace_bytes(B, 1100, 300)
        assert extra >= 4 * min(B, GRID) * 1100 and extra % 256 == 0
        assert f(B, 1100, 300, 4, 0) >= lib.ge2e_workspace_bytes_ragged(B, 150, 300, 4, 0) + 4 * B * (2 * 1100 + 300 + 3) + extra
    assert lib.ge2e_label_index_masked_workspace_bytes(3, 67, 300) % 256 == 0       # may be 0
    assert f(1, 4, 1, 1, 0) > 0 and f(1, 1, 1, 1, 0) > 0          # legal: N is a bound, R >= 2 N is not asked for
    assert f(1, 4, 7, 8, 0) > 0
    for bad in ((0, 4, 20, 8), (1, 0, 20, 8), (1, 4, 20, 0), (1, 4, 0, 8), (-1, 4, 20, 8), (1, 4, -20, 8), (1, -4, 20, 8)):
        assert f(*bad, 0) == 0, bad
    for bad in ((0, 4, 20), (1, 0, 20), (1, 4, 0), (-1, 4, 20)):
        assert lib.ge2e_label_index_masked_workspace_bytes(*bad) == 0, bad


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_loss_fwd_bwd_labeled_masked
    big = 1 << 40
    ok = dict(E=16, labels=16, B=1, N=4, R=20, D=8, w=16, b=16, eps_cos=1e-8, eps=1e-6, variant=0, loss=16, per=None, dE=None,
              dw=None, db=None, active=None, ws=256, ws_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    assert call(E=None) == ERR_NULL and call(labels=None) == ERR_NULL
    assert call(loss=None) == ERR_NULL
    assert call(w=None) == ERR_NULL and call(b=None) == ERR_NULL
    assert call(dE=32) == ERR_NULL and call(dE=32, dw=16) == ERR_NULL and call(dE=32, db=16) == ERR_NULL
    assert call(B=0) == ERR_SHAPE and call(N=0) == ERR_SHAPE and call(D=0) == ERR_SHAPE and call(R=0) == ERR_SHAPE
    assert call(R=-3) == ERR_SHAPE
    assert call(variant=7) == ERR_VARIANT and call(variant=-1) == ERR_VARIANT
    need = lib.ge2e_workspace_bytes_labeled_masked(1, 4, 20, 8, 0)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE             # short
    assert call(ws=None, ws_bytes=0) == ERR_WORKSPACE           # missing
    assert call(ws=264) == ERR_WORKSPACE                         # not 256-byte aligned
    # R < 2 N is a legal shape: N is a bound.  (Nothing is launched here: the next check refuses the call.)
    assert call(R=7, ws_bytes=lib.ge2e_workspace_bytes_labeled_masked(1, 4, 7, 8, 0) - 1) == ERR_WORKSPACE
    assert call(R=1, N=50, ws=None) == ERR_WORKSPACE and call(R=7, E=24) == ERR_ALIGN
    assert call(E=24) == ERR_ALIGN
    assert call(dE=40, dw=16, db=16) == ERR_ALIGN
    # the order of the checks is the labelled entry's: NULL, shape, variant, workspace, alignment
    assert call(labels=None, R=0) == ERR_NULL and call(R=0, variant=7) == ERR_SHAPE
    assert call(variant=7, ws=None) == ERR_VARIANT and call(ws=None, E=24) == ERR_WORKSPACE

    g = lib.ge2e_label_index_masked
    oki = dict(labels=16, B=1, N=1100, R=300, offsets=16, order=16, speakers=16, active=16, ws=256, ws_bytes=big, stream=None)

    def calli(**kw):
        a = dict(oki, **kw)
        return g(*[a[k] for k in oki])

    for k in ("labels", "offsets", "order", "speakers", "active"):
        assert calli(**{k: None}) == ERR_NULL, k
    assert calli(B=0) == ERR_SHAPE and calli(N=0) == ERR_SHAPE and calli(R=0) == ERR_SHAPE
    needi = lib.ge2e_label_index_masked_workspace_bytes(1, 1100, 300)
    assert needi > 0
    assert calli(ws_bytes=needi - 1) == ERR_WORKSPACE and calli(ws=None, ws_bytes=0) == ERR_WORKSPACE
    assert calli(ws=264) == ERR_WORKSPACE
    assert calli(active=None, N=0) == ERR_NULL and calli(N=0, ws=None) == ERR_SHAPE


def test_host_labels_masked():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    ids, n = GF.dense_labels([7, 7, 42, -3, -3], masked=True)
    assert ids.dtype == torch.int32 and not ids.is_cuda and ids.tolist() == [0, 0, 1, -1, -1] and n == 2
    # every batch by its own ascending ids; the speaker counts may differ and N is the largest
    ids, n = GF.dense_labels(torch.tensor([[500, 500, -9, 9, 3, 3], [1, 1, 1, 1, -1, 1]]), masked=True)
    assert ids.tolist() == [[2, 2, -1, 1, 0, 0], [0, 0, 0, 0, -1, 0]] and n == 3
    ids, n = GF.dense_labels([-1, -5, -2 ** 40], masked=True)
    assert ids.tolist() == [-1, -1, -1] and n == 1                       # nothing counts: N is at least 1
    ids, n = GF.dense_labels(np.array([5, 2 ** 40, 5], dtype=np.int64), masked=True)
    assert ids.tolist() == [0, 1, 0] and n == 2
    with pytest.raises(ValueError, match="integers"):
        GF.dense_labels([1.0, 1.0, 2.0, 2.0], masked=True)
    with pytest.raises(ValueError, match="integers"):
        GF.dense_labels(torch.tensor([True, True]), masked=True)
    with pytest.raises(ValueError):
        GF.dense_labels([], masked=True)
    # a bound below the distinct count; a bound above it is the N of the call
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="num_speakers = 1 "):
        GF._labels_on_device([7, 7, 42, -3, -3], 1, 1, 5, cpu, masked=True)
    lab, n = GF._labels_on_device([7, 7, 42, -3, -3], None, 1, 5, cpu, masked=True)
    assert lab.tolist() == [[0, 0, 1, -1, -1]] and n == 2
    lab, n = GF._labels_on_device([7, 7, 42, -3, -3], 9, 1, 5, cpu, masked=True)
    assert lab.tolist() == [[0, 0, 1, -1, -1]] and n == 9
    # masked=False: results and messages as they were
    assert GF.dense_labels([7, 7, -3, 42, -3, 42, 42], masked=False)[0].tolist() == [1, 1, 0, 2, 0, 2, 2]
    with pytest.raises(ValueError, match=r"speaker 42\b has 1 row: every speaker needs at least 2 \(the leave-one-out"):
        GF.dense_labels([7, 7, 42, -3, -3])
    with pytest.raises(ValueError, match="every batch must hold the same number of distinct speakers: batch 0 has 2, batch 1 has 1"):
        GF.dense_labels([[1, 1, 2, 2], [1, 1, 1, 1]], masked=False)
    with pytest.raises(ValueError, match="num_speakers = 3, the labels hold 2 distinct speakers"):
        GF._labels_on_device([4, 4, 9, 9], 3, 1, 4, cpu)
    # the two forms of one table are cached apart
    a = GF._labels_on_device([4, 4, 9, 9], None, 1, 4, cpu)
    m = GF._labels_on_device([4, 4, 9, 9], 7, 1, 4, cpu, masked=True)
    assert a[1] == 2 and m[1] == 7 and GF._labels_on_device([4, 4, 9, 9], None, 1, 4, cpu)[1] == 2


def test_checks_before_anything_touches_the_device():
    """As far as a machine without a GPU can say (a tensor on the `meta` device stands in for one that is not on the host)."""
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    from speaker_embedding_ge2e_loss_amd import functional as GF
    meta = torch.device("meta")
    lab = torch.zeros(8, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="num_speakers"):
        GF._labels_on_device(lab, None, 1, 8, meta, masked=True)
    with pytest.raises(ValueError, match="num_speakers must be >= 1"):
        GF._labels_on_device(lab, 0, 1, 8, meta, masked=True)
    with pytest.raises(TypeError, match="int32 or torch.int64"):
        GF._labels_on_device(lab.to(torch.float32), 2, 1, 8, meta, masked=True)
    # a bound far above the rows is fine (without masking it is refused, as before)
    got, n = GF._labels_on_device(lab, 1251, 1, 8, meta, masked=True)
    assert n == 1251 and got.shape == (1, 8) and got.dtype == torch.int32
    got, n = GF._labels_on_device(lab.to(torch.int64), 1251, 1, 8, meta, masked=True)
    assert n == 1251 and got.dtype == torch.int32
    with pytest.raises(ValueError, match="rows"):
        GF._labels_on_device(lab, 1251, 1, 8, meta)
    mod = GE2ELoss(HParams("cpu"))
    e = torch.zeros(8, 4, device="meta")
    with pytest.raises(ValueError, match="labels"):
        mod(e, masked=True)
    with pytest.raises(ValueError, match="labels"):
        mod(e, counts=[4, 4], masked=True)
    with pytest.raises(ValueError, match='impl="auto"'):
        GE2ELoss(HParams("cpu"), impl="generic")(e, labels=lab, num_speakers=3, masked=True)
    with pytest.raises(NotImplementedError, match="float64"):
        mod(e.double(), labels=lab, num_speakers=3, masked=True)
    with pytest.raises(NotImplementedError, match="float64"):
        GF.ge2e_loss_labeled(e.double(), lab, mod.w, mod.b, num_speakers=3, masked=True)
    with pytest.raises(ValueError, match="return_active"):
        GF.ge2e_loss_labeled(e, lab, mod.w, mod.b, num_speakers=3, return_active=True)


def test_masked_ref_on_hand_made_batches():
    labels = np.array([0, 5, 2, 2, -1, 7, 2, 0, 9, 5, 3])
    idx = mr.index_ref(labels, 8)          # 9 is outside the bound, 7 and 3 are lone, 1, 4, 6 are absent
    assert idx["active"].tolist() == [3, 7]
    assert idx["order"].tolist() == [0, 7, 2, 3, 6, 1, 9, 4, 5, 8, 10]
    assert idx["offsets"].tolist() == [0, 2, 5, 7, 7, 7, 7, 7, 7]
    assert idx["speakers"].tolist() == [0, 2, 5, -1, -1, -1, -1, -1]
    assert idx["counts"].tolist() == [2, 3, 2]
    none = mr.index_ref([3, 4, -1, 8], 8)
    assert none["active"].tolist() == [0, 0] and none["order"].tolist() == [0, 1, 2, 3]
    assert none["offsets"].tolist() == [0] * 9 and none["speakers"].tolist() == [-1] * 8
    # the loss: the ragged reference on the rows that count, zeros elsewhere, whatever the other rows hold
    E = rr.ragged_inputs([len(labels)], 6, 3)
    ref = mr.masked_loss(E, labels, 8)
    rows = idx["order"][:7]
    want = rr.ragged_loss(E[rows], [2, 3, 2])
    assert ref["loss"] == want["loss"] and np.array_equal(ref["dE"][rows], want["dE"]) and np.array_equal(ref["per"][rows], want["per"])
    rest = idx["order"][7:]
    assert not ref["dE"][rest].any() and not ref["per"][rest].any()
    E2 = E.copy()
    E2[rest] = np.nan
    again = mr.masked_loss(E2, labels, 8)
    assert all(np.array_equal(ref[k], again[k]) for k in ("loss", "per", "dE", "dw", "db"))
    empty = mr.masked_loss(E2, [3, 4, -1, 8, 9, 9, 9, 9, 9, 9, 9], 8)
    assert empty["loss"] == 0 and not empty["dE"].any() and not empty["per"].any() and empty["dw"] == 0 and empty["db"] == 0
