"""CPU: the host side of the labelled evaluation calls -- ge2e_cos_sim_labeled_workspace_bytes / ge2e_cos_sim_labeled /
ge2e_eer_counts_labeled and evaluation.eer_from_labeled_counts: declared, exported and bound, a sane per-batch workspace
size, every error code and the order of the checks.  tests/labeled_eval_ref.py, the reference of the GPU tests, is held
to the oracle and to the committed fixtures here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from capi import built_lib as lib  # noqa: F401
from capi import header_text
import labeled_eval_ref as ler
from conftest import golden_names, load_golden
from oracle import ge2e_oracle as orc
from speaker_embedding_ge2e_loss_amd import _lib, build
from speaker_embedding_ge2e_loss_amd import evaluation as EV

SYMS = ("ge2e_cos_sim_labeled_workspace_bytes", "ge2e_cos_sim_labeled", "ge2e_eer_counts_labeled")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -6
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "callers", "eer.npz"))
EER_CASES = sorted({k.split(".")[0] for k in Z.files})


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_cos_sim_labeled_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    res, args = _lib.PROTOTYPES["ge2e_cos_sim_labeled"]
    assert res is ctypes.c_int and len(args) == 18 and args[2:6] == [ctypes.c_int] * 4 and args[9] is ctypes.c_int
    assert args[6:8] == [ctypes.c_float] * 2 and args[16] is ctypes.c_size_t
    res, args = _lib.PROTOTYPES["ge2e_eer_counts_labeled"]
    assert res is ctypes.c_int and len(args) == 10 and args[3:6] == [ctypes.c_int] * 3 and args[7] is ctypes.c_int


def bound(lib, B, N, R, D):
    NA = max(1, min(N, R // 2))
    return 4 * B * (2 * NA * D + 4 * NA + 2 * N + 3 * R + 3) + lib.ge2e_label_index_masked_workspace_bytes(B, N, R) + 4096


def test_workspace_bytes(lib):
    f = lib.ge2e_cos_sim_labeled_workspace_bytes
    base = (3, 7, 2100, 36)
    for axis in range(4):
        prev = 0
        for step in (0, 1, 2, 5, 30, 700, 3000):
            shape = list(base)
            shape[axis] += step
            cur = f(*shape)
            assert cur > 0 and cur % 256 == 0 and cur >= prev and cur <= bound(lib, *shape), (shape, cur, prev)
            prev = cur
    prev = 0
    for B in (1, 2, 3, 64, 511, 512, 513, 5000):                    # per batch: no cap by a grid
        cur = f(B, 7, 40, 36)
        assert cur >= prev and cur <= bound(lib, B, 7, 40, 36) and cur % 256 == 0, (B, cur, prev)
        assert cur >= 4 * B * (2 * 7 * 36 + 4 * 7 + 2 * 7 + 3 * 40 + 3)
        prev = cur
    for shape in ((1, 5000, 64, 256), (3, 1251, 640, 256), (1, 4, 1, 1), (515, 1100, 30, 4), (2, 1, 1, 1), (1, 3, 9, 2),
                  (1, 64, 640, 256), (1, 1024, 16384, 256)):
        cur = f(*shape)
        assert 0 < cur <= bound(lib, *shape) and cur % 256 == 0, (shape, cur)
    # laid out for the speakers the rows can hold, not for the bound
    assert f(1, 5000, 64, 256) < 4 * 2 * 100 * 256
    for bad in ((0, 4, 20, 8), (1, 0, 20, 8), (1, 4, 20, 0), (1, 4, 0, 8), (-1, 4, 20, 8), (1, 4, -20, 8), (1, -4, 20, 8), (1, 4, 20, -8)):
        assert f(*bad) == 0, bad


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_cos_sim_labeled
    big = 1 << 40
    ok = dict(E=16, labels=16, B=1, N=4, R=20, D=8, eps_cos=1e-8, eps=1e-6, thr=16, T=50, cos=16, col=None, speakers=None,
              active=None, counts=16, ws=256, ws_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    assert call(E=None) == ERR_NULL and call(labels=None) == ERR_NULL
    assert call(cos=None, counts=None) == ERR_NULL                       # nothing asked for
    assert call(cos=None, counts=None, thr=None, T=0) == ERR_NULL
    for k in ("B", "N", "R", "D"):
        assert call(**{k: 0}) == ERR_SHAPE and call(**{k: -2}) == ERR_SHAPE, k
    assert call(T=-1) == ERR_SHAPE and call(T=4097) == ERR_SHAPE and call(T=4097, counts=None) == ERR_SHAPE
    assert call(thr=None) == ERR_SHAPE and call(T=0) == ERR_SHAPE          # counts without thresholds / with T = 0
    need = lib.ge2e_cos_sim_labeled_workspace_bytes(1, 4, 20, 8)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE
    assert call(ws=None, ws_bytes=0) == ERR_WORKSPACE
    assert call(ws=264) == ERR_WORKSPACE
    assert call(T=4096, ws_bytes=need - 1) == ERR_WORKSPACE                # T = 4096 is a legal shape
    assert call(counts=None, thr=None, T=0, ws_bytes=need - 1) == ERR_WORKSPACE   # cos alone is a legal call
    assert call(cos=None, ws_bytes=need - 1) == ERR_WORKSPACE              # counts alone too
    assert call(E=24) == ERR_ALIGN and call(E=20) == ERR_ALIGN
    # the order: NULL, shape, workspace, alignment
    assert call(labels=None, R=0) == ERR_NULL and call(cos=None, counts=None, T=4097) == ERR_NULL
    assert call(R=0, ws=None) == ERR_SHAPE and call(T=4097, ws=None, E=24) == ERR_SHAPE
    assert call(ws=None, E=24) == ERR_WORKSPACE

    g = lib.ge2e_eer_counts_labeled
    okc = dict(sim=16, col=16, active=16, B=1, N=7, R=29, thr=16, T=33, counts=16, stream=None)

    def callc(**kw):
        a = dict(okc, **kw)
        return g(*[a[k] for k in okc])

    for k in ("sim", "col", "active", "thr", "counts"):
        assert callc(**{k: None}) == ERR_NULL, k
    for k in ("B", "N", "R", "T"):
        assert callc(**{k: 0}) == ERR_SHAPE, k
    assert callc(T=4097) == ERR_SHAPE and callc(sim=None, T=4097) == ERR_NULL


def test_cos_ref_is_the_oracle_at_equal_counts():
    for (N, M, D), seed in (((5, 3, 12), 1), ((4, 2, 7), 2), ((1, 4, 6), 3), ((9, 5, 33), 4)):
        E = orc.synth_embeddings((N, M, D), "unit", seed=seed).astype(np.float64)
        e = torch.as_tensor(E)
        want = orc.expand_form_cos_sim(e, orc.centroids(e)).numpy().reshape(N * M, N)
        labels = np.repeat(np.arange(N), M)
        cos, col, speakers, active = ler.cos_ref(E.reshape(N * M, D), labels, N)
        assert np.abs(cos - want).max() <= 1e-12
        assert col.tolist() == labels.tolist() and speakers.tolist() == list(range(N)) and active.tolist() == [N, N * M]
        # shuffled rows, and a bound above the speaker count: the same numbers at the rows' new places, zeros beyond
        perm = np.random.default_rng(seed).permutation(N * M)
        cos2, col2, spk2, act2 = ler.cos_ref(E.reshape(N * M, D)[perm], labels[perm], N + 3)
        assert np.abs(cos2[:, :N] - want[perm]).max() <= 1e-12 and not cos2[:, N:].any()
        assert col2.tolist() == labels[perm].tolist() and spk2.tolist() == list(range(N)) + [-1] * 3


def test_cos_ref_leaves_out_what_does_not_count():
    labels = np.array([0, 5, 2, 2, -1, 7, 2, 0, 9, 5, 3])          # 9 is outside the bound 8, 7 and 3 are lone
    E = np.random.default_rng(0).standard_normal((11, 6))
    cos, col, speakers, active = ler.cos_ref(E, labels, 8)
    assert active.tolist() == [3, 7] and col.tolist() == [0, 2, 1, 1, -1, -1, 1, 0, -1, 2, -1]
    assert not cos[col < 0].any() and not cos[:, 3:].any() and cos[col >= 0][:, :3].all()
    rows = [0, 7, 2, 3, 6, 1, 9]
    want, _, _, _ = ler.cos_ref(E[rows], [0, 0, 1, 1, 1, 2, 2], 3)
    assert np.array_equal(cos[rows][:, :3], want)
    E2 = E.copy()
    E2[col < 0] = np.nan
    assert np.array_equal(ler.cos_ref(E2, labels, 8)[0], cos)
    empty = ler.cos_ref(E2, [3, 4, -1, 8, 9, 0, 1, 2, 5, 6, 7], 8)
    assert not empty[0].any() and (empty[1] == -1).all() and empty[3].tolist() == [0, 0]


@pytest.mark.parametrize("name", golden_names())
def test_cos_ref_on_every_fixture(name):
    g = load_golden(name)
    N, M, D = g["E"].shape
    cos, col, _, active = ler.cos_ref(g["E"].reshape(N * M, D), np.repeat(np.arange(N), M), N)
    err = np.abs(cos - g["cos64"].reshape(N * M, N)).max()
    assert active.tolist() == [N, N * M] and err <= 1e-12, err


@pytest.mark.parametrize("name", EER_CASES)
def test_counts_ref_and_the_sweep_on_the_eer_fixtures(name):
    S = Z[name + ".S"]
    N, M, _ = S.shape
    col = np.repeat(np.arange(N), M)
    counts = ler.counts_ref(S.reshape(N * M, N), col, N, EV.THRESHOLDS)
    assert np.array_equal(counts, Z[name + ".counts"])
    assert EV.eer_from_labeled_counts(counts, N, N * M) == EV.eer_from_counts(counts, N, M, normalized=True)


def test_counts_ref_and_the_sweep_at_the_edges():
    sim = np.array([[0.7, 0.2, np.nan], [0.6, np.inf, 9.0], [9.0, 9.0, 9.0]], dtype=np.float32)
    counts = ler.counts_ref(sim, [0, 1, -1], 2, [0.5, 0.6, 0.6, 0.7])
    assert counts.tolist() == [[1, 2], [0, 2], [0, 2], [0, 1]]           # strict >, the row with col = -1 and column 2 not read
    assert EV.eer_from_labeled_counts([[0, 0]] * 50, 0, 0) == {"EER": 0.0, "thres": EV.THRESHOLDS[0], "FAR": 0, "FRR": 0}
    r = EV.eer_from_labeled_counts([[0, 3]] * 50, 1, 4)                   # one speaker: no false accept is possible
    assert r["FAR"] == 0 and r["FRR"] == 0.25
