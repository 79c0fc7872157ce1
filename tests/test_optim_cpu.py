"""CPU: the host side of the native optimizer step -- ge2e_sgd_clip_workspace_bytes / ge2e_sgd_clip_step /
ge2e_sgd_clip_plan: declared, exported and bound, every error code and the order of the checks, the workspace size, the plan
-- tests/optim_ref.py, the oracle of the GPU tests, against torch's own clip_grad_norm_ + SGD in float64, the layout builder
on CPU tensors, and the trainer flag's refusal of CPU parameters."""
import ctypes
import re

import numpy as np
import pytest
import torch

import optim_ref as orf
from capi import built_lib as lib  # noqa: F401
from capi import header_text
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_sgd_clip_workspace_bytes", "ge2e_sgd_clip_step", "ge2e_sgd_clip_plan")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -6
I, P, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_float


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES["ge2e_sgd_clip_workspace_bytes"] == (ctypes.c_size_t, [I])
    assert _lib.PROTOTYPES["ge2e_sgd_clip_step"] == (I, [P, P, I, I, I, P, P, P, F, I, P, P, P, ctypes.c_size_t, P])
    assert _lib.PROTOTYPES["ge2e_sgd_clip_plan"] == (I, [I, I, I, I, I, ctypes.c_char_p, ctypes.c_size_t])
    assert (_lib.MACROS["GE2E_SGD_MAX_GROUPS"], _lib.MACROS["GE2E_SGD_CHUNK"]) == (8, 4096)
    assert (_lib.MACROS["GE2E_SGD_FLAG_ZERO_GRAD"], _lib.MACROS["GE2E_SGD_FLAG_SKIP_NONFINITE"]) == (1, 2)
    assert not any(a.startswith("sgd") for a in _lib.plan_atoms())
    from speaker_embedding_ge2e_loss_amd import functional as GF, optim
    for f in ("sgd_layout", "sgd_clip_step", "sgd_clip_plan"):
        assert callable(getattr(GF, f))
    assert issubclass(optim.ClipSGD, torch.optim.Optimizer)


def test_workspace_is_one_float_a_chunk_in_whole_256_bytes(lib):
    w = lib.ge2e_sgd_clip_workspace_bytes
    assert [w(c) for c in (1, 64, 65, 360, 24415)] == [256, 256, 512, 1536, 97792]
    assert w(2 ** 31 - 1) == 2 ** 33 and w(0) == 0 and w(-1) == 0 and w(-2 ** 31) == 0


def test_step_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_sgd_clip_step
    ok = dict(seg=512, chunk_start=1024, S=3, C=5, G=2, grad=2052, momentum=4100, hyper=8192, scale=1.0, flags=3, stats=64,
              skipped=128, ws=256, ws_bytes=256, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("seg", "chunk_start", "grad", "hyper"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(skipped=None) == ERR_NULL and call(skipped=None, flags=2) == ERR_NULL       # the skip flag needs its counter
    for kw in (dict(S=0), dict(S=-1), dict(C=0), dict(G=0), dict(G=-3), dict(C=2), dict(G=9), dict(flags=4), dict(flags=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(ws=None), dict(ws=384), dict(ws=257), dict(ws_bytes=255), dict(ws_bytes=0), dict(C=65), dict(C=65, ws_bytes=511)):
        assert call(**kw) == ERR_WORKSPACE, kw
    for kw in (dict(grad=2053), dict(grad=2054), dict(momentum=4101), dict(momentum=4102), dict(momentum=4103)):
        assert call(**kw) == ERR_ALIGN, kw
    # the order: NULL, shape, workspace, alignment
    assert call(grad=None, S=0) == ERR_NULL and call(hyper=None, ws=None, momentum=4101) == ERR_NULL
    assert call(skipped=None, G=9) == ERR_NULL
    assert call(S=0, ws=None) == ERR_SHAPE and call(C=2, grad=2053) == ERR_SHAPE and call(G=9, ws_bytes=0, momentum=4101) == ERR_SHAPE
    assert call(ws=257, grad=2053) == ERR_WORKSPACE and call(ws_bytes=255, momentum=4102) == ERR_WORKSPACE


def test_plan_names_the_two_launches_and_their_grids(lib):
    plan = lambda *a: _lib._plan(lib.ge2e_sgd_clip_plan, *a)  # noqa: E731
    assert plan(20, 360, 2, 0, 0) == ["sgd_sqsum/4096/360", "sgd_update<plain>/4096/360"]
    assert plan(20, 360, 2, 1, 3) == ["sgd_sqsum/4096/360", "sgd_update<mom>/4096/360"]
    assert plan(1, 1, 1, 0, 1) == ["sgd_sqsum/4096/1", "sgd_update<plain>/4096/1"]
    assert plan(300, 300, 8, 7, 2)[1] == "sgd_update<mom>/4096/300"
    f = lib.ge2e_sgd_clip_plan
    assert f(1, 1, 1, 0, 0, None, 0) == len("sgd_sqsum/4096/1,sgd_update<plain>/4096/1")
    for bad in ((0, 1, 1, 0, 0), (1, 0, 1, 0, 0), (1, 1, 0, 0, 0), (3, 2, 1, 0, 0), (1, 1, 9, 0, 0), (1, 1, 1, 0, 4), (-1, 5, 1, 1, 0)):
        assert f(*bad, None, 0) == ERR_SHAPE, bad
    with pytest.raises(ValueError):
        plan(3, 2, 1, 0, 0)


SIZES = (1, 1, 3, 5, 37, 64, 129)
GROUPS = (0, 0, 1, 0, 1, 1, 0)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_the_oracle_is_clip_grad_norm_then_sgd(momentum, weight_decay):
    """Three steps, two groups: clip_grad_norm_ on each group's parameters, then torch.optim.SGD, in float64 on the CPU --
    the statements s4:201-203 call -- against optim_ref.step to 1e-12.  The second group's threshold is high enough never to
    clip and the first's low enough always to; the scale 0.5 is exact in either form (div_(2) and a product)."""
    rng = np.random.default_rng(5)
    lrs, max_norms, scale = (0.05, 0.2), (0.7, 1e3), 0.5
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n))) for n in SIZES]
    by_group = [[p for p, k in zip(params, GROUPS) if k == g] for g in (0, 1)]
    opt = torch.optim.SGD([{"params": by_group[0], "lr": lrs[0]}, {"params": by_group[1], "lr": lrs[1]}], lr=1.0,
                          momentum=momentum, weight_decay=weight_decay)
    hyper = [[lrs[g], max_norms[g], weight_decay, momentum] for g in (0, 1)]
    mine = [p.detach().numpy().copy() for p in params]
    moms = [np.zeros(n) for n in SIZES] if momentum else None
    clipped = []
    for s in range(3):
        grads = [rng.standard_normal(n) * (3.0 if s != 1 else 0.05) for n in SIZES]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
            p.grad.div_(2.0)
        for g in (0, 1):
            torch.nn.utils.clip_grad_norm_(by_group[g], max_norms[g])
        opt.step()
        r = orf.step(mine, grads, moms, GROUPS, hyper, grad_scale=scale)
        mine, moms = r["params"], r["moms"]
        clipped.append(r["coef"][0] < 1)
        assert r["coef"][1] == 1.0 and r["skipped"] == 0
        for p, q, gq in zip(params, mine, r["grads"]):
            assert np.abs(p.detach().numpy() - q).max() <= 1e-12
            assert np.abs(p.grad.numpy() - gq).max() <= 1e-12                   # what the clips leave in .grad
        if momentum:
            for p, m in zip(params, moms):
                assert np.abs(opt.state[p]["momentum_buffer"].numpy() - m).max() <= 1e-12
    assert clipped == [True, False, True]


def test_the_oracle_on_zero_and_nonfinite_gradients():
    hyper = [[0.1, 1.0, 0.0, 0.0], [0.1, 1.0, 0.0, 0.0]]
    p = [np.ones(3), np.ones(2)]
    r = orf.step(p, [np.zeros(3), np.array([3.0, 4.0])], None, (0, 1), hyper)
    assert r["norm"].tolist() == [0.0, 5.0] and r["coef"][0] == 1.0 and abs(r["coef"][1] - 1 / (5 + 1e-6)) < 1e-15
    assert np.array_equal(r["params"][0], p[0])
    r = orf.step(p, [np.array([1.0, np.nan, 0.0]), np.array([np.inf, 4.0])], None, (0, 1), hyper)
    assert np.isnan(r["coef"][0]) and r["coef"][1] == 0.0 and np.isnan(r["params"][0]).all()
    assert np.isnan(r["grads"][1][0]) and r["grads"][1][1] == 0.0 and r["skipped"] == 0
    r = orf.step(p, [np.array([1.0, np.nan, 0.0]), np.array([1.0, 4.0])], None, (0, 1), hyper, skip_nonfinite=True, zero_grad=True)
    assert r["skipped"] == 1 and all(np.array_equal(a, b) for a, b in zip(r["params"], p)) and not r["grads"][0].any()
    # the float32 emulation rounds every operation on its own: a case where a fused multiply-add would differ
    f32 = np.float32
    g, pp, lr = f32(1.3040000200271606), f32(0.9470809698104858), f32(0.543624997138977)
    got = orf.emulate_f32([1.0], [[pp]], [[g]], None, (0,), [[lr, np.inf, 0, 0]])[0][0][0]
    fused = f32(np.float64(pp) - np.float64(lr) * np.float64(g))              # (the product of two float32 is exact in float64)
    assert got == f32(pp - f32(lr * g)) != fused and got.dtype == np.float32
    assert orf.stats_f32([np.inf, np.nan, 0.0, 3.0], [1.0, 1.0, 1.0, 1.5]).tolist()[::2] == [0.0, 1.0]


def test_layout_counts_chunks_sorts_by_group_and_refuses_what_it_cannot_update():
    from speaker_embedding_ge2e_loss_amd import functional as GF
    sizes = (1, 1, 3, 5, 4095, 4096, 4097, 8193)
    a = [torch.zeros(n) for n in sizes]
    groups = [[a[0], a[2], a[4], a[6]], [a[1], a[3], a[5], a[7]]]
    off = dict(zip(map(id, a), np.cumsum((0,) + sizes[:-1]).tolist()))
    lay = GF.sgd_layout(groups, [[off[id(t)] for t in g] for g in groups])
    assert (lay.S, lay.G) == (8, 2) and lay.C == sum(orf.chunk_counts(sizes)) == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3
    seg = lay.seg.tolist()
    assert [s[3] for s in seg] == [0, 0, 0, 0, 1, 1, 1, 1] and [s[2] for s in seg] == [1, 3, 4095, 4097, 1, 5, 4096, 8193]
    assert [s[0] for s in seg] == [t.data_ptr() for g in groups for t in g] and [s[1] for s in seg] == [off[id(t)] for g in groups for t in g]
    assert lay.chunk_start.dtype == torch.int32 and lay.chunk_start.tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 11]
    assert lay.seg.dtype == torch.int64 and lay.seg.device.type == "cpu" and lay.workspace is None
    # an empty tensor has nothing to update; a moved storage is noticed
    lay = GF.sgd_layout([[a[0], torch.zeros(0)], [a[1]]], [[0, 1], [1]])
    assert (lay.S, lay.C, lay.G) == (2, 2, 2) and not lay.refresh()
    old = a[0].data_ptr()
    a[0].data = torch.ones(1)
    assert lay.refresh() and lay.seg[0, 0].item() == a[0].data_ptr() != old and not lay.refresh()
    with pytest.raises(ValueError, match="twice"):
        GF.sgd_layout([[a[2]], [a[3], a[2]]], [[0], [3, 8]])
    with pytest.raises(TypeError, match="float32"):
        GF.sgd_layout([[a[2], torch.zeros(4, dtype=torch.float64)]], [[0, 3]])
    with pytest.raises(TypeError, match="float32"):
        GF.sgd_layout([[torch.zeros(4, dtype=torch.float16)]], [[0]])
    with pytest.raises(ValueError, match="one device"):
        GF.sgd_layout([[a[2], torch.zeros(4, device="meta")]], [[0, 3]])
    for bad in (dict(groups=[], flat_grad_offsets=[]), dict(groups=[[a[2]]] * 9, flat_grad_offsets=[[0]] * 9),
                dict(groups=[[a[2]]], flat_grad_offsets=[[0, 1]]), dict(groups=[[a[2]]], flat_grad_offsets=[[-1]]),
                dict(groups=[[torch.zeros(0)]], flat_grad_offsets=[[0]]), dict(groups=[[torch.zeros(4, 4).t()]], flat_grad_offsets=[[0]])):
        with pytest.raises(ValueError):
            GF.sgd_layout(**bad)


def test_native_step_needs_gpu_float32_parameters():
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    from speaker_embedding_ge2e_loss_amd.optim import ClipSGD
    from speaker_embedding_ge2e_loss_amd.trainer import DPTrainer

    class Loss(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor(10.0))
            self.b = torch.nn.Parameter(torch.tensor(-5.0))

    with pytest.raises(ValueError, match="native_step"):
        DPTrainer(SpeakerEncoder(4, 4, 1, 4), Loss(), native_step=True)
    tr = DPTrainer(SpeakerEncoder(4, 4, 1, 4), Loss())                     # the default is torch's route, as before
    assert tr.native_step is False and type(tr.optimizer) is torch.optim.SGD
    with pytest.raises(ValueError, match="float32 parameters of one GPU"):
        ClipSGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    import inspect
    from speaker_embedding_ge2e_loss_amd.trainer import TrainEmbedModel
    assert inspect.signature(TrainEmbedModel.__init__).parameters["native_step"].default is False
