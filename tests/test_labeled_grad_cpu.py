"""CPU: the host side of the differentiable labelled helpers -- ge2e_cos_sim_labeled_bwd (+ its workspace query),
ge2e_calc_loss_labeled / _bwd and `functional.cos_sim_labeled(differentiable=True)` / `functional.calc_loss_labeled`:
declared, exported and bound, the ABI version unmoved, the error codes and their order, the workspace between the one plane
it cannot do without and the wide entry's, the float64 reference of tests/labeled_grad_ref.py held to the references that
exist (labeled_eval_ref.cos_ref, masked_ref.masked_loss), and the argument errors raised before any device is needed."""
import ctypes
import re

import numpy as np
import pytest
import torch

from capi import built_lib as lib  # noqa: F401
from capi import header_text
import labeled_eval_ref as ler
import labeled_grad_ref as lgr
import masked_ref as mr
from rowlist_cases import LOSS_CASES, inputs
from speaker_embedding_ge2e_loss_amd import _lib, build

SYMS = ("ge2e_cos_sim_labeled_bwd_workspace_bytes", "ge2e_cos_sim_labeled_bwd", "ge2e_calc_loss_labeled",
        "ge2e_calc_loss_labeled_bwd")
ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_VARIANT, ERR_ALIGN = -1, -2, -3, -4, -6


def test_header_library_and_binding_have_the_symbols(lib):
    text = header_text()
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} not declared in include/ge2e_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.PROTOTYPES
    assert lib.ge2e_abi_version() == 2 and "#define GE2E_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert _lib.PROTOTYPES[SYMS[0]] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert len(_lib.PROTOTYPES[SYMS[1]][1]) == 13 and len(_lib.PROTOTYPES[SYMS[2]][1]) == 11
    assert len(_lib.PROTOTYPES[SYMS[3]][1]) == 12
    from speaker_embedding_ge2e_loss_amd import functional as GF
    ent = GF._ENTRIES["labeled_cos_bwd"]
    assert ent.entry == SYMS[1] and ent.size_query == SYMS[0] and not ent.dense_f32
    assert all(ent.tag != other.tag for k, other in GF._ENTRIES.items() if k != "labeled_cos_bwd")


def test_argument_validation_of_the_cosine_backward(lib):
    """Codes and their order: NULL, shape, workspace, alignment; g_cos needs float alignment only."""
    big = 1 << 40
    ok = dict(E=16, labels=16, g_cos=16, B=1, N=4, R=20, D=8, eps_cos=1e-8, dE=32, active=None, ws=256, ws_bytes=big,
              stream=None)
    need = lib.ge2e_cos_sim_labeled_bwd_workspace_bytes
    table = [
        (dict(E=None), ERR_NULL), (dict(labels=None), ERR_NULL), (dict(g_cos=None), ERR_NULL), (dict(dE=None), ERR_NULL),
        (dict(B=0), ERR_SHAPE), (dict(N=0), ERR_SHAPE), (dict(D=0), ERR_SHAPE), (dict(R=0), ERR_SHAPE), (dict(R=-3), ERR_SHAPE),
        (dict(ws_bytes=need(1, 4, 20, 8) - 1), ERR_WORKSPACE), (dict(ws=None, ws_bytes=0), ERR_WORKSPACE),
        (dict(ws=264), ERR_WORKSPACE), (dict(R=7, ws_bytes=need(1, 4, 7, 8) - 1), ERR_WORKSPACE),
        (dict(R=1, N=50, ws=None), ERR_WORKSPACE),
        (dict(E=24), ERR_ALIGN), (dict(dE=40), ERR_ALIGN), (dict(R=7, E=24), ERR_ALIGN),
        # the order of the checks
        (dict(g_cos=None, R=0), ERR_NULL), (dict(dE=None, ws=None), ERR_NULL), (dict(R=0, ws=None), ERR_SHAPE),
        (dict(D=0, E=24), ERR_SHAPE), (dict(ws=None, E=24), ERR_WORKSPACE), (dict(ws=264, dE=40), ERR_WORKSPACE),
    ]
    for kw, want in table:
        a = dict(ok, **kw)
        got = lib.ge2e_cos_sim_labeled_bwd(*[a[k] for k in ok])
        assert got == want, (kw, got, want)
    # g_cos one float past a 16-byte boundary passes every host check the others fail on: the first failing check is not its own
    assert lib.ge2e_cos_sim_labeled_bwd(*[dict(ok, g_cos=20, E=24)[k] for k in ok]) == ERR_ALIGN
    assert lib.ge2e_cos_sim_labeled_bwd(*[dict(ok, g_cos=20, ws=None)[k] for k in ok]) == ERR_WORKSPACE


def test_argument_validation_of_calc_loss_labeled(lib):
    """Codes and their order: NULL, shape, variant; loss and the two gradients may be NULL."""
    fwd = dict(sim=16, col=16, active=16, B=1, N=4, R=20, eps=1e-6, variant=0, loss=None, per=16, stream=None)
    bwd = dict(sim=16, col=16, active=16, B=1, N=4, R=20, eps=1e-6, variant=1, g_loss=None, g_per=None, d_sim=16, stream=None)
    common = [
        (dict(sim=None), ERR_NULL), (dict(col=None), ERR_NULL), (dict(active=None), ERR_NULL),
        (dict(B=0), ERR_SHAPE), (dict(N=0), ERR_SHAPE), (dict(R=0), ERR_SHAPE), (dict(R=-2), ERR_SHAPE),
        (dict(variant=2), ERR_VARIANT), (dict(variant=-1), ERR_VARIANT),
        (dict(col=None, N=0), ERR_NULL), (dict(N=0, variant=9), ERR_SHAPE), (dict(active=None, variant=9), ERR_NULL),
    ]
    for f, ok, own in ((lib.ge2e_calc_loss_labeled, fwd, [(dict(per=None), ERR_NULL), (dict(per=None, B=0), ERR_NULL)]),
                       (lib.ge2e_calc_loss_labeled_bwd, bwd, [(dict(d_sim=None), ERR_NULL), (dict(d_sim=None, R=0), ERR_NULL)])):
        for kw, want in common + own:
            a = dict(ok, **kw)
            got = f(*[a[k] for k in ok])
            assert got == want, (f.__name__, kw, got, want)


def test_workspace_bytes(lib):
    f, wide = lib.ge2e_cos_sim_labeled_bwd_workspace_bytes, lib.ge2e_workspace_bytes_labeled_wide
    for bad in ((0, 4, 20, 8), (1, 0, 20, 8), (1, 4, 20, 0), (1, 4, 0, 8), (-1, 4, 20, 8), (1, 4, -20, 8), (1, -4, 20, 8)):
        assert f(*bad) == 0, bad
    for N, R in ((1251, 640), (1, 1), (64, 640), (12, 48), (4, 1), (7, 2100), (1100, 300), (1024, 16384), (9, 129)):
        for D in (1, 37, 256):
            prev = 0
            for B in (1, 2, 3, 37, 600):
                if B * R * N * D > 1 << 33:
                    continue
                NA = max(1, min(N, R // 2))
                cur = f(B, N, R, D)
                assert cur > 0 and cur % 256 == 0, (B, N, R, D, cur)
                assert 4 * B * R * NA <= cur <= wide(B, N, R, D, 0), (B, N, R, D, cur)
                assert cur >= prev and (cur > prev or B * R * NA * 4 < 256), (B, N, R, D, cur, prev)
                prev = cur
    # no tile partials: one 256-byte part less than the wide entry where they fit into one
    assert wide(1, 64, 640, 256, 0) - f(1, 64, 640, 256) == 256


@pytest.mark.parametrize("name", ["nact17_of_N40_D36", "ract33_in_R48", "nact0", "nact1_D5"])
def test_reference_cosines_are_the_evaluation_references(name):
    labels, N, D, _ = LOSS_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    cos, col, speakers, active = ler.cos_ref(E, labels, N)
    poisoned = E.copy()
    poisoned[col < 0] = np.nan                                   # the rows that do not count are never looked at
    _, got, idx, got_col = lgr.cos_graph(poisoned, labels, N)
    assert np.array_equal(got_col, col) and np.array_equal(idx["active"], active)
    assert np.abs(got.detach().numpy() - cos).max() <= 1e-14


@pytest.mark.parametrize("variant", ["softmax", "contrast"])
@pytest.mark.parametrize("name", ["nact17_of_N40_D36", "ract33_in_R48"])
def test_reference_composed_chain_is_the_masked_loss(name, variant):
    labels, N, D, _ = LOSS_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    want = mr.masked_loss(E, labels, N, 10.0, -5.0, variant=variant)
    got = lgr.composed(E, labels, N, 10.0, -5.0, variant=variant)
    for k in ("loss", "per", "dE", "dw", "db"):
        err = float(np.abs(got[k] - want[k]).max())
        print(f"{name} {variant} {k}: max|diff| {err:.2e}")
        assert err <= 1e-12, (name, variant, k, err)
    # the same dE from the cosine backward alone, fed with the chain's dL/dcos; and calc_loss_ref on the chain's sim
    dE = lgr.cos_bwd(E, labels, N, got["g_cos"])
    assert np.abs(dE - want["dE"]).max() <= 1e-12
    r = lgr.calc_loss_ref(10.0 * got["cos"] - 5.0, got["col"], got["active"][0], variant=variant, g_loss=1.0)
    assert np.abs(r["per"] - want["per"]).max() <= 1e-12 and abs(r["loss"] - want["loss"]) <= 1e-12
    assert np.abs(10.0 * r["dS"] - got["g_cos"]).max() <= 1e-12


def test_reference_calc_loss_ignores_what_does_not_count():
    rng = np.random.default_rng(3)
    R, N, n_act = 9, 7, 4
    sim = rng.standard_normal((R, N)) * 3
    col = rng.integers(-1, n_act, R).astype(np.int32)
    col[0], col[1] = -1, n_act                                   # not counted: no column, a column past n_act
    gp = rng.standard_normal(R)
    a = lgr.calc_loss_ref(sim, col, n_act, variant="contrast", g_loss=0.5, g_per=gp)
    wild, gw = sim.copy(), gp.copy()
    wild[:, n_act:], wild[:2], gw[:2] = np.nan, np.nan, np.nan
    b = lgr.calc_loss_ref(wild, col, n_act, variant="contrast", g_loss=0.5, g_per=gw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not a["dS"][:2].any() and not a["dS"][:, n_act:].any() and not a["per"][:2].any() and a["dS"][2:, :n_act].any()
    assert lgr.calc_loss_ref(sim, col, 0, g_loss=1.0)["loss"] == 0.0 and not lgr.calc_loss_ref(sim, col, 0, g_loss=1.0)["dS"].any()


def test_python_argument_errors_before_any_device():
    """As far as a machine without a GPU can say."""
    from speaker_embedding_ge2e_loss_amd import functional as GF
    e = torch.zeros(8, 4, device="meta")
    lab = torch.zeros(8, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="differentiable=True"):
        GF.cos_sim_labeled(e, lab, num_speakers=3, differentiable=True, need_cos=False)
    with pytest.raises(ValueError, match="differentiable=True"):
        GF.cos_sim_labeled(e, lab, num_speakers=3, differentiable=True, need_cos=False, thresholds=[0.5])
    sim = torch.zeros(8, 3)
    col, active = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for bad_col, bad_active in ((col.long(), active), (col, active.float()), (col.tolist(), active), (col[:5], active),
                                (col, torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(TypeError, match="torch.int32"):
            GF.calc_loss_labeled(sim, bad_col, bad_active)
    with pytest.raises(ValueError, match=r"\(R,N\) or \(B,R,N\)"):
        GF.calc_loss_labeled(sim[0], col, active)
    with pytest.raises(ValueError, match="variant"):
        GF.calc_loss_labeled(sim, col, active, variant="hinge")
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # well-typed arguments on the host: the usual refusal
        GF.calc_loss_labeled(sim, col, active)
