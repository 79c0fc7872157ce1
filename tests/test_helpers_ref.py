"""CPU: anchors tests/helpers_ref.py (the fp64 reference of tests/test_gpu_helpers.py) before anything is compared with it.

With B = 1, n = N, j0 = 0 it must BE the oracle's expand form (values and autograd gradients); a (j0, n) slice must equal
the corresponding rows of the whole batch whatever the other speakers' rows are; and it must be finite on every seeded
input the GPU module feeds it.
"""
import numpy as np
import pytest
import torch

import helpers_ref as hr
from conftest import load_golden
from oracle import ge2e_oracle as orc

F64 = torch.float64


def close12(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max(), np.abs(b).max())


def anchor_inputs():
    out = {f"{N}x{M}x{D}": orc.synth_embeddings((N, M, D), "raw", seed=N * M + D) for (N, M, D) in ((4, 5, 16), (3, 2, 7), (7, 3, 33))}
    name = [n for n in __import__("conftest").golden_names() if "g8_degenerate" in n][0]
    out["g8_degenerate"] = load_golden(name)["E"]
    return out


@pytest.mark.parametrize("name", ["4x5x16", "3x2x7", "7x3x33", "g8_degenerate"])
def test_whole_batch_form_is_the_oracles_expand_form(name):
    E = anchor_inputs()[name].astype(np.float64)
    N, M, D = E.shape
    rng = np.random.default_rng(3)
    Cn = rng.standard_normal((N, D))                       # NOT the centroids of E
    g = torch.as_tensor(rng.standard_normal((N, M, N)))
    e1, c1 = torch.tensor(E, requires_grad=True), torch.tensor(Cn, requires_grad=True)
    cos1 = orc.expand_form_cos_sim(e1, c1)
    cos1.backward(g)
    e2, c2 = torch.tensor(E[None], requires_grad=True), torch.tensor(Cn[None], requires_grad=True)
    cos2 = hr.cos_rows(e2, c2, 0)
    cos2.backward(g[None])
    close12(cos2[0].detach(), cos1.detach(), "cos")
    close12(e2.grad[0], e1.grad, "dE")
    close12(c2.grad[0], c1.grad, "dC")
    for variant in ("softmax", "contrast"):
        e1 = torch.tensor(E, requires_grad=True)
        w1, b1 = torch.tensor(10.0, dtype=F64, requires_grad=True), torch.tensor(-5.0, dtype=F64, requires_grad=True)
        loss1, per1, _ = orc.expand_form_loss(e1, w1, b1, variant=variant)
        loss1.backward()
        e2 = torch.tensor(E[None], requires_grad=True)
        w2, b2 = torch.tensor(10.0, dtype=F64, requires_grad=True), torch.tensor(-5.0, dtype=F64, requires_grad=True)
        loss2, per2 = hr.calc_loss_rows(w2 * hr.cos_rows(e2, hr.centroids(e2), 0) + b2, 0, orc.SMALL_ERR, variant)
        loss2.sum().backward()
        close12(loss2[0].detach(), loss1.detach(), "loss")
        close12(per2[0].detach(), per1.detach(), "per")
        close12(e2.grad[0], e1.grad, f"{variant} dE")
        close12(w2.grad, w1.grad, "dw")
        close12(b2.grad, b1.grad, "db")
    close12(hr.utterance_centroids(torch.tensor(E[None]))[0], orc._leave_one_out_centroids(torch.tensor(E)), "loo")


@pytest.mark.parametrize("j0,n", [(0, 1), (6, 1), (2, 3), (4, 3), (0, 7)])
def test_a_slice_equals_its_rows_of_the_whole_batch(j0, n):
    rng = np.random.default_rng(9)
    B, N, M, D = 2, 7, 3, 10
    E, C = rng.standard_normal((B, N, M, D)), rng.standard_normal((B, N, D))
    g = rng.standard_normal((B, N, M, N))
    whole = hr.cos_rows_np(E, C, 0, g)
    E2 = rng.standard_normal((B, N, M, D))                 # other speakers' rows: arbitrary
    E2[:, j0:j0 + n] = E[:, j0:j0 + n]
    g2 = np.zeros_like(g)
    g2[:, j0:j0 + n] = g[:, j0:j0 + n]
    masked = hr.cos_rows_np(E2, C, 0, g2)                  # whole-batch form, gradient through the slice's rows only
    part = hr.cos_rows_np(E[:, j0:j0 + n], C, j0, g[:, j0:j0 + n])
    close12(part["cos"], whole["cos"][:, j0:j0 + n], "cos")
    close12(part["dE"], whole["dE"][:, j0:j0 + n], "dE")
    close12(part["dC"], masked["dC"], "partial dC")
    S = rng.standard_normal((B, N, M, N)) * 3
    gl, gp = rng.standard_normal(B), rng.standard_normal((B, N, M))
    for variant in ("softmax", "contrast"):
        w = hr.calc_loss_rows_np(S, 0, 1e-6, variant, None, gp)
        p = hr.calc_loss_rows_np(S[:, j0:j0 + n], j0, 1e-6, variant, gl, gp[:, j0:j0 + n])
        close12(p["per"], w["per"][:, j0:j0 + n], "per")
        close12(p["loss"], w["per"][:, j0:j0 + n].sum(axis=(1, 2)), "loss")
        # d_sim of a row = (g_loss[b] + g_per[row]) * d per_row / d S_row
        unit = hr.calc_loss_rows_np(S, 0, 1e-6, variant, None, np.ones_like(gp))["dS"][:, j0:j0 + n]
        close12(p["dS"], unit * (gl[:, None, None] + gp[:, j0:j0 + n])[..., None], "dS")


def test_shards_partial_centroid_gradients_sum_to_the_whole():
    rng = np.random.default_rng(4)
    B, N, M, D = 1, 9, 2, 5
    E, C, g = rng.standard_normal((B, N, M, D)), rng.standard_normal((B, N, D)), rng.standard_normal((B, N, M, N))
    whole = hr.cos_rows_np(E, C, 0, g)
    tot = sum(hr.cos_rows_np(E[:, a:b], C, a, g[:, a:b])["dC"] for a, b in ((0, 1), (1, 5), (5, 9)))
    close12(tot, whole["dC"], "sum of partial dC")


def test_reference_is_finite_on_every_gpu_case():
    for case in hr.COS_CASES:
        E, C, g = hr.cos_inputs(case)
        r = hr.cos_rows_np(E, C, case[5], g)
        assert all(np.isfinite(v).all() for v in r.values()), case
    for kind in hr.DEGENERATE:
        E, C, g = hr.degenerate_inputs(kind)
        r = hr.cos_rows_np(E, C, 0, g)
        assert all(np.isfinite(v).all() for v in r.values()), kind
    for case in hr.LOSS_CASES:
        S, gl, gp = hr.loss_inputs(case)
        r = hr.calc_loss_rows_np(S, case[4], case[6], case[5], gl, gp)
        assert all(np.isfinite(v).all() for v in r.values()), case
    S, gl, gp, _ = hr.tie_inputs()
    r = hr.calc_loss_rows_np(S, 0, 1e-6, "contrast", gl, gp)
    assert all(np.isfinite(v).all() for v in r.values())


def test_degenerate_inputs_are_what_they_claim():
    for kind in ("tiny_row", "tiny_centroid"):
        E, C, _ = hr.degenerate_inputs(kind)
        norms = np.concatenate([np.linalg.norm(E.astype(np.float64), axis=-1).ravel(), np.linalg.norm(C.astype(np.float64), axis=-1).ravel()])
        assert ((norms > 0) & (norms < hr.EPS_COS)).sum() == 1
    E, _, _ = hr.degenerate_inputs("loo_zero")
    assert np.all(E[0, 2, 1] + E[0, 2, 2] == 0)
    S, _, _, pairs = hr.tie_inputs()
    for idx in np.ndindex(pairs.shape[:3]):
        k1, k2 = pairs[idx]
        row = S[idx].copy()
        assert row[k1] == row[k2] and idx[1] not in (k1, k2)
        row[idx[1]] = -np.inf
        assert row[k1] == row.max() and (row == row.max()).sum() == 2
