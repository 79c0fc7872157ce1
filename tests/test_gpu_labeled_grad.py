"""GPU: the differentiable labelled helpers -- ge2e_cos_sim_labeled_bwd, ge2e_calc_loss_labeled / _bwd, and
functional.cos_sim_labeled(differentiable=True) / functional.calc_loss_labeled.

Reference, never the code under test: tests/labeled_grad_ref.py (torch autograd in float64 on the CPU, on
masked_ref.index_ref), which tests/test_labeled_grad_cpu.py holds to labeled_eval_ref.cos_ref and masked_ref.masked_loss.
The C-ABI tests call through ctypes on the guarded buffers of tests/guarded.py: inputs between guards, outputs poisoned, the
workspace exactly ge2e_cos_sim_labeled_bwd_workspace_bytes between guard bands, filled with 0xFF bytes in one run and 0x00 in
another (the two must agree bit for bit), guards intact and inputs unmodified afterwards.  g_cos is seeded standard normal
with NaN on every entry that must not be read (rows that are not active, columns >= n_act); E holds NaN on the rows that do
not count.

Gates are the project's own.  dE against fp64: rowlist_harness.check_rows' gradient gate -- relative Frobenius norm <= GT = 1e-5 or
max-abs <= 1e-8, and max-abs <= 4 GT max(1, max|ref|) -- and the same at factor 2 between two fp32 results.  per / loss /
d_sim of calc_loss_labeled: the gates tests/test_gpu_helpers.py holds ge2e_calc_loss / _bwd to (per rtol 2e-4 atol 2e-5, loss
rtol 2e-5 + 3e-7 sum|per| + 2e-7 rows, d_sim rel-Frobenius < 1e-5, and for one speaker with eps > 0, where d_sim vanishes by
cancellation, 4x the fp32 reference's own max error).  `-s` prints every figure before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import labeled_grad_ref as lgr
import masked_ref as mr
import rowlist_cases as rc
from capi import GF, lib  # noqa: F401
from conftest import rel_fro
from rowlist_cases import EDGE_CASES, LOSS_CASES, draw, host_ids, inputs
from rowlist_harness import (BIAS, DEV, EPS, EPS_COS, GT, VAR, VARIANTS, W, check_rows, run_bwd, run_calc, run_wide, same_bits,
                             two_part)

pytestmark = pytest.mark.gpu


# ---- gates -------------------------------------------------------------------------------------------------------------------
def grad_gate(got, ref, what, factor=1.0):
    """rowlist_harness.check_rows' gate on dE."""
    ref = np.asarray(ref, np.float64)
    scale = max(1.0, float(np.abs(ref).max()))
    fro, mabs = rel_fro(got, ref), float(np.abs(got - ref).max())
    print(f"{what}: dE fro {fro:.3e} / {factor * GT:.0e}  max-abs {mabs:.3e} / {factor * 4 * GT * scale:.3e}  max|ref| {np.abs(ref).max():.3e}")
    assert fro <= factor * GT or mabs <= factor * 1e-8, f"{what} dE rel-fro {fro}"
    assert mabs <= factor * 4 * GT * scale, f"{what} dE max-abs {mabs}"


def plus_zero(a):
    return not a.any() and not np.signbit(a).any()


def seeded_g(col, n_act, N, seed):
    """g_cos (R, N) float32: standard normal on the entries that count, NaN everywhere else."""
    g = np.random.default_rng(seed).standard_normal((len(col), N)).astype(np.float32)
    g[~lgr.counted(col, n_act, N)] = np.nan
    return g


# ---- 1. edge shapes against fp64 ------------------------------------------------------------------------------------------------
def _edge_cases():
    cases = dict(EDGE_CASES)                                                    # name: (labels, N, D)
    cases["D64_steps4"] = (draw(10, 40, 4, 2, 3, 64), 10, 64)
    cases["D128_steps8"] = (draw(10, 40, 4, 2, 3, 65), 10, 128)
    cases["D256_steps16"] = (draw(10, 40, 4, 2, 3, 66), 10, 256)
    cases["N20_16_byte_g_cos"] = (draw(20, 70, 18, 1, 3, 67), 20, 24)           # N % 4 == 0, two column tiles of which one partial
    cases["R300_three_pieces"] = (draw(20, 300, 9, 3, 6, 68), 20, 24)           # wide_split = 3, r_act = 291
    return cases


GRAD_CASES = _edge_cases()


@functools.lru_cache(maxsize=None)
def grad_case(name):
    """(E with NaN on the rows that do not count, labels, N, g_cos, fp64 dE, index reference) of one batch: computed once,
    shared, read-only."""
    labels, N, D = GRAD_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    idx = mr.index_ref(labels, N)
    E[~idx["active_row"]] = np.nan
    _, _, _, col = lgr.cos_graph(E, labels, N)
    g = seeded_g(col, idx["active"][0], N, 900 + len(labels) + D)
    dE = lgr.cos_bwd(E, labels, N, g, EPS, EPS_COS)
    for v in (E, g, dE):
        v.setflags(write=False)
    return E, labels, N, g, dE, idx


def test_the_cases_reach_what_they_are_named_for():
    assert rc.wide_split(300) == 3 and grad_case("R300_three_pieces")[5]["active"][1] == 291
    assert int(grad_case("nact67_of_2_rows_D36")[5]["active"][0]) == 67 and 67 % 4 != 0
    assert grad_case("N20_16_byte_g_cos")[5]["active"][0] == 18 and 20 % 4 == 0
    assert grad_case("nact0")[5]["active"].tolist() == [0, 0]


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_edge_shapes(lib, name):
    E, labels, N, g, ref, idx = grad_case(name)
    full = run_bwd(lib, E[None], labels[None], N, g[None], 0xFF)
    zero = run_bwd(lib, E[None], labels[None], N, g[None], 0x00)
    for k in full:
        assert same_bits(full[k], zero[k]), f"{name}: {k} depends on what the workspace held before the call"
    assert full["active"][0].tolist() == idx["active"].tolist(), f"{name}: active"
    grad_gate(full["dE"][0], ref, name)
    assert plus_zero(full["dE"][0][~idx["active_row"]]), f"{name}: dE is not +0 on a row that is not active"
    # without `active`; g_cos at float alignment only (element loads where the 16-byte ones ran): the same gradient
    alone = run_bwd(lib, E[None], labels[None], N, g[None], 0xFF, want_active=False)
    assert same_bits(alone["dE"], full["dE"]), f"{name}: dE differs without active"
    shifted = run_bwd(lib, E[None], labels[None], N, g[None], 0xFF, g_offset=1)
    assert same_bits(shifted["dE"], full["dE"]), f"{name}: dE depends on the alignment of g_cos"


# ---- 2. nothing active, everything active, mixed ----------------------------------------------------------------------------------
def test_batches_none_all_and_mixed(lib):
    N, R, D = 9, 24, 24
    rng = np.random.default_rng(21)
    labels = np.stack([np.concatenate([np.arange(8), np.full(16, -1)])[rng.permutation(R)],   # eight lone speakers
                       np.repeat(np.arange(6), 4)[rng.permutation(R)],
                       draw(N, R, 3, 2, 4, 22)]).astype(np.int32)
    idxs = [mr.index_ref(labels[i], N) for i in range(3)]
    assert [i["active"].tolist() for i in idxs][:2] == [[0, 0], [6, 24]] and 0 < idxs[2]["active"][1] < R
    E = np.stack([inputs(labels[i], N, D, 6100 + i) for i in range(3)])
    g = np.empty((3, R, N), dtype=np.float32)
    for i in range(3):
        E[i][~idxs[i]["active_row"]] = np.nan
        g[i] = seeded_g(lgr.cos_graph(E[i], labels[i], N)[3], idxs[i]["active"][0], N, 6200 + i)
    o = run_bwd(lib, E, labels, N, g)
    for i in range(3):
        assert o["active"][i].tolist() == idxs[i]["active"].tolist(), f"batch {i}: active"
        assert plus_zero(o["dE"][i][~idxs[i]["active_row"]]), f"batch {i}: dE is not +0 where nothing counts"
        grad_gate(o["dE"][i], lgr.cos_bwd(E[i], labels[i], N, g[i]), f"B3 batch {i}")
    assert plus_zero(o["dE"][0])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------
def test_stack_of_37_and_its_flip(lib):
    B, N, R, D = 37, 12, 48, 20
    labels = np.stack([draw(N, R, 2 + i % 4, i % 5, 3 + i % 7, 300 + i) for i in range(B)])
    labels[11] = -1                                                       # a batch in which nothing counts
    E = np.stack([inputs(labels[i], N, D, 6300 + i) for i in range(B)])
    g = np.stack([seeded_g(lgr.cos_graph(E[i], labels[i], N)[3], mr.index_ref(labels[i], N)["active"][0], N, 6400 + i)
                  for i in range(B)])
    a = run_bwd(lib, E, labels, N, g, 0xFF)
    again = run_bwd(lib, E, labels, N, g, 0x00)
    flipped = run_bwd(lib, E[::-1], labels[::-1], N, g[::-1], 0xFF)
    for k in a:
        assert same_bits(a[k], again[k]), f"{k}: two launches differ"
        for i in range(B):
            assert same_bits(a[k][i], flipped[k][B - 1 - i]), f"{k}: batch {i} depends on its position in the stack"
    for i in (0, 11, 36):
        grad_gate(a["dE"][i], lgr.cos_bwd(E[i], labels[i], N, g[i]), f"B37 batch {i}")


# ---- 4. consistency with the wide loss ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(name, variant):
    """(E, labels, N, float64 references) of one LOSS_CASES batch: the composed chain of labeled_grad_ref and the masked loss."""
    labels, N, D, _ = LOSS_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    return E, labels, N, lgr.composed(E, labels, N, W, BIAS, variant=variant), mr.masked_loss(E, labels, N, W, BIAS, variant=variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_the_wide_loss_gradient_from_its_own_dcos(lib, name, variant):
    E, labels, N, chain, masked = chain_case(name, variant)
    g = chain["g_cos"].astype(np.float32)                                  # A and AD of the wide loss: w g, from the reference
    g[~lgr.counted(chain["col"], chain["active"][0], N)] = np.nan
    got = run_bwd(lib, E[None], labels[None], N, g[None])["dE"][0]
    wide = run_wide(lib, E[None], labels[None], N, variant)["dE"][0]
    grad_gate(got, wide.astype(np.float64), f"{name}/{variant} against the wide loss", factor=2.0)
    grad_gate(got, masked["dE"], f"{name}/{variant} against masked_ref")


# ---- 5. calc_loss_labeled ----------------------------------------------------------------------------------------------------------
N_ACTS = (0, 1, 2, 17, 67)


def calc_inputs(seed, N=70, R=75):
    """One batch per n_act of N_ACTS: sim (B, R, N) with NaN on everything that must not be read, col with -1 and columns past
    n_act among the rows, active, and the two incoming gradients (g_per NaN on the rows that do not count)."""
    rng = np.random.default_rng(seed)
    B = len(N_ACTS)
    sim = (rng.standard_normal((B, R, N)) * 3).astype(np.float32)
    col = np.empty((B, R), dtype=np.int32)
    for i, n in enumerate(N_ACTS):
        col[i] = rng.integers(-1, n + 2, R)                                # -1 .. n + 1: both kinds of rows that do not count
        if n:
            col[i][:n] = rng.permutation(n)                                # every column is somebody's own
        sim[i][~lgr.counted(col[i], n, N)] = np.nan
    active = np.array([[n, int(((col[i] >= 0) & (col[i] < n)).sum())] for i, n in enumerate(N_ACTS)], dtype=np.int32)
    gl = rng.standard_normal(B).astype(np.float32)
    gp = rng.standard_normal((B, R)).astype(np.float32)
    for i, n in enumerate(N_ACTS):
        gp[i][~((col[i] >= 0) & (col[i] < n))] = np.nan
    return sim, col, active, gl, gp


def check_calc(o, sim, col, active, eps, variant, gl, gp, what):
    B, R, N = sim.shape
    for i in range(B):
        n = int(active[i][0])
        gli, gpi = (None if gl is None else float(gl[i])), (None if gp is None else gp[i])
        ref = lgr.calc_loss_ref(sim[i], col[i], n, eps, variant, gli, gpi)
        floor = 0.0
        if variant == "softmax" and n == 1 and eps > 0:
            # one speaker: d_sim = g (p_jj - 1) is what fp32 leaves of 1 / (1 + eps e^-s) - 1; the reference in fp32 loses it the
            # same way (tests/test_gpu_helpers.py: 4x the fp32 reference's max error, absolute)
            r32 = lgr.calc_loss_ref(sim[i], col[i], n, eps, variant, gli, gpi, dtype=torch.float32)
            floor = 4 * float(np.abs(r32["dS"] - ref["dS"]).max())
        lfloor = 3e-7 * np.abs(ref["per"]).sum() + 2e-7 * R
        lerr = abs(float(o["loss"][i]) - float(ref["loss"]))
        perr = float(np.abs(o["per"][i] - ref["per"]).max())
        rf, mx = rel_fro(o["dS"][i], ref["dS"]), float(np.abs(o["dS"][i] - ref["dS"]).max())
        print(f"{what} n_act {n}: loss {lerr:.3e} / {2e-5 * abs(float(ref['loss'])) + lfloor:.3e}  per max|diff| {perr:.3e}"
              f"  d_sim rel_fro {rf:.3e} max|diff| {mx:.3e} floor {floor:.3e}")
        assert lerr <= 2e-5 * abs(float(ref["loss"])) + lfloor, f"{what} n_act {n}: loss"
        assert np.allclose(o["per"][i], ref["per"], rtol=2e-4, atol=2e-5), f"{what} n_act {n}: per"
        assert rf < 1e-5 or mx <= floor, f"{what} n_act {n}: d_sim rel_fro {rf:.3e}, max|diff| {mx:.3e} (floor {floor:.3e})"
        rest = ~lgr.counted(col[i], n, N)
        assert plus_zero(o["dS"][i][rest]), f"{what} n_act {n}: d_sim is not +0 where nothing counts"
        assert plus_zero(o["per"][i][rest.all(axis=1)]), f"{what} n_act {n}: per is not +0 on a row that does not count"


@pytest.mark.parametrize("incoming", ["g_loss", "g_per", "both"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_calc_loss_labeled_forward_and_backward(lib, variant, incoming):
    sim, col, active, gl, gp = calc_inputs(70 + VAR[variant])
    gl = gl if incoming != "g_per" else None
    gp = gp if incoming != "g_loss" else None
    for eps in (EPS, 0.0):
        o = run_calc(lib, sim, col, active, eps, variant, gl, gp)
        check_calc(o, sim, col, active, eps, variant, gl, gp, f"{variant} {incoming} eps {eps}")
    noloss = run_calc(lib, sim, col, active, EPS, variant, gl, gp, want_loss=False)      # loss = NULL: the same per
    assert same_bits(noloss["per"], run_calc(lib, sim, col, active, EPS, variant, gl, gp)["per"])


def test_calc_loss_labeled_contrast_tie_goes_to_the_lowest_index(lib):
    rng = np.random.default_rng(5)
    R, N, n_act = 12, 9, 7
    sim = (rng.standard_normal((1, R, N))).astype(np.float32)
    col = rng.integers(0, n_act, (1, R)).astype(np.int32)
    pairs = np.empty((R, 2), dtype=np.int64)
    for r in range(R):
        others = np.setdiff1d(np.arange(n_act), [col[0, r]])
        pairs[r] = np.sort(rng.choice(others, 2, replace=False))
        sim[0, r, pairs[r]] = 4.0                                          # bit-equal, above everything else of the row
    sim[0, :, n_act:] = np.nan
    active = np.array([[n_act, R]], dtype=np.int32)
    gl = np.array([0.75], dtype=np.float32)
    o = run_calc(lib, sim, col, active, EPS, "contrast", gl, None)
    check_calc(o, sim, col, active, EPS, "contrast", gl, None, "tie")
    got = np.take_along_axis(o["dS"][0], pairs, axis=1)
    assert (got[:, 0] != 0).all() and not got[:, 1].any(), "the max term's gradient belongs to the lower index of the pair"


# ---- 6. the Python surface -----------------------------------------------------------------------------------------------------------
def chain(GF, E, labels, variant, w=W, b=BIAS, **kw):
    """The composed chain in Python: cosines, w * cos + b in torch, calc_loss_labeled, backward -> numpy loss, per, dE, dw, db."""
    dev = torch.device(DEV)
    e = torch.as_tensor(E, device=dev).clone().requires_grad_(True)
    wt = torch.tensor(w, device=dev, requires_grad=True)
    bt = torch.tensor(b, device=dev, requires_grad=True)
    o = GF.cos_sim_labeled(e, labels, differentiable=True, **kw)
    loss, per = GF.calc_loss_labeled(wt * o.cos + bt, o.col, o.active, variant=variant)
    loss.sum().backward()
    f = lambda t: t.detach().cpu().numpy()  # noqa: E731
    return {"loss": f(loss), "per": f(per), "dE": f(e.grad), "dw": wt.grad.item(), "db": bt.grad.item(), "active": f(o.active)}


def wide_loss(GF, E, labels, variant, w=W, b=BIAS, **kw):
    """ge2e_loss_labeled(wide=True) and its backward; per from the same entry, forward only."""
    dev = torch.device(DEV)
    e = torch.as_tensor(E, device=dev).clone().requires_grad_(True)
    wt = torch.tensor(w, device=dev, requires_grad=True)
    bt = torch.tensor(b, device=dev, requires_grad=True)
    loss = GF.ge2e_loss_labeled(e, labels, wt, bt, variant=variant, wide=True, **kw)
    loss.sum().backward()
    per = GF.loss_fwd_bwd_labeled(e.detach(), labels, wt.detach(), bt.detach(), variant=variant, wide=True, need_grad=False,
                                  need_per=True, **kw).per
    f = lambda t: t.detach().cpu().numpy()  # noqa: E731
    return {"loss": f(loss), "per": f(per).reshape(e.shape[:-1]), "dE": f(e.grad), "dw": wt.grad.item(), "db": bt.grad.item()}


def as_ref(o):
    return {k: np.asarray(o[k], np.float64) for k in ("loss", "per", "dE", "dw", "db")}


def test_python_surface(GF, lib):
    dev = torch.device(DEV)
    E, labels, N, g, ref_dE, idx = grad_case("nact17_of_N40_D36")
    R, D = E.shape
    clean = np.nan_to_num(E)                                               # (torch would carry the NaN rows into dw)
    e = torch.as_tensor(clean, device=dev).requires_grad_(True)
    lab32 = torch.as_tensor(labels, device=dev)
    o = GF.cos_sim_labeled(e, lab32, num_speakers=N, differentiable=True, thresholds=[0.5])
    assert o.cos.requires_grad and o.cos.shape == (R, N) and o.counts.shape == (1, 2)
    assert not any(t.requires_grad for t in (o.col, o.speakers, o.active, o.counts))
    plain = GF.cos_sim_labeled(e, lab32, num_speakers=N)
    assert not plain.cos.requires_grad and torch.equal(plain.cos, o.cos.detach()) and torch.equal(plain.col, o.col)
    # a seeded linear functional of cos: test 1's dE, bit for bit (the call does not depend on whose workspace it runs on)
    G = torch.as_tensor(np.nan_to_num(g), device=dev)
    (dE,) = torch.autograd.grad((o.cos * G).sum(), e)
    want = run_bwd(lib, clean[None], labels[None], N, g[None])["dE"][0]
    assert same_bits(dE.cpu().numpy(), want), "autograd's dE is not ge2e_cos_sim_labeled_bwd's"
    grad_gate(dE.cpu().numpy(), ref_dE, "autograd.grad of a linear functional")
    # a float64, non-contiguous incoming gradient is made contiguous float32
    (dE64,) = torch.autograd.grad(GF.cos_sim_labeled(e, lab32, num_speakers=N, differentiable=True).cos,
                                  e, grad_outputs=G.double().t().contiguous().t())
    assert torch.equal(dE64, dE)
    # no gradient asked for: nothing is recorded
    assert not GF.cos_sim_labeled(e.detach(), lab32, num_speakers=N, differentiable=True).cos.requires_grad
    with pytest.raises(ValueError, match="differentiable=True"):
        GF.cos_sim_labeled(e, lab32, num_speakers=N, differentiable=True, need_cos=False, thresholds=[0.5])
    with pytest.raises(TypeError, match="torch.int32"):
        GF.calc_loss_labeled(o.cos, o.col.long(), o.active)

    # the composed chain: device int32 labels with a bound, device int64 labels, host labels of arbitrary ids, 3-D input
    host = host_ids(labels, N, 9).tolist()
    lab64 = torch.as_tensor(labels.astype(np.int64), device=dev)
    for variant in VARIANTS:
        ref = mr.masked_loss(clean, labels, N, W, BIAS, variant=variant)
        wide = wide_loss(GF, clean, lab32, variant, num_speakers=N)
        routes = {"int32 device labels": chain(GF, clean, lab32, variant, num_speakers=N),
                  "int64 device labels": chain(GF, clean, lab64, variant, num_speakers=N + 9),
                  "host labels": chain(GF, clean, host, variant)}
        b3 = chain(GF, clean[None], lab32[None], variant, num_speakers=N)
        assert b3["loss"].shape == (1,) and b3["per"].shape == (1, R) and b3["dE"].shape == (1, R, D)
        routes["3-D input"] = {k: (v[0] if k in ("loss", "per", "dE", "active") else v) for k, v in b3.items()}
        for what, got in routes.items():
            assert got["active"].tolist() == idx["active"].tolist(), what
            assert got["loss"].shape == () and got["per"].shape == (R,) and got["dE"].shape == (R, D)
            check_rows(got, ref, f"[chain {variant}] {what} against masked_ref")
            check_rows(got, as_ref(wide), f"[chain {variant}] {what} against ge2e_loss_labeled(wide=True)", factor=2.0)
            assert plus_zero(got["dE"][~idx["active_row"]]) and plus_zero(got["per"][~idx["active_row"]])


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_forward_and_backward(GF):
    dev = torch.device(DEV)
    N, R, D = 12, 48, 20
    lab_a, lab_b = draw(N, R, 5, 6, 9, 2), draw(N, R, 3, 2, 20, 51)
    assert mr.index_ref(lab_a, N)["active"].tolist() != mr.index_ref(lab_b, N)["active"].tolist()
    e = torch.as_tensor(inputs(lab_a, N, D, 8000), device=dev)[None].contiguous().requires_grad_(True)
    w = torch.tensor(W, device=dev, requires_grad=True)
    b = torch.tensor(BIAS, device=dev, requires_grad=True)
    lab = torch.zeros(1, R, dtype=torch.int32, device=dev)

    def step():
        o = GF.cos_sim_labeled(e, lab, num_speakers=N, differentiable=True)
        loss, per = GF.calc_loss_labeled(w * o.cos + b, o.col, o.active)
        return (loss, per, o.active) + torch.autograd.grad(loss.sum(), (e, w, b))

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()                                                             # (nothing counts yet)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    names = ("loss", "per", "active", "dE", "dw", "db")
    for labels in (lab_a, lab_b):
        lab.copy_(torch.as_tensor(labels, device=dev)[None])
        with torch.no_grad():
            for t in out:
                t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for k, got, want in zip(names, out, eager):
            assert torch.equal(got, want), f"replay differs from the eager calls: {k}"
        ref = mr.masked_loss(e.detach().cpu().numpy()[0], labels, N, W, BIAS)
        assert out[2][0].tolist() == ref["index"]["active"].tolist()
        check_rows({"loss": out[0][0].item(), "per": out[1][0].detach().cpu().numpy(), "dE": out[3][0].cpu().numpy(), "dw": out[4].item(),
                    "db": out[5].item()}, ref, f"replay with active {ref['index']['active'].tolist()}")


# ---- 8. degenerate inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", ["identical_rows", "zero_row"])
def test_degenerate_rows_through_the_chain(GF, kind, variant):
    """Held as tests/test_gpu_rowlist_inputs.py holds these kinds: the clamped speaker's rows relative to the largest entry,
    every other row at the ordinary bound (rowlist_harness.two_part)."""
    E, labels, N, ref, deg = rc.degenerate_case(kind, variant)
    idx = ref["index"]
    got = chain(GF, E, torch.as_tensor(labels, device=DEV), variant, num_speakers=N)
    assert got["active"].tolist() == idx["active"].tolist()
    assert plus_zero(got["dE"][~idx["active_row"]]) and plus_zero(got["per"][~idx["active_row"]])
    two_part(got, ref, deg, idx["active_row"], f"[degenerate chain] {kind}/{variant}")
    wide = wide_loss(GF, E, torch.as_tensor(labels, device=DEV), variant, num_speakers=N)
    two_part(got, as_ref(wide), deg, idx["active_row"], f"[degenerate chain-vs-wide] {kind}/{variant}", factor=2.0)
