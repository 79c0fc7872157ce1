"""GPU: every kernel instantiation that bounds_cases.LOSS_CASES / RAW_CASES / COS_CASES do not launch, against fp64.

bounds_cases.PLAN_CASES has one entry per kernel name ("atom") the other tables miss (tests/test_plan_cases.py keeps the
four tables' union equal to ge2e_plan_atoms on the CPU).  Each entry runs through the implementation it names and is
compared with oracle.closed_form in fp64 by dense_harness.check_dense(strict=False) at that implementation's row of
dense_harness.TOL; forward-only entries (team_fwd) are held to the loss and per lines of that gate.  Every case first asks
ge2e_loss_plan ON THIS MACHINE and requires the atom in the answer, so it cannot pass by running another kernel.

Small entries (B N M D <= 6e6: every team, team_fwd and fused entry) take the route of tests/test_gpu_bounds.py: the
C ABI on tests/guarded.py buffers, NaN-poisoned outputs between guards, the workspace exactly ge2e_workspace_bytes long,
filled with 0xFF and with 0x00 (both runs must agree bit for bit), every batch checked.

The five tiled entries (the 256 x 256 centroid-gradient tile: at least 192 of them, 7 to 16 M elements) make their
inputs on the device with a seeded generator, as test_gpu_parity.test_config5_benched_launch_sampled does; outputs are
NaN-poisoned before the call; every batch must be finite and EVERY batch is checked against fp64 (the closed form of the
largest, 25 x 800 x 3 x 264, takes about 3 s on the CPU).  w = 7.5, b = -2 as in the other tables; unit rows.

The last test holds the plan of every LOSS_CASES and PLAN_CASES call, asked on this machine, to tests/golden/plans.json,
computed without a GPU: a plan does not depend on the device.
"""
import json

import numpy as np
import pytest
import torch

import bounds_cases as bc
from capi import lib  # noqa: F401
from dense_harness import FILLS, PLANS_JSON, TOL, call_loss, check_dense, check_forward, current_plans
from guarded import same_bits
from oracle import ge2e_oracle as orc

pytestmark = pytest.mark.gpu


def errors(o, ref):
    e = {"loss": np.max(np.abs(o["loss"] - ref["loss"]) / np.maximum(np.abs(ref["loss"]), 1e-30)),
         "per abs": np.abs(o["per"] - ref["per"]).max()}
    if "dE" in o:
        e.update({"dE fro": np.linalg.norm(o["dE"] - ref["dE"]) / np.linalg.norm(ref["dE"]),
                  "dw": np.max(np.abs(o["dw"] - ref["dw"]) / np.maximum(np.abs(ref["dw"]), 1e-30)),
                  "db abs": np.abs(o["db"] - ref["db"]).max()})
    return "  ".join(f"{k} {float(v):.3e}" for k, v in e.items())


def run_small(lib, case):
    atom, impl, B, N, M, D, variant, grad = case
    key = case[1:7]
    E, ref = bc.loss_inputs(key), bc.loss_reference(key)
    combo = ("all", True, True, False) if grad else ("fwd_per", True, False, False)
    o, o0 = (call_loss(lib, key, E, combo, p) for p in FILLS)
    for k in o:
        assert same_bits(o[k], o0[k]), f"{atom}: {k} depends on what the workspace held before the call"
    assert set(o) == ({"loss", "per", "dE", "dw", "db"} if grad else {"loss", "per"})
    print(f"{bc.plan_id(case)}: {errors(o, ref)}   TOL[{impl}] = {TOL[impl]}")
    if grad:
        check_dense(o, ref, impl, atom, strict=False)
    else:
        check_forward(o, ref, impl, atom)


def run_on_device_inputs(case):
    from speaker_embedding_ge2e_loss_amd import functional as GF
    atom, impl, B, N, M, D, variant, grad = case
    assert grad and variant == bc.S
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(B + N + M + D)
    e = torch.nn.functional.normalize(torch.randn(B, N, M, D, generator=g, device=dev), dim=-1)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    out = GF.LossOutputs(loss=nan(B), per=nan(B, N, M), dE=nan(B, N, M, D), dw=nan(B), db=nan(B))
    o = GF.loss_fwd_bwd(e, torch.tensor(bc.W, device=dev), torch.tensor(bc.BIAS, device=dev), variant=variant, impl=impl, out=out)
    torch.cuda.synchronize()
    for k in ("loss", "per", "dE", "dw", "db"):
        assert getattr(o, k).data_ptr() == getattr(out, k).data_ptr(), f"{atom}: {k} is not the poisoned buffer"
        assert bool(torch.isfinite(getattr(o, k)).all()), f"{atom}: {k} keeps NaN poison or holds inf"
    got = {k: getattr(o, k).cpu().numpy() for k in ("loss", "per", "dE", "dw", "db")}
    ref = orc.closed_form(e.cpu().numpy(), bc.W, bc.BIAS, variant=variant)
    for k in ("loss", "per", "dE", "dw", "db"):
        assert np.isfinite(ref[k]).all(), f"{atom}: reference {k}"
    print(f"{bc.plan_id(case)}: {errors(got, ref)}   TOL[{impl}] = {TOL[impl]}")
    for i in range(B):                                  # every batch
        check_dense({k: v[i] for k, v in got.items()}, {k: ref[k][i] for k in got}, impl, f"{atom} batch {i}", strict=False)


@pytest.mark.parametrize("case", bc.PLAN_CASES, ids=bc.plan_id)
def test_the_kernel_a_plan_case_is_there_for(lib, case):
    from speaker_embedding_ge2e_loss_amd import _lib
    atom, impl, B, N, M, D, variant, grad = case
    plan = _lib.loss_plan(B, N, M, D, variant, impl, grad)
    assert atom in plan, f"{case}: this machine would launch {plan}"
    if bc.plan_is_small(case):
        run_small(lib, case)
    else:
        run_on_device_inputs(case)


def test_plans_on_this_machine_are_the_committed_ones(lib):
    with open(PLANS_JSON) as f:
        committed = json.load(f)
    here = current_plans(lib)
    assert len(here) == 2 * len(bc.LOSS_CASES) + len(bc.PLAN_CASES)
    different = {k: (here.get(k), committed.get(k)) for k in set(here) | set(committed) if here.get(k) != committed.get(k)}
    assert not different, f"(here, committed): {different}"
