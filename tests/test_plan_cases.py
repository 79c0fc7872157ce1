"""CPU: which kernels the GPU tables launch, against every kernel the library can launch (no GPU, no launch).

ge2e_resolve_impl names an implementation; below it every launcher picks again among kernels and template
instantiations.  The library reports that pick (ge2e_loss_plan, ge2e_cos_sim_plan: the launchers' own decision functions,
printed) and lists every kernel name there is (ge2e_plan_atoms).  Here:

  - a scan of shapes wide enough for every threshold must reach every listed name, and no other: a name the scan cannot
    reach is an instantiation that is compiled and never run;
  - the calls the GPU tests make from bounds_cases.LOSS_CASES / RAW_CASES / COS_CASES / PLAN_CASES must launch every listed
    name between them (the failure names the missing ones), and PLAN_CASES holds only what the other three miss;
  - tests/golden/plans.json keeps the plan of every LOSS_CASES and PLAN_CASES call as computed here;
    tests/test_gpu_plans.py asks again on the GPU machine (a plan must not depend on the device);
  - every PLAN_CASES entry that runs on CPU-made inputs has a finite fp64 reference and, as contrast, no row that ties
    its two largest other-speaker similarities (the GPU tests skip nothing; a draw that ties is changed in SEEDS).  The five
    tiled entries make their inputs on the device: tests/test_gpu_plans.py holds their references finite there; they
    are softmax.
"""
import ctypes
import json

import numpy as np
import pytest

import bounds_cases as bc
from capi import built_lib as lib  # noqa: F401
from dense_harness import PLANS_JSON, current_plans
from speaker_embedding_ge2e_loss_amd import _lib, build

# The scan.  N to 1024 (tiled's limit) around 8 (a team), 16 (AUTO's team / cos thresholds), 64, 128, 256 and the wave
# kernels' speaker counts; M 2..17 one by one (the wave kernels' M, 10 | 11: prep and team registers, 16 | 17: team) and
# 64 | 65 (fused), 70; D in every residue class mod 4, 8, 32 and 64 that a predicate asks about, either side of 64, 128,
# 192, 256, 512, 768, 1024; B either side of 192 / 256 tiles at 1, 2, 4, 8 tiles per batch and of AUTO's 208, 256, 384.
NS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 57, 64, 65, 128, 129, 255, 256, 257, 272, 512, 513, 528, 800, 1024)
MS = tuple(range(2, 18)) + (64, 65, 70)
DS = (1, 4, 7, 8, 32, 36, 64, 65, 72, 100, 128, 132, 192, 200, 252, 256, 260, 264, 288, 320, 512, 520, 768, 776, 1024)
BS = (1, 2, 3, 24, 25, 32, 47, 48, 65, 96, 191, 192, 224, 256, 257, 4096)
AUTO_BS = (1, 207, 208, 256, 257, 383, 384, 4096)
COMBOS = ((0, 0), (0, 1), (1, 0), (1, 1))      # (variant, want_grad)
EXPLICIT = ("generic", "fused_f32", "fused_split", "tiled", "team", "wave")


@pytest.fixture(scope="module")
def atoms(lib):
    names = _lib.plan_atoms()
    assert len(names) == len(set(names)) and all(names), names
    return names


def scan(lib):
    """{atom: first (query, arguments) that names it} over the grid above: every implementation that accepts a shape
    (explicitly and through both AUTOs), both variants, with and without gradients; the raw entry; ge2e_cos_sim."""
    buf = ctypes.create_string_buffer(512)
    seen, first = set(), {}

    def take(what):
        s = buf.value
        if s not in seen:
            seen.add(s)
            for a in _lib.split_plan(s.decode()):
                first.setdefault(a, what)

    loss, cos = lib.ge2e_loss_plan, lib.ge2e_cos_sim_plan
    for N in NS:
        for M in MS:
            for D in DS:
                for name in EXPLICIT + ("auto", "auto_no_team"):
                    impl = _lib.IMPLS[name]
                    # (an implementation refuses a shape whatever B is; only TILED's plan and AUTO's choice look at B)
                    if loss(1, N, M, D, 0, impl, 1, 0, buf, 512) < 0:
                        continue
                    for B in BS if name == "tiled" else AUTO_BS if name.startswith("auto") else (1, 4096):
                        for variant, grad in COMBOS:
                            n = loss(B, N, M, D, variant, impl, grad, 0, buf, 512)
                            assert 0 < n < 512, (name, B, N, M, D, variant, grad, n)
                            take(("loss", name, B, N, M, D, variant, grad))
                for grad in (0, 1):
                    if loss(3, N, M, D, 1, 0, grad, 1, buf, 512) > 0:
                        take(("raw", 3, N, M, D, 1, grad))
                for B in (1, 48, 192):
                    assert cos(B, N, M, D, buf, 512) > 0
                    take(("cos", B, N, M, D))
    return first


def test_scan_reaches_every_kernel_the_library_lists_and_no_other(lib, atoms):
    first = scan(lib)
    unreachable = [a for a in atoms if a not in first]
    assert not unreachable, f"compiled, listed and launched for no shape of the scan: {unreachable}"
    unlisted = {a: w for a, w in first.items() if a not in atoms}
    assert not unlisted, f"launched but not in ge2e_plan_atoms: {unlisted}"
    assert len(atoms) == 94      # 1 generic + 8 fused + 24 wave + 18 team + 18 team_fwd + 25 tiled


def test_the_gpu_tables_launch_every_kernel(lib, atoms):
    plans = bc.table_plans(lib)
    have = {a for table in plans.values() for _, plan in table for a in plan}
    missing = [a for a in atoms if a not in have]
    assert not missing, f"no case of LOSS_CASES, RAW_CASES, COS_CASES or PLAN_CASES launches: {missing}"
    assert have <= set(atoms), sorted(have - set(atoms))


def test_plan_cases_hold_exactly_what_the_other_tables_miss(lib, atoms):
    plans = bc.table_plans(lib)
    others = {a for t in ("LOSS_CASES", "RAW_CASES", "COS_CASES") for _, plan in plans[t] for a in plan}
    named = [c[0] for c in bc.PLAN_CASES]
    assert len(set(named)) == len(named) and len(set(bc.PLAN_CASES)) == len(bc.PLAN_CASES)
    want = [a for a in atoms if a not in others]
    assert sorted(named) == sorted(want), (f"PLAN_CASES lacks {sorted(set(want) - set(named))} and holds, beyond what the other "
                                           f"tables miss, {sorted(set(named) - set(want))}")
    for c, (_, plan) in zip(bc.PLAN_CASES, plans["PLAN_CASES"]):
        atom, impl, B, N, M, D, variant, grad = c
        assert atom in plan, f"{c}: launches {plan}"
        assert lib.ge2e_resolve_impl(B, N, M, D, _lib.VARIANTS[variant], _lib.IMPLS[impl]) == _lib.IMPLS[impl], c
        # contrast only where the kernel's name carries the variant; the forward-only kernels run forward only
        assert (variant == bc.C) == atom.endswith("contrast>"), c
        assert grad == (not atom.startswith("team_fwd")), c
        # only the 256 x 256 centroid-gradient tiles are too large for the guarded C-ABI route
        assert bc.plan_is_small(c) == (not atom.startswith("tiled_gc")), c


def test_the_walked_tiles_of_every_dma_kernel_run_more_than_one_round(lib):
    tiled = [c for c in bc.PLAN_CASES if c[1] == "tiled"]
    assert {c[0]: bc.c3_tiles(c) for c in tiled} == bc.PLAN_TILES
    for kernel in ("tiled_sim<C3>", "tiled_gc<C3>", "tiled_ge<C3>"):
        assert max(t[kernel] for t in bc.PLAN_TILES.values()) > 256, f"{kernel}: no case walks more than 256 tiles"
    for c in tiled:      # the smallest launch of the big centroid-gradient tile there is: 192 of them
        assert c[2] * ((c[3] + 255) // 256) * ((c[5] + 255) // 256) >= 192, c


def test_committed_plans_are_the_plans_computed_here(lib):
    """tests/golden/plans.json, which the GPU machine is held to.  Regenerate from the repository root:
    PYTHONPATH=. python tests/test_plan_cases.py"""
    with open(PLANS_JSON) as f:
        committed = json.load(f)
    assert committed == current_plans(lib)


def test_plan_queries_answer_like_snprintf_and_refuse_what_the_call_refuses(lib):
    args = (48, 288, 9, 320, 0, _lib.IMPLS["tiled"], 1, 0)
    want = b"tiled_prep<10,2>,tiled_sim<C3>,tiled_rows<64>,tiled_gc<C3>/4,tiled_spk,tiled_ge<C3>"
    assert lib.ge2e_loss_plan(*args, None, 0) == len(want)                      # NULL, 0: just measures
    buf = ctypes.create_string_buffer(b"#" * 255, 256)
    assert lib.ge2e_loss_plan(*args, buf, 256) == len(want) and buf.value == want
    buf = ctypes.create_string_buffer(b"#" * 255, 256)
    assert lib.ge2e_loss_plan(*args, buf, 10) == len(want) and buf.raw[:11] == want[:9] + b"\0#"     # truncated, terminated
    assert _lib.split_plan(want.decode()) == ["tiled_prep<10,2>", "tiled_sim<C3>", "tiled_rows<64>", "tiled_gc<C3>/4",
                                              "tiled_spk", "tiled_ge<C3>"]
    assert _lib.loss_plan(48, 288, 9, 320, impl="tiled", want_grad=False)[-2:] == ["tiled_rows<64>", "tiled_reduce"]
    buf = ctypes.create_string_buffer(64)
    assert lib.ge2e_loss_plan(1, 4, 1, 8, 0, 0, 1, 0, buf, 64) == -2                        # M = 1
    assert lib.ge2e_loss_plan(1, 4, 5, 8, 7, 0, 1, 0, buf, 64) == -4                        # variant
    assert lib.ge2e_loss_plan(1, 64, 10, 512, 0, _lib.IMPLS["team"], 1, 0, buf, 64) == -5   # what ge2e_resolve_impl says
    assert lib.ge2e_loss_plan(1, 64, 10, 256, 0, 0, 1, 1, buf, 64) == -5                    # no raw shape
    assert lib.ge2e_cos_sim_plan(1, 4, 1, 8, buf, 64) == -2
    assert _lib.cos_sim_plan(2, 15, 4, 64) == ["generic"]                                   # N < 16: the VALU kernel
    assert _lib.cos_sim_plan(1, 16, 3, 64) == ["tiled_prep<10,1>", "tiled_sim<C1>", "tiled_cos"]
    # AUTO's plan is the plan of what it resolves to; the metric shape has kernels of its own
    assert _lib.loss_plan(3, 64, 10, 256) == _lib.loss_plan(3, 64, 10, 256, impl="team") == ["team<4,10,5,softmax>"]
    assert _lib.loss_plan(3, 64, 10, 256, "contrast", want_grad=False) == ["team_fwd<4,10,5,contrast>"]
    assert _lib.loss_plan(5, 4, 5, 256, raw=True) == ["wave<5,4,raw>"] and _lib.loss_plan(5, 8, 5, 256, impl="wave") == ["wave<5,8>"]


SMALL = [c for c in bc.PLAN_CASES if bc.plan_is_small(c)]


@pytest.mark.parametrize("case", SMALL, ids=bc.plan_id)
def test_plan_reference_is_finite_and_contrast_does_not_tie(case):
    ref = bc.loss_reference(case[1:7])
    for k in ("loss", "per", "dE", "dw", "db"):
        assert np.isfinite(ref[k]).all(), f"{case}: {k}"
    if case[6] == bc.C:
        assert bc.top2_gap_ok(ref, case[3]), f"{case}: two largest other-speaker similarities tie; change the seed"


if __name__ == "__main__":
    build.build(verbose=False)
    with open(PLANS_JSON, "w") as out:
        json.dump(current_plans(_lib.load()), out, indent=0, sort_keys=True)
        out.write("\n")
    print("wrote", PLANS_JSON)
