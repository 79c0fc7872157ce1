"""CPU: the case tables of tests/bounds_cases.py against the library's own predicates (no GPU, no launch).

Every case must be accepted by the implementation it names, the tables must hold the padding edges the library reports
(scanned through ge2e_resolve_impl / ge2e_raw_supported, not remembered), every fp64 reference must be finite and no
contrast case may tie its two largest other-speaker similarities: the GPU tests skip nothing, so a seed that ties is
changed here.
"""
import numpy as np
import pytest

import bounds_cases as bc
from capi import built_lib as lib  # noqa: F401
from speaker_embedding_ge2e_loss_amd import _lib

VAR = _lib.VARIANTS
IMPL = _lib.IMPLS


def accepts(lib, impl, N, M, D, B=1):
    return lib.ge2e_resolve_impl(B, N, M, D, 0, IMPL[impl]) == IMPL[impl]


def cases_of(impl):
    return [c for c in bc.LOSS_CASES if c[0] == impl]


def test_every_case_is_accepted_and_sized(lib):
    assert len(set(bc.LOSS_CASES)) == len(bc.LOSS_CASES)
    for c in bc.LOSS_CASES:
        impl, B, N, M, D, variant = c
        assert B * N * M * D <= bc.MAX_ELEMS, c
        assert variant == bc.S or N >= 2, c
        got = lib.ge2e_resolve_impl(B, N, M, D, VAR[variant], IMPL[impl])
        if impl in bc.AUTO_REACHES:
            assert got > 0, c
        else:
            assert got == IMPL[impl], f"{c}: ge2e_resolve_impl returned {got}"
        nbytes = lib.ge2e_workspace_bytes(B, N, M, D, VAR[variant], IMPL[impl])
        if _lib.IMPL_NAMES[got] == "wave":
            assert nbytes == 0, c
        else:
            assert nbytes > 0 and nbytes % 256 == 0, f"{c}: {nbytes} workspace bytes"


def test_auto_cases_reach_every_implementation(lib):
    for auto, want in bc.AUTO_REACHES.items():
        got = {_lib.IMPL_NAMES[lib.ge2e_resolve_impl(B, N, M, D, VAR[v], IMPL[auto])] for _, B, N, M, D, v in cases_of(auto)}
        assert got == want, f"{auto}: reaches {sorted(got)}, wanted {sorted(want)}"
        assert len(cases_of(auto)) == len(want)


def test_the_listed_edges_are_in_the_table():
    field = {"B": 1, "N": 2, "M": 3, "D": 4}
    for impl, edges in bc.REQUIRED.items():
        for name, values in edges.items():
            have = {c[field[name]] for c in cases_of(impl)}
            assert values <= have, f"{impl}: no case with {name} in {sorted(values - have)}"
        assert {c[5] for c in cases_of(impl)} == {bc.S, bc.C}, impl
    assert {c[0] for c in bc.COMBOS} == {"all", "no_per", "fwd_per", "fwd", "misaligned"}


@pytest.mark.parametrize("impl", ["fused_f32", "fused_split"])
def test_fused_tables_hold_the_extremes_the_library_reports(lib, impl):
    D = 256
    ns = [n for n in range(1, 130) if accepts(lib, impl, n, 2, D)]
    ms = [m for m in range(2, 130) if accepts(lib, impl, ns[0], m, D)]
    have = cases_of(impl)
    for n in (ns[0], ns[-1]):
        assert any(c[2] == n for c in have), f"{impl}: no case at N = {n}"
    for m in (ms[0], ms[-1]):
        assert any(c[3] == m for c in have), f"{impl}: no case at M = {m}"
    assert any(c[2] == ns[-1] and c[3] == ms[-1] for c in have), f"{impl}: no case at its largest N and M together"
    ds = [d for d in range(1, 300) if accepts(lib, impl, 4, 4, d)]
    assert any(c[4] == ds[0] for c in have) and any(c[4] == ds[-1] for c in have), f"{impl}: D range {ds[0]}..{ds[-1]}"
    assert any(c[1] > 256 for c in have), f"{impl}: no B beyond the grid"        # grids: 256 workgroups / one per CU (256)


def test_team_table_holds_the_largest_member_image(lib):
    ok = [(n, m) for n in range(1, 65) for m in range(2, 17) if accepts(lib, "team", n, m, 256)]
    assert ok, "the team kernel takes no shape here"
    top = max((n + 7) // 8 * m for n, m in ok)
    have = cases_of("team")
    assert any((c[2] + 7) // 8 * c[3] == top and c[4] == 256 for c in have), f"no team case with (N + 7) / 8 * M = {top} at D = 256"
    assert any(c[2] % 8 != 0 for c in have)                                       # uneven members
    assert any(c[1] % 2 == 1 and c[1] > 1 for c in have)                          # odd B: team_fwd keeps two batches in flight
    assert not accepts(lib, "team", 64, 16, 256)


def test_tiled_table_sits_off_its_tile_sizes(lib):
    have = cases_of("tiled")
    assert any(c[3] > 64 for c in have)
    for t in (64, 128, 256):
        assert any((c[2] * c[3]) % t != 0 for c in have)
    assert all(((c[2] + 63) // 64 * 64) % c[2] != 0 for c in have if c[2] in (15, 65, 130, 300))
    assert any(c[4] % 32 == 0 for c in have) and any(c[4] % 32 != 0 for c in have)
    assert not accepts(lib, "tiled", 65, 3, 196) and not accepts(lib, "tiled", 65, 3, 1032)


def test_wave_and_raw_tables_hold_every_instantiation_at_its_largest_n(lib):
    ms = [m for m in range(2, 65) if accepts(lib, "wave", 1, m, 256)]
    assert tuple(ms) == bc.RAW_MS
    have = cases_of("wave")
    raw = [bc.resolve_raw(lib, c) for c in bc.RAW_CASES]
    for m in ms:
        nxl = max(n for n in range(1, 65) if accepts(lib, "wave", n, m, 256))
        nx = bc.raw_max_n(lib, m, 256)
        assert 1 <= nx < nxl and not lib.ge2e_raw_supported(nx + 1, m, 256)
        assert any(c[2] == nxl and c[3] == m for c in have), f"wave: no case at M = {m}, N = {nxl} (large)"
        assert any(c[2] == nx and c[3] == m for c in have), f"wave: no case at M = {m}, N = {nx} (register-only)"
        assert any(c[1] == nx and c[2] == m for c in raw), f"raw: no case at M = {m}, N = {nx}"
        assert any(c[1] == 1 and c[2] == m for c in raw), f"raw: no case at M = {m}, N = 1"
    for B, N, M, D, variant in raw:
        assert lib.ge2e_raw_supported(N, M, D) and B * N * M * D <= bc.MAX_ELEMS and (variant == bc.S or N >= 2)
        for n in (nx, 1):
            for b in bc.RAW_BS:
                assert any(c[:3] == (b, n, m) for c in raw), f"raw: no case with B = {b}, N = {n}, M = {m}"
    assert bc.RAW_BS == (1, 3, 2100) and len(raw) == len(set(raw)) == len(ms) * 2 * 3
    for b in bc.RAW_BS:
        assert {c[3] for c in raw if c[0] == b} == {4, 36, 252, 256}, f"raw: B = {b} misses a D"
        assert {c[3] for c in raw if c[0] == b and c[1] > 1} >= {4, 36}, f"raw: B = {b} at the largest N"
    assert all((c[4] == bc.C) == (c[1] >= 2 and c[0] < 2100) for c in raw)


def test_cos_cases_take_both_routes(lib):
    for B, N, M, D in bc.COS_CASES:
        big = lib.ge2e_cos_sim_workspace_bytes(B, N, M, D)
        small = lib.ge2e_workspace_bytes(B, N, M, D, 0, IMPL["generic"])
        assert big >= small > 0 and big % 256 == 0 and small % 256 == 0
    assert (1, 16, 3, 64) in bc.COS_CASES                                          # the header's edge: N = 16, D % 64 == 0
    exact = [c for c in bc.COS_CASES if lib.ge2e_cos_sim_workspace_bytes(*c) > lib.ge2e_workspace_bytes(*c, 0, IMPL["generic"])]
    # where the matrix-core size is the larger one the workspace ends with tiled_layout's last region: the guard can bite
    assert any(B == 1 and N == 16 and D % 64 == 0 for B, N, M, D in exact), exact
    assert any((N * M) % 64 != 0 and N >= 16 and D % 64 == 0 for _, N, M, D in exact), exact
    assert any(N < 16 for _, N, M, D in bc.COS_CASES)


@pytest.mark.parametrize("case", bc.LOSS_CASES, ids=bc.case_id)
def test_reference_is_finite_and_contrast_does_not_tie(case):
    ref = bc.loss_reference(case)
    for k in ("loss", "per", "dE", "dw", "db"):
        assert np.isfinite(ref[k]).all(), f"{case}: {k}"
    if case[5] == bc.C:
        assert bc.top2_gap_ok(ref, case[2]), f"{case}: two largest other-speaker similarities tie; change the seed"


@pytest.mark.parametrize("case", bc.RAW_CASES, ids=bc.raw_id)
def test_raw_reference_is_finite_and_contrast_does_not_tie(lib, case):
    c = bc.resolve_raw(lib, case)
    Y, src = bc.raw_inputs(c)
    for s in (src, None):
        ref = bc.raw_reference(c, Y, s)
        for k in ("loss", "per", "dY", "dw", "db"):
            assert np.isfinite(ref[k]).all(), f"{c}: {k}"
        if c[4] == bc.C:
            assert bc.top2_gap_ok(ref, c[1]), f"{c}: two largest other-speaker similarities tie; change the seed"
    assert all(sorted(row) == list(range(c[1] * c[2])) for row in src[:3])
    assert c[0] == 1 or not np.array_equal(src[0], src[1]) or c[1] * c[2] <= 2
