"""GPU: score normalisation against a cohort (ge2e_cohort_stats, ge2e_selftest_cohort_stats_chunk,
ge2e_verify_scores_normed, functional.cohort_stats / verify_scores_normed, evaluation.SpeakerBank.set_cohort and
normalize=True).

References, never the code under test: tests/snorm_ref.py (numpy) applied to two score matrices -- the fp32 matrix that
ge2e_verify_scores, a kernel of the parent commit, returns for the same rows against the cohort (the multiset rule, the
row maximum, the float32 restatement of the normalisation: bit for bit where the rule fixes the bits), and the float64
enroll_ref.scores_ref (the gate g = 3e-6 of tests/test_gpu_enroll.py on the scores, 2 g on mean and spread, and their
first-order propagation through the normalisation on the cases tests/test_snorm_cpu.py licenses).  The C-ABI tests call
through ctypes on the guarded buffers of tests/guarded.py: inputs between guards, NaN in everything that must not be read,
outputs poisoned, the workspace exactly the advertised size between guard bands.  `-s` prints every figure before it is
asserted.
"""
import numpy as np
import pytest
import torch

import enroll_cases as ec
import enroll_ref as er
import snorm_cases as sc
import snorm_ref as sr
from capi import GF, lib  # noqa: F401
from guarded import Buf, IntBuf, Workspace, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = ec.GATE
EPS, EPS_COS, EPS_STD = er.EPS, er.EPS_COS, sc.EPS_STD
NAMES = list(ec.VALUE_CASES)
UNIT = np.float32([0, 1])


# ---- the calls on guarded buffers ------------------------------------------------------------------------------------------
def run_stats(lib, X, sel, sel_min, cohort, ccnt, n_top, chunk=None, pattern=0xFF):
    """One ge2e_cohort_stats call (`chunk`: ge2e_selftest_cohort_stats_chunk with that many rows) -> stats (R, 2)."""
    X, cohort, ccnt = np.array(X, dtype=np.float32), np.array(cohort, dtype=np.float32), np.array(ccnt, dtype=np.int32)
    (R, D), C = X.shape, len(ccnt)
    what = f"cohort_stats C{C} R{R} D{D} n{n_top} chunk {chunk} fill {pattern:#04x}"
    x, m, c, out = Buf(X.shape, X), Buf(cohort.shape, cohort), IntBuf((C,), ccnt), Buf((R, 2))
    s = IntBuf((R,), np.array(sel, dtype=np.int32)) if sel is not None else None
    nbytes = int(lib.ge2e_cohort_stats_workspace_bytes(C, R, D, n_top) if chunk is None
                 else lib.ge2e_selftest_cohort_stats_workspace_bytes(C, R, D, n_top, chunk))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Workspace(nbytes, pattern)
    args = (x.ptr, s.ptr if s else None, sel_min, m.ptr, c.ptr, C, R, D, n_top, EPS_COS, EPS, EPS_STD, out.ptr, ws.ptr, nbytes, None)
    code = lib.ge2e_cohort_stats(*args) if chunk is None else lib.ge2e_selftest_cohort_stats_chunk(*args, chunk)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    ws.check(what)
    stats = out.get(what, finite=False)
    assert all(b.guards_intact() for b in (x, m, c) + ((s,) if s else ())), f"{what}: an input's guard"
    assert same_bits(x.get(what + " X", finite=False), X) and same_bits(m.get(what + " cohort", finite=False), cohort)
    return stats


def verify_matrix(lib, E, labels, models, cnt, thr=None):
    """ge2e_verify_scores, a kernel of the parent commit, for the same inputs -> scores (R, K)[, counts, trials]."""
    E, models, cnt = np.array(E, dtype=np.float32), np.array(models, dtype=np.float32), np.array(cnt, dtype=np.int32)
    (R, D), K = E.shape, len(cnt)
    e, m, c, s = Buf(E.shape, E), Buf(models.shape, models), IntBuf((K,), cnt), Buf((R, K))
    lab = IntBuf((R,), np.array(labels, dtype=np.int32)) if labels is not None else None
    T = len(thr) if thr is not None else 0
    t = Buf((T,), np.asarray(thr, dtype=np.float64).astype(np.float32)) if T else None
    counts, trials = (IntBuf((T, 2)), IntBuf((2,))) if T else (None, None)
    code = lib.ge2e_verify_scores(e.ptr, lab.ptr if lab else None, m.ptr, c.ptr, K, R, D, EPS_COS, EPS, t.ptr if T else None, T, s.ptr,
                                  counts.ptr if T else None, trials.ptr if T else None, None)
    torch.cuda.synchronize()
    assert code == 0
    scores = s.get("verify_scores", finite=False)
    return (scores, counts.get("counts"), trials.get("trials")) if T else scores


def run_normed(lib, E, labels, models, cnt, row_stats, model_stats, thr=None, need_scores=True, offset=0):
    """One ge2e_verify_scores_normed call -> dict of numpy outputs (scores, counts, trials)."""
    E, models, cnt = np.array(E, dtype=np.float32), np.array(models, dtype=np.float32), np.array(cnt, dtype=np.int32)
    (R, D), K = E.shape, len(cnt)
    T = len(thr) if thr is not None else 0
    what = f"verify_scores_normed K{K} R{R} D{D} T{T} scores {need_scores} offset {offset}"
    e, m, c = Buf(E.shape, E), Buf(models.shape, models), IntBuf((K,), cnt)
    rs, ms = Buf((R, 2), np.array(row_stats, dtype=np.float32)), Buf((K, 2), np.array(model_stats, dtype=np.float32))
    lab = IntBuf((R,), np.array(labels, dtype=np.int32)) if labels is not None else None
    t = Buf((T,), np.asarray(thr, dtype=np.float64).astype(np.float32)) if T else None
    outs = {}
    if need_scores:
        outs["scores"] = Buf((R, K), offset=offset)
    if T:
        outs["counts"] = IntBuf((T, 2))
    if lab is not None:
        outs["trials"] = IntBuf((2,))
    ptr = lambda b: b.ptr if b is not None else None  # noqa: E731
    code = lib.ge2e_verify_scores_normed(e.ptr, ptr(lab), m.ptr, c.ptr, K, R, D, EPS_COS, EPS, rs.ptr, ms.ptr, ptr(t), T,
                                         ptr(outs.get("scores")), ptr(outs.get("counts")), ptr(outs.get("trials")), None)
    torch.cuda.synchronize()
    assert code == 0, f"{what} returned {code}"
    res = {key: (b.get(f"{what} {key}", finite=False) if key == "scores" else b.get(f"{what} {key}")) for key, b in outs.items()}
    assert all(b.guards_intact() for b in (e, m, c, rs, ms)), f"{what}: an input's guard"
    return res


_banks = {}


def bank_of(GF, name):
    """-> cnt, models: the case's bank as the library fills it over the case's two calls: made once, read-only."""
    if name not in _banks:
        c = ec.case(name)
        dev = torch.device(DEV)
        sums = torch.zeros(c["K"], c["D"], device=dev)
        cnt = torch.zeros(c["K"], dtype=torch.int32, device=dev)
        for E, lab in c["calls"]:
            GF.enroll_accumulate(sums, cnt, torch.as_tensor(np.nan_to_num(E), device=dev), torch.as_tensor(np.array(lab), device=dev))
        models = GF.enroll_finalize(sums, cnt).cpu().numpy()
        cnt = cnt.cpu().numpy()
        assert np.array_equal(cnt, c["cnt"])
        models[cnt <= 0] = np.nan        # the model of a speaker that is not enrolled must not matter anywhere below
        for a in (cnt, models):
            a.setflags(write=False)
        _banks[name] = cnt, models
    return _banks[name]


_stats = {}


def lib_stats(GF, lib, name, n_top):
    """-> (row stats, model stats) of the case as the library computes them: made once, read-only."""
    if (name, n_top) not in _stats:
        c, s = ec.case(name), sc.case(name)
        cnt, models = bank_of(GF, name)
        rows = run_stats(lib, c["E"], c["labels"], 0, s["cohort"], s["ccnt"], n_top)
        mods = run_stats(lib, models, cnt, 1, s["cohort"], s["ccnt"], n_top)
        rows.setflags(write=False)
        mods.setflags(write=False)
        _stats[name, n_top] = rows, mods
    return _stats[name, n_top]


def is_unit(stats):
    return same_bits(np.ascontiguousarray(stats), np.tile(UNIT, (len(stats), 1)))


# ---- 1. cohort_stats against float64 and against the library's own matrix ---------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_stats_against_float64_and_the_verify_matrix(GF, lib, name):
    c, s = ec.case(name), sc.case(name)
    cnt, models = bank_of(GF, name)
    member, members = s["member"], int(s["member"].sum())
    sides = {"rows": (c["E"], c["labels"], 0, c["labels"] >= 0), "models": (models, cnt, 1, cnt > 0)}
    for side, (X, sel, sel_min, scored) in sides.items():
        matrix = verify_matrix(lib, X, np.where(scored, 0, -1), s["cohort"], s["ccnt"])   # (NaN rows are ignored rows there)
        assert not matrix[:, ~member].any() and not matrix[~scored].any()
        got = {}
        for n_top in sc.n_tops(name):
            ref = sc.stats_ref(name, n_top)[0 if side == "rows" else 1]
            g = got[n_top] = run_stats(lib, X, sel, sel_min, s["cohort"], s["ccnt"], n_top)
            err = np.abs(g[scored] - ref[scored]).max(0) if scored.any() else np.zeros(2)
            print(f"{name} {side} n_top {n_top}: max|mean - ref| {err[0]:.2e}, max|std - ref| {err[1]:.2e} / {2 * GATE:.0e}")
            assert np.isfinite(g).all(), f"{name} {side} n_top {n_top}: NaN poison (or a NaN result) in stats"
            assert err[0] <= 2 * GATE and err[1] <= 2 * GATE, f"{name} {side} n_top {n_top}"
            assert is_unit(g[~scored]), f"{name} {side}: a row that is not scored does not hold (+0, 1)"
            # the multiset rule on the library's own fp32 scores: only the rounding of the sums is left
            own = sr.cohort_stats_ref(matrix, member, n_top, scored)
            assert np.abs(g - own).max() <= GATE, f"{name} {side} n_top {n_top}: {np.abs(g - own).max():.3e} from the multiset rule"
        # n_top = 1: the row maximum over the members, bit for bit, and the floor
        best = matrix[:, member].max(1)
        assert same_bits(np.ascontiguousarray(got[1][scored, 0]), np.ascontiguousarray(best[scored])), f"{name} {side}: n_top 1"
        assert (got[1][scored, 1] == np.float32(EPS_STD)).all()
        # n above the member count: the whole cohort
        assert same_bits(got[members + 10], got[members]) and (members >= 64 or same_bits(got[64], got[members]))


# ---- 2. ties, inf, no members, rows that are not scored ---------------------------------------------------------------------
def test_tie_cohort_follows_the_multiset_rule(lib):
    t = sc.tie_cohort()
    scored = t["labels"] >= 0
    matrix = verify_matrix(lib, t["E"], t["labels"], t["cohort"], t["ccnt"])
    near = np.arange(sc.TIE_ROWS)
    assert all(same_bits(np.ascontiguousarray(matrix[:, 3]), np.ascontiguousarray(matrix[:, at])) for at in sc.TIE_AT)
    assert (matrix[near][:, t["member"]].max(1) == matrix[near, 3]).all()
    cuts = 0
    for n_top in (1, 2, 3, 4, 11, 14, 18, 26, 64, 113):   # (the tied score is a row's 11th, 14th, 18th, 26th, 63rd somewhere)
        got = run_stats(lib, t["E"], t["labels"], 0, t["cohort"], t["ccnt"], n_top)
        own = sr.cohort_stats_ref(matrix, t["member"], n_top, scored)
        cut = sr.cut_through_tie(matrix, t["member"], n_top) & scored
        cuts += int(cut.sum())
        print(f"tie cohort n_top {n_top}: {int(cut.sum())} rows cut through a tie; max distance from the rule {np.abs(got - own).max():.2e}")
        assert np.abs(got - own).max() <= GATE and is_unit(got[~scored])
        if n_top <= 2:      # one or two of three bit-equal best scores: the mean is that score, the spread the floor
            assert cut[near].all()
            assert same_bits(np.ascontiguousarray(got[near, 0]), np.ascontiguousarray(matrix[near, 3]))
            assert (got[near, 1] == np.float32(EPS_STD)).all()
    assert cuts > 2 * sc.TIE_ROWS, "no boundary beyond the two hand-made ones cut through the tie"


def test_inf_member_stands_behind_every_number(lib):
    i = sc.inf_cohort()
    scored = i["labels"] >= 0
    matrix = verify_matrix(lib, i["E"], i["labels"], i["cohort"], i["ccnt"])
    assert np.isnan(matrix[scored, 2]).all() and np.isfinite(matrix[scored][:, np.arange(17) != 2]).all()
    members = i["finite"] + 1
    for n_top in (1, 5, i["finite"]):
        got = run_stats(lib, i["E"], i["labels"], 0, i["cohort"], i["ccnt"], n_top)
        assert np.isfinite(got).all() and np.abs(got - sr.cohort_stats_ref(matrix, i["member"], n_top, scored)).max() <= GATE
    for n_top in (members, members + 10):
        got = run_stats(lib, i["E"], i["labels"], 0, i["cohort"], i["ccnt"], n_top)
        assert np.isnan(got[scored]).all() and is_unit(got[~scored]), f"n_top {n_top}: the NaN score is among the n"


def test_no_members_rows_not_scored_and_rows_never_read(lib):
    e = sc.empty_cohort()
    for n_top in (1, 300):
        assert is_unit(run_stats(lib, np.nan_to_num(e["E"]), None, 0, e["cohort"], e["ccnt"], n_top)), "a cohort without members"
    name = "K130_D36_R65"
    c, s = ec.case(name), sc.case(name)
    E, lab = c["E"], c["labels"]
    assert np.isnan(E[lab < 0]).all() and (lab < 0).sum() >= 3
    base = run_stats(lib, E, lab, 0, s["cohort"], s["ccnt"], 5)
    assert is_unit(base[lab < 0]) and np.isfinite(base).all()
    filled = E.copy()
    filled[lab < 0] = 0.25
    assert same_bits(run_stats(lib, filled, lab, 0, s["cohort"], s["ccnt"], 5), base), "an ignored row is read"
    top = run_stats(lib, E, lab, 2 ** 31 - 1, s["cohort"], s["ccnt"], 5)          # only the row labelled INT_MAX is left
    assert (lab == ec.I32_MAX).sum() == 1 and is_unit(top[lab != ec.I32_MAX]) and same_bits(top[lab == ec.I32_MAX], base[lab == ec.I32_MAX])
    # a selector is compared, not used: sel_min picks other rows
    some = run_stats(lib, np.nan_to_num(E), np.arange(c["R"]), 40, s["cohort"], s["ccnt"], 5)
    assert is_unit(some[:40]) and same_bits(np.ascontiguousarray(some[40:][lab[40:] >= 0]), np.ascontiguousarray(base[40:][lab[40:] >= 0]))


@pytest.mark.parametrize("C", [2048, 2049, 6144, 6145])
def test_every_form_of_the_select_kernel(lib, C):
    """Up to 2 048 and up to 6 144 columns a row's keys stay in registers (8 and 24 per thread); above that every pass
    reads them from the workspace: either side of both thresholds, against the multiset rule on the library's own matrix."""
    D, R = 8, 9
    cohort, ccnt = sc.make_cohort(C, D, 300 + C)
    rng = np.random.default_rng(C)
    X = ec.unit_rows(rng, rng.standard_normal((R, D)), np.arange(R))
    sel = np.arange(R) % 4 - 1                             # rows 0, 4, 8 are not scored
    X[sel < 0] = np.nan
    scored, member = sel >= 0, ccnt > 0
    matrix = verify_matrix(lib, X, sel, cohort, ccnt)
    for n_top in (1, 300, 3000):
        got = run_stats(lib, X, sel, 0, cohort, ccnt, n_top)
        own = sr.cohort_stats_ref(matrix, member, n_top, scored)
        print(f"C {C} n_top {n_top}: max distance from the rule {np.abs(got - own).max():.2e}")
        assert np.abs(got - own).max() <= GATE and is_unit(got[~scored])
        assert same_bits(run_stats(lib, X, sel, 0, cohort, ccnt, n_top, chunk=64, pattern=0x00), got)
    one = run_stats(lib, X, sel, 0, cohort, ccnt, 1)
    assert same_bits(np.ascontiguousarray(one[scored, 0]), np.ascontiguousarray(matrix[scored][:, member].max(1)))


# ---- 3. the same bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K130_D256_R130", "K16_D100_R130", "K67_D260_R64"])
def test_same_bits_over_chunks_fills_launches_and_row_order(GF, lib, name):
    c, s = ec.case(name), sc.case(name)
    cnt, models = bank_of(GF, name)
    E, lab, R = c["E"], c["labels"], c["R"]
    for n_top in (2, 64):
        base = run_stats(lib, E, lab, 0, s["cohort"], s["ccnt"], n_top)
        assert same_bits(run_stats(lib, E, lab, 0, s["cohort"], s["ccnt"], n_top, pattern=0x00), base), "the workspace's contents matter"
        assert same_bits(run_stats(lib, E, lab, 0, s["cohort"], s["ccnt"], n_top), base), "launch to launch"
        for chunk in (64, 128):      # R = 130: three chunks of 64 rows, two of 128; R = 64: one
            for pattern in (0xFF, 0x00):
                again = run_stats(lib, E, lab, 0, s["cohort"], s["ccnt"], n_top, chunk=chunk, pattern=pattern)
                assert same_bits(again, base), f"{name} n_top {n_top}: chunk {chunk}, fill {pattern:#04x} gives other bits"
        perm = np.random.default_rng(9).permutation(R)
        for chunk in (None, 64):
            moved = run_stats(lib, E[perm], lab[perm], 0, s["cohort"], s["ccnt"], n_top, chunk=chunk)
            assert same_bits(moved, base[perm]), "a row's statistics depend on its place"
        # the bank's models through sel = cnt, 1 against the enrolled subset on its own
        whole = run_stats(lib, models, cnt, 1, s["cohort"], s["ccnt"], n_top)
        subset = run_stats(lib, models[cnt > 0], None, 0, s["cohort"], s["ccnt"], n_top)
        assert same_bits(np.ascontiguousarray(whole[cnt > 0]), subset) and is_unit(whole[cnt <= 0])
    assert R <= 64 or -(-R // 64) == 3


# ---- 4. verify_scores_normed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_normed_scores_are_the_float32_restatement_bit_for_bit(GF, lib, name):
    c = ec.case(name)
    cnt, models = bank_of(GF, name)
    E, lab, K = c["E"], c["labels"], c["K"]
    scored, enrolled = lab >= 0, cnt > 0
    matrix = verify_matrix(lib, E, lab, models, cnt)
    members = int(sc.case(name)["member"].sum())
    for n_top in sorted({1, 2, 5, members}):
        rs, ms = lib_stats(GF, lib, name, n_top)
        want = sr.normed_f32(matrix, rs, ms, scored, enrolled)
        thr = sc.normed_thresholds(50)
        base = run_normed(lib, E, lab, models, cnt, rs, ms, thr=thr)
        assert same_bits(base["scores"], want), f"{name} n_top {n_top}: {(base['scores'].view(np.uint32) != want.view(np.uint32)).sum()} elements differ"
        shifted = run_normed(lib, E, lab, models, cnt, rs, ms, offset=1)          # scores one float off a 16-byte boundary
        assert same_bits(shifted["scores"], want) and set(shifted) == {"scores", "trials"}
        # counts and trials: counted in numpy on the library's own normalised matrix
        for T in (1, 50, 257):
            thr = sc.normed_thresholds(T)
            got = run_normed(lib, E, lab, models, cnt, rs, ms, thr=thr) if T != 50 else base
            counts, trials = er.counts_ref(want, lab, cnt, thr)
            assert np.array_equal(got["counts"], counts) and np.array_equal(got["trials"], trials), f"{name} n_top {n_top} T {T}"
            only = run_normed(lib, E, lab, models, cnt, rs, ms, thr=thr, need_scores=False)
            assert set(only) == {"counts", "trials"} and np.array_equal(only["counts"], counts) and np.array_equal(only["trials"], trials)
        # NaN in the statistics of ignored rows and of speakers that are not enrolled changes nothing
        rs2, ms2 = rs.copy(), ms.copy()
        rs2[~scored], ms2[~enrolled] = np.nan, np.nan
        again = run_normed(lib, E, lab, models, cnt, rs2, ms2, thr=sc.normed_thresholds(50))
        assert all(np.array_equal(again[k].view(np.int32), base[k].view(np.int32)) for k in base)
    assert K % 4 or name.startswith("K16_")


@pytest.mark.parametrize("name", NAMES)
def test_unit_tables_give_verify_scores_bits(GF, lib, name):
    c = ec.case(name)
    cnt, models = bank_of(GF, name)
    E, lab, K, R = c["E"], c["labels"], c["K"], c["R"]
    thr = ec.thresholds_of(50)
    scores, counts, trials = verify_matrix(lib, E, lab, models, cnt, thr=thr)
    got = run_normed(lib, E, lab, models, cnt, np.tile(UNIT, (R, 1)), np.tile(UNIT, (K, 1)), thr=thr)
    assert same_bits(got["scores"], scores) and np.array_equal(got["counts"], counts) and np.array_equal(got["trials"], trials)
    plain = run_normed(lib, np.nan_to_num(E), None, models, cnt, np.tile(UNIT, (R, 1)), np.tile(UNIT, (K, 1)))   # no labels
    assert set(plain) == {"scores"} and same_bits(plain["scores"], verify_matrix(lib, np.nan_to_num(E), None, models, cnt))


@pytest.mark.parametrize("name", NAMES)
def test_normed_scores_against_float64(GF, lib, name):
    c = ec.case(name)
    cnt, models = bank_of(GF, name)
    E, lab = c["E"], c["labels"]
    scored, enrolled = lab >= 0, cnt > 0
    compared = 0
    for n_top in sc.n_tops(name):
        if not sc.licensed(name, n_top):
            continue
        lo = sc.assert_licence(name, n_top)                 # (asserted on the CPU too, before anything is launched)
        rs64, ms64 = sc.stats_ref(name, n_top)
        ref = sr.normed_f64(c["scores"], rs64, ms64, scored, enrolled)
        bound = sr.normed_bound(c["scores"], rs64, ms64, scored, enrolled, GATE)
        rs, ms = lib_stats(GF, lib, name, n_top)
        got = run_normed(lib, E, lab, models, cnt, rs, ms)["scores"]
        err = np.abs(got - ref)
        worst = float((err / bound).max())
        print(f"{name} n_top {n_top}: smallest spread {lo:.2e}; max|normed - ref| {err.max():.2e}, at most {worst:.3f} of its bound")
        assert (err <= bound).all(), f"{name} n_top {n_top}: {worst:.3f} of the bound"
        compared += 1
    assert compared or sc.taken(name, 10 ** 6) < 5


# ---- 5. the chain in a graph, and the Python surface ------------------------------------------------------------------------
def cohort_bank(EV, name, dev):
    s = sc.case(name)
    bank = EV.SpeakerBank(s["C"], s["cohort"].shape[1], dev)
    member = np.flatnonzero(s["member"])
    bank.enroll(torch.as_tensor(np.array(s["cohort"][member]), device=dev), member.tolist())   # one row each: the model is the row
    return bank


def test_graph_capture_replayed_on_other_rows_and_labels(GF):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    dev = torch.device(DEV)
    name = "K17_D7_R63"
    c = ec.case(name)
    K, D, R = c["K"], c["D"], c["R"]
    E1, lab1 = c["calls"][0]
    e1 = torch.as_tensor(np.nan_to_num(E1), device=dev)
    l1 = torch.as_tensor(np.array(lab1), device=dev)
    coh = cohort_bank(EV, name, dev)
    cmodels, ccnt = coh.models(), coh.cnt
    thr = torch.as_tensor(sc.normed_thresholds(50).astype(np.float32), device=dev)
    perm = np.random.default_rng(78).permutation(R)
    rows_a, lab_a = np.nan_to_num(c["E"]), np.array(c["labels"])
    rows_b, lab_b = rows_a[perm] * np.float32(1.5), np.roll(np.array(c["labels"]), 5)[perm]
    et = torch.zeros(R, D, device=dev)
    tl = torch.full((R,), -1, dtype=torch.int32, device=dev)
    sums = torch.zeros(K, D, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)

    def chain():
        sums.zero_()
        cnt.zero_()
        GF.enroll_accumulate(sums, cnt, e1, l1)
        models = GF.enroll_finalize(sums, cnt)
        ms = GF.cohort_stats(models, cmodels, ccnt, n_top=5, select=cnt, select_min=1)
        rs = GF.cohort_stats(et, cmodels, ccnt, n_top=5, select=tl, select_min=0)
        return GF.verify_scores_normed(et, models, cnt, rs, ms, labels=tl, thresholds=thr)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = chain()
    for rows, labs in ((rows_a, lab_a), (rows_b, lab_b)):
        et.copy_(torch.as_tensor(rows, device=dev))
        tl.copy_(torch.as_tensor(labs, device=dev))
        out.scores.fill_(float("nan"))
        out.counts.fill_(-7)
        out.trials.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = {key: getattr(out, key).cpu().numpy().copy() for key in ("scores", "counts", "trials")}
        eager = chain()
        torch.cuda.synchronize()
        for key in got:
            assert np.array_equal(got[key].view(np.int32), getattr(eager, key).cpu().numpy().view(np.int32)), f"replay differs: {key}"
        assert got["trials"].sum() > 0 and not got["scores"][labs < 0].any() and np.isfinite(got["scores"]).all()
        assert 0 < got["counts"][0].sum() and (got["counts"][:-1] >= got["counts"][1:]).all()
    assert not np.array_equal(lab_a, lab_b)


def test_speaker_bank_normalize_equals_the_functional_chain(GF):
    from speaker_embedding_ge2e_loss_amd import evaluation as EV
    dev = torch.device(DEV)
    name = "K130_D36_R65"
    c = ec.case(name)
    K, D = c["K"], c["D"]
    coh = cohort_bank(EV, name, dev)
    bank = EV.SpeakerBank(K, D, dev)
    (Ea, la), (Eb, lb) = c["calls"]
    bank.enroll(torch.as_tensor(np.nan_to_num(Ea), device=dev), la.tolist())
    e = torch.as_tensor(np.nan_to_num(c["E"]), device=dev)
    ids = torch.as_tensor(np.array(c["labels"]), device=dev)
    thr = sc.normed_thresholds(50).tolist()
    with pytest.raises(ValueError, match="cohort"):
        bank.verify(e, ids, thresholds=thr, normalize=True)
    raw = bank.verify(e, ids)                                      # the defaults keep today's results
    bank.set_cohort(coh, n_top=5)
    assert torch.equal(bank.verify(e, ids).scores, raw.scores) and torch.equal(bank.score(e), GF.verify_scores(e, bank.models(), bank.cnt).scores)

    def functional_chain():
        ms = GF.cohort_stats(bank.models(), coh.models(), coh.cnt, n_top=5, select=bank.cnt, select_min=1)
        rs = GF.cohort_stats(e, coh.models(), coh.cnt, n_top=5, select=ids, select_min=0)
        return ms, GF.verify_scores_normed(e, bank.models(), bank.cnt, rs, ms, labels=ids, thresholds=thr)

    ms1, want = functional_chain()
    got = bank.verify(e, ids, thresholds=thr, normalize=True)
    assert torch.equal(got.scores, want.scores) and torch.equal(got.counts, want.counts) and torch.equal(got.trials, want.trials)
    assert torch.equal(bank.model_stats(), ms1) and not torch.equal(got.scores, raw.scores)
    only = bank.verify(e, ids, thresholds=thr, need_scores=False, normalize=True)
    assert only.scores is None and torch.equal(only.counts, want.counts)
    rs_all = GF.cohort_stats(e, coh.models(), coh.cnt, n_top=5)
    assert torch.equal(bank.score(e, normalize=True), GF.verify_scores_normed(e, bank.models(), bank.cnt, rs_all, ms1).scores)
    # the model-side statistics are recomputed after enroll
    bank.enroll(torch.as_tensor(np.nan_to_num(Eb), device=dev), lb.tolist())
    assert bank._model_stats is None
    ms2, want2 = functional_chain()
    got2 = bank.verify(e, ids, thresholds=thr, normalize=True)
    assert not torch.equal(ms2, ms1) and torch.equal(bank.model_stats(), ms2) and torch.equal(got2.scores, want2.scores)
    # a caller's workspace, and evaluate_enrolled with a cohort
    ws = torch.empty(int(GF._lib.load().ge2e_cohort_stats_workspace_bytes(coh.cnt.shape[0], e.shape[0], D, 5)) + 256, dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 256:]
    assert torch.equal(GF.cohort_stats(e, coh.models(), coh.cnt, n_top=5, workspace=ws), rs_all)
    enroll = [(torch.as_tensor(np.nan_to_num(E))[:, None, :], l.tolist()) for E, l in c["calls"]]
    trials = [(torch.as_tensor(np.nan_to_num(c["E"]))[:, None, :], c["labels"].tolist())]
    r = EV.evaluate_enrolled(lambda x: x[:, 0, :], enroll, trials, K, device=DEV, thresholds=thr, verbose=False, cohort=coh, n_top=5)
    assert r["n_imp"] == int(got2.trials[0]) and r["n_tgt"] == int(got2.trials[1]) and 0 <= r["EER"] <= 1
    with pytest.raises(ValueError, match="thresholds"):
        EV.evaluate_enrolled(lambda x: x[:, 0, :], enroll, trials, K, device=DEV, verbose=False, cohort=coh)
