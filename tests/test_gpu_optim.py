"""GPU: the native optimizer step (ge2e_sgd_clip_step, functional.sgd_layout / sgd_clip_step, optim.ClipSGD,
DPTrainer(native_step=True)) against tests/optim_ref.py.

The C ABI is called with raw pointers on guarded buffers (tests/guarded.py): every parameter a buffer of its own between
NaN guards, the gradient bucket and the momentum buffer between NaN guards with NaN in the gaps between segments, the tables
between sentinels, the workspace of exactly the advertised size between byte guards.  The default case has the segment sizes
1, 1, 3, 5, 4095, 4096, 4097, 8193 over two groups: a one-element tensor, a tail, an exact chunk, a chunk plus one, a
multi-chunk tensor.  Their gradients start 0, 4, 8 and 12 bytes past a 16-byte boundary; two parameters (5 and 4097
elements) are NOT congruent to their gradients mod 16 and take the word-at-a-time path, the others peel to the boundary.

Norm and coefficient are compared with the float64 oracle at rtol 1e-5.  Every term is a square, so the relative error of
a sum is at most (additions on one element's path + 1) 2^-24 and the square root halves it; 1e-5 covers 160 additions.
THE IMPLEMENTATION'S PATH: launch 1 adds at most 16 elements a thread (a full chunk: four 16-byte pieces), then a butterfly
of 6 and a tree of 2 -- 24; launch 2 adds ceil(chunks of the group / 256) partials a thread, then the same 8 -- 9 here, 10
with 300 chunks, 104 for 10^8 parameters in one group: 33 additions here, 128 there.
The update is compared BIT FOR BIT with the float32 emulation, given the call's own coef output."""
import numpy as np
import pytest
import torch

import optim_ref as orf
import trainer_fixtures as tfx
from capi import GF, lib, ok  # noqa: F401
from guarded import Buf, IntBuf, Workspace, same_bits

pytestmark = pytest.mark.gpu
NAN = np.float32(np.nan)
SIZES = (1, 1, 3, 5, 4095, 4096, 4097, 8193)
GROUP_OF = (0, 1, 0, 1, 0, 1, 1, 0)
GAPS = {6: 1}                      # elements left out of the bucket in front of a tensor: the offsets mod 4 become 0 1 2 1 2 1 2 3
INCONGRUENT = (3, 6)               # parameters one word off their gradient's position in a 16-byte line
U24 = 2.0 ** -24
ZERO_GRAD, SKIP_NONFINITE = 1, 2


class Case:
    """Tensors of `sizes` in groups `group_of` (any order: the table is sorted by group, the bucket is not), on guarded
    buffers; the host copies `p`, `g`, `m` follow the device."""

    def __init__(self, lib, sizes=SIZES, group_of=GROUP_OF, G=2, gaps=GAPS, incongruent=INCONGRUENT, seed=0, momentum=False,
                 mom_offset=0, amp=1.0, same_sign=False, one_buffer=False):
        self.lib, self.sizes, self.group_of, self.G, self.n = lib, tuple(sizes), tuple(group_of), G, len(sizes)
        self.rng = np.random.default_rng(seed)
        self.same_sign, self.one_buffer = same_sign, one_buffer
        self.off, at = [], 0
        for i, n in enumerate(sizes):
            at += gaps.get(i, 0)
            self.off.append(at)
            at += n
        self.total = at
        self.sign = [np.where(self.rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32) for n in sizes]
        self.p = [self._draw(i, 1.0, 0.5) for i in range(self.n)]
        self.g = self.new_grads(amp)
        self.m = [np.zeros(n, np.float32) for n in sizes] if momentum else None
        if one_buffer:                                   # adjacent parameters in one buffer (many one-element tensors)
            self.arena = Buf((sum(sizes),), np.concatenate(self.p))
            starts = np.cumsum((0,) + self.sizes[:-1])
            self.pt = [self.arena.t[a:a + n] for a, n in zip(starts, sizes)]
            self.pbufs = [self.arena]
        else:
            self.pbufs = [Buf((n,), self.p[i], offset=(self.off[i] + (i in incongruent)) % 4) for i, n in enumerate(sizes)]
            self.pt = [b.t for b in self.pbufs]
        self.grad = Buf((self.total,), self._flat(self.g))
        self.mom = Buf((self.total,), self._flat(self.m), offset=mom_offset) if momentum else None
        order = sorted(range(self.n), key=lambda i: self.group_of[i])
        self.order = order
        counts = orf.chunk_counts([sizes[i] for i in order])
        self.chunk_start = [0] + np.cumsum(counts).tolist()
        self.S, self.C = self.n, self.chunk_start[-1]
        self.d_seg = IntBuf((self.S, 4), [[self.pt[i].data_ptr(), self.off[i], sizes[i], group_of[i]] for i in order], dtype=torch.int64)
        self.d_chunk = IntBuf((self.S + 1,), self.chunk_start)
        self.hyper = Buf((G, 4), np.zeros((G, 4), np.float32))
        self.stats = Buf((G, 2))
        self.skipped = IntBuf((1,), [0])
        self.ws = Workspace(lib.ge2e_sgd_clip_workspace_bytes(self.C))
        assert self.ws.nbytes == -(-4 * self.C // 256) * 256

    def _draw(self, i, scale, floor=0.0):
        x = self.rng.standard_normal(self.sizes[i]).astype(np.float32) * np.float32(scale)
        if self.same_sign:                              # |x| >= floor, the tensor's fixed sign pattern
            x = (np.abs(x) + np.float32(floor)) * self.sign[i]
        return x.astype(np.float32)

    def new_grads(self, amp=1.0):
        return [self._draw(i, amp) for i in range(self.n)]

    def _flat(self, parts):
        flat = np.full(self.total, NAN, np.float32)
        for o, x in zip(self.off, parts):
            flat[o:o + len(x)] = x
        return flat

    def _parts(self, flat, what):
        keep = np.ones(self.total, bool)
        for o, n in zip(self.off, self.sizes):
            keep[o:o + n] = False
        assert np.isnan(flat[keep]).all(), f"{what}: a gap between segments was written"
        return [flat[o:o + n].copy() for o, n in zip(self.off, self.sizes)]

    def set_grads(self, grads):
        self.g = [np.asarray(x, np.float32) for x in grads]
        self.grad.t.copy_(torch.from_numpy(self._flat(self.g)))

    def set_hyper(self, hyper):
        self.h = np.asarray(hyper, np.float32).reshape(self.G, 4)
        self.hyper.t.copy_(torch.from_numpy(self.h))

    def run(self, scale=1.0, flags=0, finite=True, stats=True):
        """One call; -> (before, after) host states as dicts of p, g, m; after also norm, coef, skipped."""
        before = dict(p=self.p, g=self.g, m=self.m)
        ok(self.lib.ge2e_sgd_clip_step(self.d_seg.ptr, self.d_chunk.ptr, self.S, self.C, self.G, self.grad.ptr,
                                       None if self.mom is None else self.mom.ptr, self.hyper.ptr, scale, flags,
                                       self.stats.ptr if stats else None, self.skipped.ptr if flags & SKIP_NONFINITE else None,
                                       self.ws.ptr, self.ws.nbytes, None), "ge2e_sgd_clip_step")
        self.ws.check("ge2e_sgd_clip_step")
        if self.one_buffer:
            flat = self.arena.get("parameters", finite=finite)
            starts = np.cumsum((0,) + self.sizes[:-1])
            self.p = [flat[a:a + n].copy() for a, n in zip(starts, self.sizes)]
        else:
            self.p = [b.get(f"parameter {i}", finite=finite) for i, b in enumerate(self.pbufs)]
        self.g = self._parts(self.grad.get("gradients", finite=False), "gradients")
        if self.mom is not None:
            self.m = self._parts(self.mom.get("momentum", finite=False), "momentum")
        st = self.stats.get("stats", finite=finite) if stats else np.full((self.G, 2), NAN, np.float32)
        for b in (self.d_seg, self.d_chunk, self.hyper, self.skipped):
            assert b.guards_intact()
        assert np.array_equal(self.d_seg.get("seg")[:, 1], [self.off[i] for i in self.order])
        assert same_bits(self.hyper.get("hyper", finite=False), self.h)
        after = dict(p=self.p, g=self.g, m=self.m, norm=st[:, 0].copy(), coef=st[:, 1].copy(),
                     skipped=int(self.skipped.get("skipped")[0]), partial=self.ws.t.view(torch.float32)[:self.C].cpu().numpy())
        return before, after

    def oracle(self, before, scale=1.0, **kw):
        return orf.step(before["p"], before["g"], before["m"], self.group_of, self.h.astype(np.float64), grad_scale=scale, **kw)

    def thresholds(self, factors, scale=1.0):
        """max_norm per group as a multiple of the group's true norm (below 1: the clip is active)."""
        return [float(np.float32(f * n)) for f, n in zip(factors, orf.norms(self.g, self.group_of, self.G, scale))]


def assert_same(got, want, what, nan_ok=False):
    for i, (a, b) in enumerate(zip(got, want)):
        if nan_ok:                                      # the NaN pattern and every other element's bits (payloads are the chip's own)
            na, nb = np.isnan(a), np.isnan(b)
            assert np.array_equal(na, nb), f"{what} {i}: NaN in other places"
            a, b = np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b)
        assert same_bits(a, b), f"{what} {i}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} elements differ"


def assert_emulated(case, before, after, scale=1.0, zero=False, skip=False, nan_ok=False):
    """The stored parameters, momentum and gradients are the float32 emulation's, from the call's own coefficients."""
    p, g, m = orf.emulate_f32(after["coef"], before["p"], before["g"], before["m"], case.group_of, case.h, scale, zero, skip)
    assert_same(after["p"], p, "parameter", nan_ok)
    assert_same(after["g"], g, "gradient", nan_ok)
    if m is not None:
        assert_same(after["m"], m, "momentum", nan_ok)


def assert_stats(after, ref):
    assert np.allclose(after["norm"], ref["norm"], rtol=1e-5, atol=0), (after["norm"], ref["norm"])
    assert np.allclose(after["coef"], ref["coef"], rtol=1e-5, atol=0), (after["coef"], ref["coef"])


def float64_bound(start, ref):
    """|dp| <= 2 (2^-24 |p'| + (1e-5 + 3 2^-24) lr |m'|) per element of the float64 result p' = p - lr m' (so lr |m'| is
    |p - p'|): the coefficient is good to 1e-5 (above), g2 takes two roundings and lr m' a third, the subtraction rounds once
    more, relative to p'; the factor 2 is slack.  With weight decay or momentum m' is a sum, and its error is bounded
    relative to the magnitudes of its TERMS: the cases that use the bound with them draw p, g and m with one sign per
    element, so that |m'| is that sum (each further term and addition brings 2^-24, inside the slack)."""
    return [2 * (U24 * np.abs(p) + (1e-5 + 3 * U24) * np.abs(np.asarray(p0, np.float64) - p)) for p0, p in zip(start, ref["params"])]


@pytest.mark.parametrize("factors", [(0.5, 0.25), (2.0, 4.0), (0.5, 2.0), (2.0, 0.5)], ids=["both", "neither", "first", "second"])
def test_norm_and_coefficient_against_float64(lib, factors):
    case = Case(lib, seed=1, amp=0.3)
    mx = case.thresholds(factors)
    case.set_hyper([[0.05, mx[0], 0, 0], [0.2, mx[1], 0, 0]])
    before, after = case.run()
    ref = case.oracle(before)
    assert_stats(after, ref)
    assert [bool(c < 1) for c in after["coef"]] == [f < 1 for f in factors] and (after["coef"] <= 1).all()
    assert_emulated(case, before, after)
    # every chunk's partial sum, with the 24 additions of launch 1 alone
    sq = [np.sum(np.asarray(before["g"][i][a:a + 4096], np.float64) ** 2) for i in case.order for a in range(0, case.sizes[i], 4096)]
    assert len(sq) == case.C == 11 and np.allclose(after["partial"], sq, rtol=25 * U24, atol=0)


def test_a_group_of_zero_gradients_is_left_alone(lib):
    case = Case(lib, seed=2)
    case.set_grads([x if k == 0 else np.zeros_like(x) for x, k in zip(case.g, case.group_of)])
    case.set_hyper([[0.05, 1.0, 0.01, 0], [0.2, 1.0, 0, 0]])
    before, after = case.run()
    assert after["norm"][1] == 0.0 and after["coef"][1] == 1.0 and after["coef"][0] < 1
    for i, k in enumerate(case.group_of):
        assert same_bits(after["p"][i], before["p"][i]) == (k == 1)
    assert_stats(after, case.oracle(before))
    assert_emulated(case, before, after)


COMBOS = [(0.0, 0.0, 0.0, 0), (0.9, 0.5, 0.0, 0), (0.0, 0.0, 0.01, 0), (0.9, 0.5, 0.01, 0), (0.9, 0.0, 0.01, 1)]
COMBO_IDS = ["plain", "momentum", "decay", "both", "both-buffer-off-line-second-group-without"]


@pytest.mark.parametrize("mu0,mu1,wd,mom_offset", COMBOS, ids=COMBO_IDS)
def test_update_bit_for_bit_over_two_steps(lib, mu0, mu1, wd, mom_offset):
    """grad_scale 0.25, a learning rate per group, the momentum buffer carried from the first step into the second; in the
    last combination the buffer lies one word off the bucket's lines (every segment a word at a time) and the second group
    has no momentum of its own (its m' = g3 is stored, its m is not read)."""
    case = Case(lib, seed=3, momentum=mu0 != 0, mom_offset=mom_offset)
    mx = case.thresholds((0.5, 2.0), 0.25)
    case.set_hyper([[0.05, mx[0], wd, mu0], [0.2, mx[1], 2 * wd, mu1]])
    for step in range(2):
        before, after = case.run(scale=0.25)
        assert_stats(after, case.oracle(before, 0.25))
        assert_emulated(case, before, after, scale=0.25)
        assert after["coef"][0] < 1 and (step == 1 or after["coef"][1] == 1)
        if case.m is not None and step == 1:
            assert all(np.abs(m).max() > 0 for m in before["m"])
        case.set_grads(case.new_grads(2.0))
    if mom_offset == 0:                                  # without `stats` the same update
        twin = Case(lib, seed=3, momentum=mu0 != 0)
        twin.set_hyper(case.h)
        _, quiet = twin.run(scale=0.25, stats=False)
        again = Case(lib, seed=3, momentum=mu0 != 0)
        again.set_hyper(case.h)
        _, loud = again.run(scale=0.25)
        assert_same(quiet["p"], loud["p"], "parameter without stats")


@pytest.mark.parametrize("mu0,mu1,wd,mom_offset", COMBOS[:4], ids=COMBO_IDS[:4])
def test_update_against_float64_within_the_derived_bound(lib, mu0, mu1, wd, mom_offset):
    """Two steps; the oracle restarts from the device's own state at each, so the bound is one step's."""
    case = Case(lib, seed=4, momentum=mu0 != 0, same_sign=True, amp=0.5)
    mx = case.thresholds((0.5, 2.0), 0.25)
    case.set_hyper([[0.05, mx[0], wd, mu0], [0.2, mx[1], 2 * wd, mu1]])
    for step in range(2):
        before, after = case.run(scale=0.25)
        ref = case.oracle(before, 0.25)
        worst = 0.0
        for got, want, bound in zip(after["p"], ref["params"], float64_bound(before["p"], ref)):
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), float((err / bound).max())
        print(f"step {step}: worst |dp| / bound = {worst:.3g}")
        assert all((np.sign(p) == s).all() for p, s in zip(after["p"], case.sign)), "a parameter changed sign: redraw the case"
        case.set_grads(case.new_grads(0.5))


def test_three_hundred_workgroups_agree_on_one_coefficient(lib):
    """300 one-element tensors in one group: C = 300 > 256, so the strided loop over the partials runs twice; every stored
    gradient must be g times ONE coef -- the emulation from the coef workgroup 0 reported."""
    n = 300
    case = Case(lib, sizes=(1,) * n, group_of=(0,) * n, G=1, gaps={}, incongruent=(), seed=5, one_buffer=True)
    assert case.C == n and case.chunk_start == list(range(n + 1))
    case.set_hyper([[0.1, case.thresholds((0.37,))[0], 0, 0]])
    before, after = case.run()
    assert_stats(after, case.oracle(before))
    assert after["coef"][0] < 0.5
    assert_emulated(case, before, after)
    assert np.allclose(after["partial"], np.concatenate(before["g"]).astype(np.float64) ** 2, rtol=2 * U24, atol=0)


def test_hyper_parameters_are_read_from_the_device(lib):
    case = Case(lib, seed=6)
    case.set_hyper([[0.05, 1.0, 0, 0], [0.2, 1.0, 0, 0]])
    before, after = case.run()
    assert_emulated(case, before, after)
    case.hyper.t[0, 0] = 0.0125                         # the device write of an LR halving (twice); no table is rebuilt
    case.h = case.h.copy()
    case.h[0, 0] = 0.0125
    case.set_grads(case.new_grads())
    before, after = case.run()
    assert_emulated(case, before, after)
    stale = case.h.copy()
    stale[0, 0] = 0.05
    old = orf.emulate_f32(after["coef"], before["p"], before["g"], None, case.group_of, stale)[0]
    for i, k in enumerate(case.group_of):                # group 0 moved by the new rate, not by the old one
        assert same_bits(old[i], after["p"][i]) == (k == 1)


def test_nonfinite_gradients_without_the_skip_flag(lib):
    """A NaN gradient: the group's norm, coef and parameters are NaN, the other group is finite.  An inf gradient: norm inf,
    coef 0, finite gradients become (signed) zeros, the inf one NaN.  The patterns are the emulation's."""
    case = Case(lib, seed=7)
    case.set_hyper([[0.05, 1.0, 0, 0], [0.2, 1.0, 0, 0]])
    g = [x.copy() for x in case.g]
    g[4][1234] = NAN                                     # group 0
    g[6][4096] = np.float32(np.inf)                      # group 1: the one element of its second chunk
    case.set_grads(g)
    before, after = case.run(finite=False)
    assert np.isnan(after["norm"][0]) and np.isnan(after["coef"][0]) and after["norm"][1] == np.inf and after["coef"][1] == 0.0
    assert same_bits(after["coef"][1:], orf.stats_f32(after["norm"], case.h[:, 1])[1:])
    assert_emulated(case, before, after, nan_ok=True)
    for i, k in enumerate(case.group_of):
        if k == 0:
            assert np.isnan(after["p"][i]).all() and np.isnan(after["g"][i]).all()
        else:
            assert np.isfinite(after["p"][i]).sum() == after["p"][i].size - (i == 6)
            assert np.isnan(after["g"][i]).sum() == (i == 6) and not np.nan_to_num(after["g"][i]).any()
    assert after["skipped"] == 0


def test_the_skip_flag_leaves_parameters_and_momentum_alone(lib):
    case = Case(lib, seed=8, momentum=True)
    case.set_hyper([[0.05, 1.0, 0.01, 0.9], [0.2, 1.0, 0, 0.9]])
    before, after = case.run(flags=SKIP_NONFINITE)       # a finite step first: the buffer is no longer zeros
    assert after["skipped"] == 0
    assert_emulated(case, before, after)
    g = case.new_grads()
    g[5][77] = np.float32(-np.inf)                       # group 1 alone is not finite; group 0 must stand still too
    case.set_grads(g)
    before, after = case.run(flags=SKIP_NONFINITE, finite=False)
    assert after["skipped"] == 1 and after["norm"][1] == np.inf and np.isfinite(after["norm"][0])
    assert_same(after["p"], before["p"], "parameter of a skipped step")
    assert_same(after["m"], before["m"], "momentum of a skipped step")
    assert_emulated(case, before, after, skip=True, nan_ok=True)         # the gradients are still the clipped ones
    case.set_grads(case.new_grads())
    before, after = case.run(flags=SKIP_NONFINITE)
    assert after["skipped"] == 1 and not any(same_bits(a, b) for a, b in zip(after["p"], before["p"]))
    assert_emulated(case, before, after)
    g = case.new_grads()
    g[0][0] = NAN
    case.set_grads(g)
    before, after = case.run(flags=SKIP_NONFINITE | ZERO_GRAD, finite=False)
    assert after["skipped"] == 2 and all(not x.view(np.uint32).any() for x in after["g"])
    assert_same(after["p"], before["p"], "parameter of a skipped step")
    assert_same(after["m"], before["m"], "momentum of a skipped step")


def test_zero_grad_stores_positive_zeros(lib):
    plain, zeroing = Case(lib, seed=9, momentum=True), Case(lib, seed=9, momentum=True)
    for case in (plain, zeroing):
        case.set_hyper([[0.05, 1.0, 0.01, 0.9], [0.2, 1.0, 0, 0.5]])
    _, a = plain.run()
    before, b = zeroing.run(flags=ZERO_GRAD)
    assert all(not x.view(np.uint32).any() for x in b["g"]) and any(x.any() for x in a["g"])
    assert_same(b["p"], a["p"], "parameter")
    assert_same(b["m"], a["m"], "momentum")
    assert same_bits(a["coef"], b["coef"]) and same_bits(a["norm"], b["norm"])
    assert_emulated(zeroing, before, b, zero=True)


def test_the_same_inputs_give_the_same_bits(lib):
    outs = []
    for _ in range(2):
        case = Case(lib, seed=10, momentum=True)
        case.set_hyper([[0.05, 0.5, 0.01, 0.9], [0.2, 0.5, 0, 0.5]])
        case.run(scale=0.25)
        case.set_grads(case.new_grads())
        outs.append(case.run(scale=0.25)[1])
    a, b = outs
    for k in ("p", "g", "m"):
        assert_same(a[k], b[k], k)
    for k in ("norm", "coef", "partial"):
        assert same_bits(a[k], b[k]), k


def functional_setup(GF, case, momentum):
    groups = [[case.pt[i] for i in range(case.n) if case.group_of[i] == g] for g in range(case.G)]
    offsets = [[case.off[i] for i in range(case.n) if case.group_of[i] == g] for g in range(case.G)]
    lay = GF.sgd_layout(groups, offsets)
    assert (lay.S, lay.C, lay.G) == (case.S, case.C, case.G) and lay.seg.tolist() == case.d_seg.get("seg").tolist()
    return lay, case.grad.t, case.hyper.t, (case.mom.t if momentum else None)


def fetch(case, lay):
    torch.cuda.synchronize()
    for b in case.pbufs + [case.grad, case.hyper] + ([case.mom] if case.mom is not None else []):
        assert b.guards_intact()
    return dict(p=[t.cpu().numpy() for t in case.pt], g=case._parts(case.grad.t.cpu().numpy(), "gradients"),
                m=case._parts(case.mom.t.cpu().numpy(), "momentum") if case.mom is not None else None,
                norm=lay.stats[:, 0].cpu().numpy(), coef=lay.stats[:, 1].cpu().numpy())


def test_a_captured_call_replays_as_three_eager_calls(GF, lib):
    """torch.cuda.graph around the one call (two kernel nodes in a line); before each replay new gradients go into the static
    bucket, and before the second the first group's learning rate is overwritten on the device."""
    hyper = [[0.05, 0.5, 0.01, 0.9], [0.2, 0.5, 0, 0.5]]
    eager, graphed = Case(lib, seed=11, momentum=True), Case(lib, seed=11, momentum=True)
    grads = [eager.g] + [eager.new_grads() for _ in range(2)]
    start_p = [x.copy() for x in eager.p]
    results = []
    for case, capture in ((eager, False), (graphed, True)):
        case.set_hyper(hyper)
        lay, grad, hyp, mom = functional_setup(GF, case, True)
        call = lambda: GF.sgd_clip_step(lay, grad, hyp, mom, grad_scale=0.25)  # noqa: E731
        graph = None
        if capture:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call()
        outs = []
        for step, g in enumerate(grads):
            case.set_grads(g)
            if step == 1:
                hyp[0, 0] = 0.025
            graph.replay() if capture else call()
            outs.append(fetch(case, lay))
        results.append(outs)
    for step, (a, b) in enumerate(zip(*results)):
        for k in ("p", "g", "m"):
            assert_same(a[k], b[k], f"step {step} {k}")
        assert same_bits(a["norm"], b["norm"]) and same_bits(a["coef"], b["coef"])
    # and the eager route is the emulation's, with the rate of each step
    state = dict(p=start_p, m=[np.zeros_like(x) for x in start_p])
    for step, out in enumerate(results[0]):
        eager.h[0, 0] = 0.05 if step == 0 else 0.025
        assert_emulated(eager, dict(p=state["p"], g=grads[step], m=state["m"]), out, scale=0.25)
        state = out


def test_a_moved_parameter_rebuilds_the_table(GF, lib):
    case = Case(lib, seed=12)
    case.set_hyper([[0.05, 0.5, 0, 0], [0.2, 0.5, 0, 0]])
    holders = [torch.nn.Parameter(t, requires_grad=False) for t in case.pt]
    assert all(h.data_ptr() == t.data_ptr() for h, t in zip(holders, case.pt))
    groups = [[holders[i] for i in range(case.n) if case.group_of[i] == g] for g in range(case.G)]
    offsets = [[case.off[i] for i in range(case.n) if case.group_of[i] == g] for g in range(case.G)]
    lay = GF.sgd_layout(groups, offsets)
    stats = GF.sgd_clip_step(lay, case.grad.t, case.hyper.t)
    first = fetch(case, lay)
    assert stats is lay.stats
    assert_emulated(case, dict(p=case.p, g=case.g, m=None), first)
    # tensor 4 (4095 elements) moves to a new guarded buffer, one word further into its line than the old one
    new_values = case.new_grads()[4]
    moved = Buf((case.sizes[4],), new_values, offset=(case.off[4] + 1) % 4)
    holders[4].data = moved.t
    case.set_grads(case.new_grads())
    GF.sgd_clip_step(lay, case.grad.t, case.hyper.t)
    second = fetch(case, lay)
    assert lay.seg[case.order.index(4), 0].item() == moved.ptr
    start = [x if i != 4 else new_values for i, x in enumerate(first["p"])]
    want = orf.emulate_f32(second["coef"], start, case.g, None, case.group_of, case.h)[0]
    assert same_bits(moved.get("the moved parameter"), want[4])
    assert same_bits(second["p"][4], first["p"][4]), "the old storage was written after the parameter had moved"
    assert_same([x for i, x in enumerate(second["p"]) if i != 4], [x for i, x in enumerate(want) if i != 4], "parameter")


@pytest.mark.parametrize("name", tfx.FIXTURES)
def test_trainer_with_the_native_step_on_gpu(name):
    """Both golden trajectories with DPTrainer(native_step=True) and the HIP loss, at the tolerances the torch route's test
    applies to the same fixtures (losses rtol 1e-4; final weights rtol 2e-3, atol 2e-6; w, b within 5e-5)."""
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    from speaker_embedding_ge2e_loss_amd.optim import ClipSGD
    from speaker_embedding_ge2e_loss_amd.trainer import DPTrainer
    dev = torch.device("cuda:0")
    z, c = tfx.load(name)
    tr = DPTrainer(tfx.encoder_from(z, c, dev), GE2ELoss(HParams(device=dev)), lr=c["lr"], seed=c["seed"], native_step=True)
    assert type(tr.optimizer) is ClipSGD and [g["max_norm"] for g in tr.optimizer.param_groups] == [3.0, 1.0]
    base = tr.flat_grad.untyped_storage().data_ptr()
    seen = []

    def after_step(t):
        assert all(p.grad is not None and p.grad.untyped_storage().data_ptr() == base for p in t._params)
        at, norms = 0, []
        for g in t.optimizer.param_groups:
            n = sum(p.numel() for p in g["params"])
            norms.append(float(t.flat_grad[at:at + n].double().norm()))
            at += n
        st = t.optimizer.stats.cpu().numpy().astype(np.float64)
        seen.append(st[:, 1].copy())
        # .grad holds the clipped gradients: norm times coef, never above the threshold
        assert np.allclose(norms, st[:, 0] * st[:, 1], rtol=1e-5, atol=1e-12) and norms[0] <= 3.0 * (1 + 1e-5) and norms[1] <= 1.0 + 1e-5

    losses, test = tfx.run_trajectory(z, c, tr, dev, after_step)
    tfx.check(z, c, tr, losses, test, rtol=1e-4)
    assert [g["lr"] for g in tr.optimizer.param_groups] == list(z["final_lrs"]) and len(seen) == c["steps"]
    assert tr.optimizer._hyper[:, 0].cpu().tolist() == [float(np.float32(v)) for v in z["final_lrs"]]


def test_clip_sgd_against_torch_on_the_same_gpu():
    """One step of ClipSGD (momentum 0.9, weight decay 0.01, two groups, one of them clipped) from copies of the same
    parameters and gradients as clip_grad_norm_ + torch.optim.SGD: both within the derived bound of the float64 oracle, so
    within twice the bound of each other.  p and g share a sign per element (float64_bound)."""
    from speaker_embedding_ge2e_loss_amd.optim import ClipSGD
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(13)
    sizes, group_of, lrs, mx = (7, 4097, 300, 1, 5000), (0, 0, 1, 1, 0), (0.05, 0.2), (1.5, 1e3)
    sign = [np.where(rng.random(n) < 0.5, -1.0, 1.0) for n in sizes]
    p0 = [((np.abs(rng.standard_normal(n)) + 0.5) * s).astype(np.float32) for n, s in zip(sizes, sign)]
    g0 = [(np.abs(rng.standard_normal(n)) * 0.3 * s).astype(np.float32) for n, s in zip(sizes, sign)]

    def fresh():
        ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(dev)) for x in p0]
        return ps, [{"params": [p for p, k in zip(ps, group_of) if k == g], "lr": lrs[g]} for g in (0, 1)]

    mine, groups = fresh()
    opt = ClipSGD(groups, lr=1.0, max_norm=mx, momentum=0.9, weight_decay=0.01)
    assert all(p.grad is not None and p.grad.untyped_storage().data_ptr() == opt.flat_grad.untyped_storage().data_ptr() for p in mine)
    for p, g in zip(mine, g0):
        p.grad.copy_(torch.from_numpy(g))
    opt.step()
    theirs, groups = fresh()
    ref_opt = torch.optim.SGD(groups, lr=1.0, momentum=0.9, weight_decay=0.01)
    for p, g in zip(theirs, g0):
        p.grad = torch.from_numpy(g.copy()).to(dev)
    for k, g in enumerate(groups):
        torch.nn.utils.clip_grad_norm_(g["params"], mx[k])
    ref_opt.step()
    hyper = np.asarray([[lrs[g], mx[g], 0.01, 0.9] for g in (0, 1)], np.float32)
    ref = orf.step(p0, g0, [np.zeros(n) for n in sizes], group_of, hyper.astype(np.float64))
    assert ref["coef"][0] < 1 and ref["coef"][1] == 1
    st = opt.stats.cpu().numpy()
    assert np.allclose(st[:, 0], ref["norm"], rtol=1e-5, atol=0) and np.allclose(st[:, 1], ref["coef"], rtol=1e-5, atol=0)
    for a, b, want, bound in zip(mine, theirs, ref["params"], float64_bound(p0, ref)):
        a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
        assert (np.abs(a - want) <= bound).all() and (np.abs(a - b) <= 2 * bound).all()
    for p, q in zip(mine, theirs):                       # and the clipped gradients both leave behind
        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=0)
    # the learning rate stays a host value that step() carries to the device when it changed
    opt.param_groups[0]["lr"] = 0.0125
    opt.zero_grad()
    assert all(p.grad is not None for p in mine) and not bool(opt.flat_grad.any())
    before = [p.detach().clone() for p in mine]
    opt.step()
    assert opt._hyper[0, 0].item() == float(np.float32(0.0125)) and opt._uploaded[0][0] == 0.0125
    # zero gradients: the parameters move by momentum and weight decay alone, the first group at its new rate
    m1 = [np.asarray(m, np.float64) for m in ref["moms"]]
    for p, b4, m, k in zip(mine, before, m1, group_of):
        lr = (0.0125, 0.2)[k]
        want = b4.cpu().numpy().astype(np.float64) - lr * (0.9 * m + 0.01 * b4.cpu().numpy().astype(np.float64))
        assert np.allclose(p.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-7)
