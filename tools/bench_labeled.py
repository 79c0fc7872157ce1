"""What the labelled ragged loss costs at one training batch, against the routes a caller had before, on one GPU:
B = 1, N = 64 speakers, a seeded draw of counts in 2..18 summing to R = 640 rows, D = 256, rows shuffled.
  (a) labeled        functional.ge2e_loss_labeled(e, device labels, num_speakers=64) + backward: index kernel, gathering
                     loss kernel, ge2e_scale_grads
  (b) torch_route    argsort(stable) + index_select + bincount / cumsum (device offsets, no sync) + ge2e_loss_ragged +
                     backward (autograd scatters the gradient through index_select)
  (c) ragged_sorted  ge2e_loss_ragged + backward on rows that are sorted already, offsets on the device
and the masked labelled loss (masked=True: masked index kernel, the loss kernel with its extents from the device) on the
same rows:
  (f) masked_all_active  the same labels with the exact num_speakers = 64: every row counts, the loss bits of (a)
  (g) masked_sparse      num_speakers = 1251 as a bound, the 64 speakers' ids spread over 0..1250 (seeded), and a seeded
                         10 % of the rows labelled -1
and the bare enqueues on preallocated outputs, no autograd:
  (d) labeled_call   functional.loss_fwd_bwd_labeled   (two launches)
  (e) ragged_call    functional.loss_fwd_bwd_ragged on the sorted rows   (one launch)
and the masked loss's wide route (wide=True: the same semantics on many workgroups per batch, seven launches) on (f)'s call:
  (h) wide               required: at most 0.5 x (f), median against median (asserted)
All in one process, the points taken in turn round after round (so that clocks and neighbours hit them alike).  Per point:
`--rounds` (>= 50) calls each between its own pair of events, median / min / max of those; then a window of `--window`
calls back to back ending in a synchronise, host clock, as the per-call time at full queue.  (d) and (e) must return the
same loss bits, as must (a) and (f); (a), (b), (c) the same loss to 1e-5, (h) and (f) to the ragged gate's loss bound.
One JSON line per point on stdout.

`--test-set`: the evaluation bench's test set instead -- B = 1, 1 024 speakers, a seeded draw of counts in 2..30 summing to
R = 16 384 rows, D = 256, shuffled -- with two points taken in turn, 20 rounds after 3 warm-ups:
  wide         functional.ge2e_loss_labeled(wide=True) + backward
  torch_ops    argsort(stable) + index_select + the loss written in torch ops in fp32 + autograd's backward (which scatters
               the gradient through index_select)
The two losses must agree to the ragged gate's loss bound (asserted); no bound on the times.  The masked entry -- one
workgroup for the whole batch -- is timed there ONCE, in a single call after the rounds, for the record only.
`--wide-only`: nothing but 20 calls of the wide point of the chosen shape, for a kernel trace.

usage: python tools/bench_labeled.py [--rounds 200] [--window 500] [--test-set] [--wide-only]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

N, D, R = 64, 256, 640
N_BOUND = 1251          # masked_sparse: the speaker count of a data set, as a bound


def drawn_counts(rng):
    """N counts in 2..18 that sum to R: a uniform draw, then single steps at random speakers until the sum fits."""
    c = rng.integers(2, 19, size=N)
    while c.sum() != R:
        j = rng.integers(N)
        step = 1 if c.sum() < R else -1
        if 2 <= c[j] + step <= 18:
            c[j] += step
    return c


def loss_bound(loss, R):
    """The loss bound of the ragged gate (tests/test_gpu_ragged.check) for a softmax loss, whose rows are all >= 0."""
    return 5e-6 * abs(loss) + 3e-7 * abs(loss) + 1e-6 + 2e-7 * R


def torch_ops_loss(e, lab, n, w, b, eps=GF.SMALL_ERR, eps_cos=GF.EPS_COS):
    """The labelled softmax loss of rows in any order in torch ops, fp32: every speaker has >= 2 rows."""
    o = torch.argsort(lab, stable=True)
    es, ls = e.index_select(0, o), lab[o]
    m = torch.bincount(lab, minlength=n).to(e.dtype)
    sums = torch.zeros(n, e.shape[1], device=e.device, dtype=e.dtype).index_add_(0, ls, es)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(eps_cos)  # noqa: E731
    u = (sums[ls] - es) / (m[ls] - 1)[:, None]
    cos = unit(es) @ unit(sums / m[:, None]).T
    own = (unit(es) * unit(u)).sum(-1)
    sim = w * (cos.scatter(1, ls[:, None], own[:, None]) + eps) + b
    per = torch.log(torch.exp(sim).sum(1) + eps) - sim.gather(1, ls[:, None])[:, 0]
    return per.sum()


def run_test_set(args, dev):
    """--test-set: see the module docstring."""
    n, R, rounds, warm = 1024, 16384, 20, 3
    rng = np.random.default_rng(4321)
    c = rng.integers(2, 31, size=n)
    while c.sum() != R:
        j = rng.integers(n)
        step = 1 if c.sum() < R else -1
        if 2 <= c[j] + step <= 30:
            c[j] += step
    lab_np = rng.permutation(np.repeat(np.arange(n), c))
    g = torch.Generator(device=dev).manual_seed(4321)
    e = torch.nn.functional.normalize(torch.randn(R, D, generator=g, device=dev), dim=-1).requires_grad_(True)
    lab = torch.as_tensor(lab_np, device=dev, dtype=torch.int64)
    lab32 = lab.to(torch.int32)
    w = torch.tensor(10.0, device=dev, requires_grad=True)
    b = torch.tensor(-5.0, device=dev, requires_grad=True)
    last, grad = {}, {}

    def step(name, loss):
        e.grad = w.grad = b.grad = None
        loss.backward()
        last[name], grad[name] = loss.detach(), e.grad

    def wide():
        step("wide", GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=n, wide=True))

    def torch_ops():
        step("torch_ops", torch_ops_loss(e, lab, n, w, b))

    if args.wide_only:
        for _ in range(20):
            wide()
        torch.cuda.synchronize()
        return
    points = [("wide", wide), ("torch_ops", torch_ops)]
    for _ in range(warm):
        for _, fn in points:
            fn()
    torch.cuda.synchronize()
    diff, bound = abs(last["wide"].item() - last["torch_ops"].item()), loss_bound(last["torch_ops"].item(), R)
    gdiff = ((grad["wide"] - grad["torch_ops"]).norm() / grad["torch_ops"].norm()).item()
    print(json.dumps({"wide_loss": last["wide"].item(), "torch_ops_loss": last["torch_ops"].item(), "difference": diff,
                      "bound": bound, "dE_rel_fro": gdiff}), flush=True)
    assert diff <= bound, f"wide and the torch-op route differ by {diff}, bound {bound}"
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for name, _ in points}
    for i in range(rounds):
        for name, fn in points:
            e0, e1 = ev[name][i]
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
    med = {}
    for name, _ in points:
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]) * 1e3
        med[name] = float(np.median(t))
        print(json.dumps({"point": name, "N": n, "R": R, "D": D, "rounds": rounds, "call_us_median": round(med[name], 2),
                          "call_us_min": round(float(t.min()), 2), "call_us_max": round(float(t.max()), 2),
                          "loss": float(last[name])}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step("masked", GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=n, masked=True))
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"point": "masked_single_workgroup", "calls": 1, "call_us": round(e0.elapsed_time(e1) * 1e3, 2),
                      "loss": float(last["masked"])}), flush=True)
    print(json.dumps({"wide_over_torch_ops": round(med["wide"] / med["torch_ops"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--test-set", action="store_true", help="the evaluation bench's test set: wide beside torch ops")
    ap.add_argument("--wide-only", action="store_true", help="20 calls of the wide point alone, for a kernel trace")
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_labeled.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    if args.test_set:
        return run_test_set(args, dev)
    rng = np.random.default_rng(1234)
    counts = drawn_counts(rng)
    lab_np = rng.permutation(np.repeat(np.arange(N), counts))
    g = torch.Generator(device=dev).manual_seed(1234)
    e = torch.nn.functional.normalize(torch.randn(R, D, generator=g, device=dev), dim=-1).requires_grad_(True)
    lab = torch.as_tensor(lab_np, device=dev, dtype=torch.int64)
    lab32 = lab.to(torch.int32)
    spread = np.sort(rng.choice(N_BOUND, size=N, replace=False))
    sparse_np = spread[lab_np]
    sparse_np[rng.choice(R, size=R // 10, replace=False)] = -1
    sparse32 = torch.as_tensor(sparse_np, device=dev, dtype=torch.int32)
    w = torch.tensor(10.0, device=dev, requires_grad=True)
    b = torch.tensor(-5.0, device=dev, requires_grad=True)
    order = torch.argsort(lab, stable=True)
    es = e.detach()[order].contiguous().requires_grad_(True)
    off = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), device=dev, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    z = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = GF.LossOutputs(loss=z(1), per=None, dE=z(1, R, D), dw=z(1), db=z(1))
    wd, bd = w.detach(), b.detach()
    last = {}

    def step(name, leaf, loss):
        leaf.grad = w.grad = b.grad = None
        loss.backward()
        last[name] = loss.detach()

    def labeled():
        step("labeled", e, GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=N))

    def torch_route():
        o = torch.argsort(lab, stable=True)
        offsets = torch.cat([zero, torch.cumsum(torch.bincount(lab, minlength=N), 0)]).to(torch.int32)
        step("torch_route", e, GF.ge2e_loss_ragged(e.index_select(0, o), offsets, w, b))

    def ragged_sorted():
        step("ragged_sorted", es, GF.ge2e_loss_ragged(es, off, w, b))

    def masked_all_active():
        step("masked_all_active", e, GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=N, masked=True))

    def masked_sparse():
        step("masked_sparse", e, GF.ge2e_loss_labeled(e, sparse32, w, b, num_speakers=N_BOUND, masked=True))

    def wide():
        step("wide", e, GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=N, wide=True))

    def labeled_call():
        last["labeled_call"] = GF.loss_fwd_bwd_labeled(e.detach(), lab32, wd, bd, num_speakers=N, out=out).loss.clone()

    def ragged_call():
        last["ragged_call"] = GF.loss_fwd_bwd_ragged(es.detach(), off, wd, bd, out=out).loss.clone()

    points = [("labeled", labeled), ("torch_route", torch_route), ("ragged_sorted", ragged_sorted),
              ("labeled_call", labeled_call), ("ragged_call", ragged_call), ("masked_all_active", masked_all_active),
              ("masked_sparse", masked_sparse), ("wide", wide)]
    if args.wide_only:
        for _ in range(20):
            wide()
        torch.cuda.synchronize()
        return
    for _ in range(10):
        for _, fn in points:
            fn()
    torch.cuda.synchronize()
    assert torch.equal(last["labeled_call"], last["ragged_call"]), "the labelled call and the ragged call on sorted rows differ"
    assert torch.equal(last["masked_all_active"], last["labeled"]), "masked with every row active and the labelled loss differ"
    assert abs(last["wide"].item() - last["masked_all_active"].item()) <= 2 * loss_bound(last["masked_all_active"].item(), R), last
    for k in ("torch_route", "ragged_sorted"):
        assert abs(last[k].item() - last["labeled"].item()) <= 1e-5 * abs(last["labeled"].item()), (k, last)
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.rounds)]
          for name, _ in points}
    for i in range(args.rounds):
        for name, fn in points:
            e0, e1 = ev[name][i]
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()          # every call starts on an idle queue: its own time, not its place in a backlog
    windows = {}
    for name, fn in points:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.window):
            fn()
        torch.cuda.synchronize()
        windows[name] = (time.perf_counter() - t0) / args.window
    med = {}
    for name, _ in points:
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]) * 1e3
        med[name] = float(np.median(t))
        print(json.dumps({"point": name, "N": N, "R": R, "D": D, "rounds": args.rounds, "call_us_median": round(med[name], 2),
                          "call_us_min": round(float(t.min()), 2), "call_us_max": round(float(t.max()), 2),
                          "window_calls": args.window, "window_us_per_call": round(windows[name] * 1e6, 2),
                          "loss": float(last[name].reshape(-1)[0])}), flush=True)
    print(json.dumps({"labeled_over_torch_route": round(med["labeled"] / med["torch_route"], 3),
                      "labeled_over_ragged_sorted": round(med["labeled"] / med["ragged_sorted"], 3),
                      "labeled_call_over_ragged_call": round(med["labeled_call"] / med["ragged_call"], 3),
                      "masked_all_active_over_labeled": round(med["masked_all_active"] / med["labeled"], 3),
                      "masked_sparse_over_labeled": round(med["masked_sparse"] / med["labeled"], 3),
                      "wide_over_masked_all_active": round(med["wide"] / med["masked_all_active"], 3)}), flush=True)
    assert med["wide"] <= 0.5 * med["masked_all_active"], \
        f"the wide route takes {med['wide']:.1f} us, more than half of the masked entry's {med['masked_all_active']:.1f} us"


if __name__ == "__main__":
    main()
