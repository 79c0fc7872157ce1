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
All in one process, the points taken in turn round after round (so that clocks and neighbours hit them alike).  Per point:
`--rounds` (>= 50) calls each between its own pair of events, median / min / max of those; then a window of `--window`
calls back to back ending in a synchronise, host clock, as the per-call time at full queue.  (d) and (e) must return the
same loss bits, as must (a) and (f); (a), (b), (c) the same loss to 1e-5.  One JSON line per point on stdout.

usage: python tools/bench_labeled.py [--rounds 200] [--window 500]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--window", type=int, default=500)
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_labeled.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
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

    def labeled_call():
        last["labeled_call"] = GF.loss_fwd_bwd_labeled(e.detach(), lab32, wd, bd, num_speakers=N, out=out).loss.clone()

    def ragged_call():
        last["ragged_call"] = GF.loss_fwd_bwd_ragged(es.detach(), off, wd, bd, out=out).loss.clone()

    points = [("labeled", labeled), ("torch_route", torch_route), ("ragged_sorted", ragged_sorted),
              ("labeled_call", labeled_call), ("ragged_call", ragged_call), ("masked_all_active", masked_all_active),
              ("masked_sparse", masked_sparse)]
    for _ in range(10):
        for _, fn in points:
            fn()
    torch.cuda.synchronize()
    assert torch.equal(last["labeled_call"], last["ragged_call"]), "the labelled call and the ragged call on sorted rows differ"
    assert torch.equal(last["masked_all_active"], last["labeled"]), "masked with every row active and the labelled loss differ"
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
                      "masked_sparse_over_labeled": round(med["masked_sparse"] / med["labeled"], 3)}), flush=True)


if __name__ == "__main__":
    main()
