"""What the differentiable labelled helpers cost beside the fused wide loss and beside torch ops, forward + backward, on one
GPU.  One process, seeded inputs, the points taken in turn round after round, each call between its own pair of events on
an idle queue, median / min / max of those (the method of tools/bench_labeled.py).  Two shapes, both B = 1, D = 256, rows
shuffled:
  default      64 speakers, a seeded draw of counts in 2..18 summing to R = 640 rows; 200 rounds after 10 warm-ups
  --test-set   1 024 speakers, counts in 2..30 summing to R = 16 384 rows; 20 rounds after 3 warm-ups
Points:
  helpers    functional.cos_sim_labeled(differentiable=True), w * cos + b in torch, functional.calc_loss_labeled, backward():
             three launches forward, two torch ops, two launches; one launch, torch's backward of the head, six launches
  wide       functional.ge2e_loss_labeled(wide=True) + backward: seven launches and ge2e_scale_grads
  torch_ops  tools/bench_labeled.py's torch_ops_loss (argsort, index_select, the loss in torch ops, fp32) + autograd
Before anything is timed, helpers and wide must agree within the ragged gate (tests/test_gpu_ragged.check) at factor 2: loss,
dE (relative Frobenius norm and max-abs), dw, db.  No bound on the times.  One JSON line per point on stdout.
`--only POINT`: nothing but 20 calls of that point at the chosen shape, for a kernel trace.

usage: python tools/bench_labeled_grad.py [--test-set] [--only helpers|wide|torch_ops]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_labeled import loss_bound, torch_ops_loss  # noqa: E402
from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

D = 256
GT, WT = 1e-5, 2e-5     # tests/test_gpu_ragged.py


def drawn_labels(rng, n, R, top):
    """n counts in 2..top that sum to R (a uniform draw, then single steps at random speakers), as shuffled row labels."""
    c = rng.integers(2, top + 1, size=n)
    while c.sum() != R:
        j = rng.integers(n)
        step = 1 if c.sum() < R else -1
        if 2 <= c[j] + step <= top:
            c[j] += step
    return rng.permutation(np.repeat(np.arange(n), c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--test-set", action="store_true", help="1 024 speakers, 16 384 rows")
    ap.add_argument("--only", choices=("helpers", "wide", "torch_ops"), help="20 calls of one point, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_labeled_grad.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    n, R, top, rounds, warm, seed = (1024, 16384, 30, 20, 3, 4321) if args.test_set else (64, 640, 18, 200, 10, 1234)
    rng = np.random.default_rng(seed)
    lab_np = drawn_labels(rng, n, R, top)
    g = torch.Generator(device=dev).manual_seed(seed)
    e = torch.nn.functional.normalize(torch.randn(R, D, generator=g, device=dev), dim=-1).requires_grad_(True)
    lab = torch.as_tensor(lab_np, device=dev, dtype=torch.int64)
    lab32 = lab.to(torch.int32)
    w = torch.tensor(10.0, device=dev, requires_grad=True)
    b = torch.tensor(-5.0, device=dev, requires_grad=True)
    last, grad = {}, {}

    def step(name, loss):
        e.grad = w.grad = b.grad = None
        loss.backward()
        last[name], grad[name] = loss.detach(), (e.grad, w.grad, b.grad)

    def helpers():
        o = GF.cos_sim_labeled(e, lab32, num_speakers=n, differentiable=True)
        step("helpers", GF.calc_loss_labeled(w * o.cos + b, o.col, o.active)[0])

    def wide():
        step("wide", GF.ge2e_loss_labeled(e, lab32, w, b, num_speakers=n, wide=True))

    def torch_ops():
        step("torch_ops", torch_ops_loss(e, lab, n, w, b))

    points = [("helpers", helpers), ("wide", wide), ("torch_ops", torch_ops)]
    if args.only:
        for _ in range(20):
            dict(points)[args.only]()
        torch.cuda.synchronize()
        return
    for _ in range(warm):
        for _, fn in points:
            fn()
    torch.cuda.synchronize()
    lw = last["wide"].item()
    (ge, gw, gb), (he, hw, hb) = grad["wide"], grad["helpers"]
    fig = {"helpers_loss": last["helpers"].item(), "wide_loss": lw, "torch_ops_loss": last["torch_ops"].item(),
           "loss_bound": 2 * loss_bound(lw, R),
           "dE_rel_fro": ((he - ge).norm() / ge.norm()).item(), "dE_max_abs": (he - ge).abs().max().item(),
           "dE_max_abs_bound": 2 * 4 * GT * max(1.0, ge.abs().max().item()),
           "dw": abs(hw.item() - gw.item()), "dw_bound": 2 * (WT * abs(gw.item()) + 1e-5 + 1e-7 * R),
           "db": abs(hb.item() - gb.item()), "db_bound": 2 * (1e-4 + 3e-7 * R)}
    print(json.dumps(fig), flush=True)
    assert abs(fig["helpers_loss"] - lw) <= fig["loss_bound"], "the helpers' loss and the wide loss differ"
    assert fig["dE_rel_fro"] <= 2 * GT and fig["dE_max_abs"] <= fig["dE_max_abs_bound"], "the helpers' dE and the wide loss's differ"
    assert fig["dw"] <= fig["dw_bound"] and fig["db"] <= fig["db_bound"], "the helpers' dw / db and the wide loss's differ"
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for name, _ in points}
    for i in range(rounds):
        for name, fn in points:
            e0, e1 = ev[name][i]
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()          # every call starts on an idle queue: its own time, not its place in a backlog
    med = {}
    for name, _ in points:
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]) * 1e3
        med[name] = float(np.median(t))
        print(json.dumps({"point": name, "N": n, "R": R, "D": D, "rounds": rounds, "call_us_median": round(med[name], 2),
                          "call_us_min": round(float(t.min()), 2), "call_us_max": round(float(t.max()), 2),
                          "loss": float(last[name])}), flush=True)
    print(json.dumps({"helpers_over_wide": round(med["helpers"] / med["wide"], 3),
                      "helpers_over_torch_ops": round(med["helpers"] / med["torch_ops"], 3)}), flush=True)


if __name__ == "__main__":
    main()
