"""What labelled evaluation (ge2e_cos_sim_labeled) costs on one GPU, against the routes a caller had before.  Two shapes:
  a  the labelled bench's batch (tools/bench_labeled.py): 64 speakers, a seeded draw of counts in 2..18 summing to
     R = 640 rows, D = 256, rows shuffled, random unit rows
  b  a test set: 1 024 speakers, R = 16 384 rows (seeded counts >= 2), D = 256, rows shuffled, unit rows centre + 0.5 noise
Points, all bare enqueues on the current stream, thresholds = evaluation.THRESHOLDS resident on the device:
  fused_counts      functional.cos_sim_labeled(need_cos=False, thresholds): the similarity matrix is never materialised
  cos               functional.cos_sim_labeled(): cos (R, N) materialised, no counts
  cos_then_counts   the same, then functional.eer_counts_labeled on that cos
  torch_route       torch ops on the same GPU: stable argsort (the rows' order), bincount, index_add_, normalise, matmul,
                    the leave-one-out fix-up of the own column, compare-and-sum against the 50 thresholds
  loss_fwd_masked   shape a only: functional.loss_fwd_bwd_labeled(masked=True, need_grad=False), the forward-only call of
                    the single-workgroup loss kernel -- the only code before this tool's subject that computes these cosines
The counts of fused_counts, cos_then_counts and torch_route must be equal (asserted).  All in one process, the points taken
in turn round after round; per point `--rounds` (>= 50) calls each between its own pair of events after 10 warm-up rounds,
median / min / max.  One JSON line per point and one of ratios per shape on stdout.  profiles/labeled_eval_bench.txt holds
two runs of the whole command.

usage: python tools/bench_labeled_eval.py [--rounds 200]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402
from speaker_embedding_ge2e_loss_amd.evaluation import THRESHOLDS  # noqa: E402

D = 256
EPS, EPS_COS = GF.SMALL_ERR, GF.EPS_COS


def drawn_counts(rng, n, rows, top):
    """n counts in 2..top that sum to rows: a uniform draw, then single steps at random speakers until the sum fits."""
    c = rng.integers(2, top + 1, size=n)
    while c.sum() != rows:
        j = rng.integers(n)
        step = 1 if c.sum() < rows else -1
        if 2 <= c[j] + step <= top:
            c[j] += step
    return c


def shape_a(dev):
    n, rows = 64, 640
    rng = np.random.default_rng(1234)
    lab = rng.permutation(np.repeat(np.arange(n), drawn_counts(rng, n, rows, 18)))
    g = torch.Generator(device=dev).manual_seed(1234)
    e = torch.nn.functional.normalize(torch.randn(rows, D, generator=g, device=dev), dim=-1)
    return "a", n, rows, e, torch.as_tensor(lab, device=dev, dtype=torch.int64)


def shape_b(dev):
    n, rows = 1024, 16384
    rng = np.random.default_rng(4321)
    lab = rng.permutation(np.repeat(np.arange(n), drawn_counts(rng, n, rows, 30)))
    g = torch.Generator(device=dev).manual_seed(4321)
    centre = torch.randn(n, D, generator=g, device=dev)
    lab_t = torch.as_tensor(lab, device=dev, dtype=torch.int64)
    e = torch.nn.functional.normalize(centre[lab_t] + 0.5 * torch.randn(rows, D, generator=g, device=dev), dim=-1)
    return "b", n, rows, e.contiguous(), lab_t


def torch_route(e, lab, n, thr):
    rows = e.shape[0]
    order = torch.argsort(lab, stable=True)                                  # the rows' sorted order (what `col` stands for)
    cnt = torch.bincount(lab, minlength=n).to(e.dtype)
    sums = torch.zeros(n, e.shape[1], device=e.device).index_add_(0, lab, e)
    cent = torch.nn.functional.normalize(sums / cnt[:, None], dim=-1, eps=EPS_COS)
    cos = torch.nn.functional.normalize(e, dim=-1, eps=EPS_COS) @ cent.t()
    loo = (sums[lab] - e) / (cnt[lab] - 1)[:, None]
    own = torch.nn.functional.cosine_similarity(e, loo, dim=-1, eps=EPS_COS)
    cos[torch.arange(rows, device=e.device), lab] = own
    cos += EPS
    total = (cos.unsqueeze(-1) > thr).sum(dim=(0, 1))
    ta = ((own + EPS).unsqueeze(-1) > thr).sum(dim=0)
    return torch.stack([total - ta, ta], dim=-1).to(torch.int32), order


def bench_shape(make, dev, rounds):
    tag, n, rows, e, lab = make(dev)
    lab32 = lab.to(torch.int32)
    thr = torch.as_tensor(THRESHOLDS, dtype=torch.float64).to(torch.float32).to(dev)
    last = {}

    def fused_counts():
        last["fused_counts"] = GF.cos_sim_labeled(e, lab32, num_speakers=n, thresholds=thr, need_cos=False).counts

    def cos():
        last["cos"] = GF.cos_sim_labeled(e, lab32, num_speakers=n).cos

    def cos_then_counts():
        o = GF.cos_sim_labeled(e, lab32, num_speakers=n)
        last["cos_then_counts"] = GF.eer_counts_labeled(o.cos, o.col, o.active, thr)

    def route():
        last["torch_route"] = torch_route(e, lab, n, thr)[0]

    points = [("fused_counts", fused_counts), ("cos", cos), ("cos_then_counts", cos_then_counts), ("torch_route", route)]
    if tag == "a":
        w, b = torch.tensor(10.0, device=dev), torch.tensor(-5.0, device=dev)
        out = GF.LossOutputs(loss=torch.empty(1, device=dev), per=None, dE=None, dw=None, db=None,
                             active=torch.empty(1, 2, dtype=torch.int32, device=dev))

        def loss_fwd_masked():
            last["loss_fwd_masked"] = GF.loss_fwd_bwd_labeled(e, lab32, w, b, num_speakers=n, need_grad=False, masked=True,
                                                              out=out).loss

        points.append(("loss_fwd_masked", loss_fwd_masked))
    for _ in range(10):
        for _, fn in points:
            fn()
    torch.cuda.synchronize()
    assert torch.equal(last["fused_counts"], last["cos_then_counts"]), "fused counts and ge2e_eer_counts_labeled differ"
    assert torch.equal(last["fused_counts"], last["torch_route"]), "fused counts and the torch route's differ"
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for name, _ in points}
    for i in range(rounds):
        for name, fn in points:
            torch.cuda.synchronize()      # every call starts on an idle queue: its own time, not its place in a backlog
            e0, e1 = ev[name][i]
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    med = {}
    for name, _ in points:
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]) * 1e3
        med[name] = float(np.median(t))
        print(json.dumps({"shape": tag, "point": name, "N": n, "R": rows, "D": D, "T": len(THRESHOLDS), "rounds": rounds,
                          "call_us_median": round(med[name], 2), "call_us_min": round(float(t.min()), 2),
                          "call_us_max": round(float(t.max()), 2),
                          "accepts_at_first_threshold": last["fused_counts"].reshape(-1, 2)[0].tolist()}), flush=True)
    ratios = {"shape": tag, "fused_counts_over_torch_route": round(med["fused_counts"] / med["torch_route"], 4),
              "cos_over_torch_route": round(med["cos"] / med["torch_route"], 4),
              "cos_then_counts_over_fused_counts": round(med["cos_then_counts"] / med["fused_counts"], 3)}
    if tag == "a":
        ratios["fused_counts_over_loss_fwd_masked"] = round(med["fused_counts"] / med["loss_fwd_masked"], 4)
        ratios["cos_over_loss_fwd_masked"] = round(med["cos"] / med["loss_fwd_masked"], 4)
    print(json.dumps(ratios), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_labeled_eval.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    for make in (shape_a, shape_b):
        bench_shape(make, dev, args.rounds)


if __name__ == "__main__":
    main()
