"""What verification against a speaker bank (ge2e_verify_scores) costs on one GPU, against what a caller wrote before.
Shape: K = 1 251 enrolled speakers, D = 256, R = 16 384 labelled trial rows (unit rows centre + 0.5 noise, one row in 50 of
an unknown speaker), the 50 reference thresholds resident on the device.  Points, all bare enqueues on the current stream:
  counts_only         functional.verify_scores(need_scores=False, thresholds): the R x K matrix is never materialised
  scores_and_counts   functional.verify_scores(thresholds): scores (R, K) written as well
  scores_alone        functional.verify_scores() without labels: the matrix alone
  torch_scores        F.normalize(e) @ models.T + eps alone
  torch_route         F.normalize(e) @ models.T + eps, then the 50-threshold count as one broadcast compare-and-sum
  torch_route_loop    the same product, the count as a loop over the thresholds (no R x K x T temporary)
  *_staged / *_streamed   counts_only and scores_alone through ge2e_selftest_verify_form: the model tiles staged in LDS once
                      per workgroup, or streamed from L2 by every wave (the product call streams)
The counts of the library's points must be equal (asserted); the torch routes round their products differently, so the
number of counts that differ from the library's is reported, not asserted.  All in one process, the points taken in turn
round after round, each call between its own pair of HIP events on an idle queue after 10 warm-up rounds; median / min / max
per point.  Every point's warm-up and every timed round runs under a watchdog (--step-timeout seconds) that ends the
process.  One JSON line per point and one of ratios on stdout.  profiles/enroll_verify_bench.txt holds a run.

usage: python tools/bench_enroll_verify.py [--rounds 100] [--step-timeout 60]
"""
import argparse
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speaker_embedding_ge2e_loss_amd import _lib  # noqa: E402
from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402
from speaker_embedding_ge2e_loss_amd.evaluation import THRESHOLDS  # noqa: E402

K, D, R = 1251, 256, 16384
EPS, EPS_COS = GF.SMALL_ERR, GF.EPS_COS


def make(dev):
    g = torch.Generator(device=dev).manual_seed(1251)
    centre = torch.randn(K + 1, D, generator=g, device=dev)
    rng = np.random.default_rng(1251)
    enrol_lab = torch.as_tensor(np.repeat(np.arange(K), 8), device=dev, dtype=torch.int32)
    lab = rng.integers(0, K, R)
    lab[rng.random(R) < 0.02] = K                                             # unknown speakers: impostors against everybody
    lab_t = torch.as_tensor(lab, device=dev, dtype=torch.int64)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1).contiguous()    # noqa: E731
    enrol = unit(centre[enrol_lab.long()] + 0.5 * torch.randn(len(enrol_lab), D, generator=g, device=dev))
    e = unit(centre[lab_t] + 0.5 * torch.randn(R, D, generator=g, device=dev))
    sums, cnt = torch.zeros(K, D, device=dev), torch.zeros(K, dtype=torch.int32, device=dev)
    GF.enroll_accumulate(sums, cnt, enrol, enrol_lab)
    return e, lab_t, GF.enroll_finalize(sums, cnt), cnt


def torch_scores(e, models):
    return torch.nn.functional.normalize(e, dim=-1, eps=EPS_COS) @ models.t() + EPS


def torch_route(e, lab, models, thr, loop):
    s = torch_scores(e, models)
    known = lab < K
    own = torch.zeros_like(s, dtype=torch.bool)
    own[known, lab[known]] = True
    if loop:
        total = torch.stack([(s > t).sum() for t in thr])
        ta = torch.stack([((s > t) & own).sum() for t in thr])
    else:
        acc = s.unsqueeze(-1) > thr
        total = acc.sum(dim=(0, 1))
        ta = (acc & own.unsqueeze(-1)).sum(dim=(0, 1))
    return torch.stack([total - ta, ta], dim=-1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=60)
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_enroll_verify.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    faulthandler.dump_traceback_later(args.step_timeout, exit=True)
    e, lab, models, cnt = make(dev)
    lab32 = lab.to(torch.int32)
    thr = torch.as_tensor(THRESHOLDS, dtype=torch.float64).to(torch.float32).to(dev)
    T = thr.numel()
    lib = _lib.load()
    scores = torch.empty(R, K, device=dev)
    counts = torch.empty(T, 2, dtype=torch.int32, device=dev)
    trials = torch.empty(2, dtype=torch.int32, device=dev)
    last = {}

    def form(name, with_counts, f):
        def run():
            args_ = (e.data_ptr(), lab32.data_ptr() if with_counts else None, models.data_ptr(), cnt.data_ptr(), K, R, D, EPS_COS,
                     EPS, thr.data_ptr() if with_counts else None, T if with_counts else 0,
                     None if with_counts else scores.data_ptr(), counts.data_ptr() if with_counts else None,
                     trials.data_ptr() if with_counts else None, None, f)
            _lib.check(lib.ge2e_selftest_verify_form(*args_), name)
            if with_counts:
                last[name] = counts.clone()
        return name, run

    def counts_only():
        last["counts_only"] = GF.verify_scores(e, models, cnt, labels=lab32, thresholds=thr, need_scores=False).counts

    def scores_and_counts():
        last["scores_and_counts"] = GF.verify_scores(e, models, cnt, labels=lab32, thresholds=thr).counts

    def scores_alone():
        last["scores"] = GF.verify_scores(e, models, cnt).scores

    def matmul():
        last["torch_scores"] = torch_scores(e, models)

    def route():
        last["torch_route"] = torch_route(e, lab, models, thr, False)

    def route_loop():
        last["torch_route_loop"] = torch_route(e, lab, models, thr, True)

    points = [("counts_only", counts_only), ("scores_and_counts", scores_and_counts), ("scores_alone", scores_alone),
              ("torch_scores", matmul), ("torch_route", route), ("torch_route_loop", route_loop),
              form("counts_only_staged", True, 1), form("counts_only_streamed", True, 2),
              form("scores_alone_staged", False, 1), form("scores_alone_streamed", False, 2)]
    for name, fn in points:
        faulthandler.dump_traceback_later(args.step_timeout, exit=True)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    for name in ("scores_and_counts", "counts_only_staged", "counts_only_streamed"):
        assert torch.equal(last["counts_only"], last[name]), f"counts_only and {name} differ"
    err = float((last["scores"] - torch_scores(e, models)).abs().max())
    off = {k: int((last[k] != last["counts_only"]).sum()) for k in ("torch_route", "torch_route_loop")}
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.rounds)]
          for name, _ in points}
    for i in range(args.rounds):
        faulthandler.dump_traceback_later(args.step_timeout, exit=True)
        for name, fn in points:
            torch.cuda.synchronize()      # every call starts on an idle queue: its own time, not its place in a backlog
            e0, e1 = ev[name][i]
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()
    med = {}
    for name, _ in points:
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]) * 1e3
        med[name] = float(np.median(t))
        print(json.dumps({"point": name, "K": K, "R": R, "D": D, "T": T, "rounds": args.rounds,
                          "call_us_median": round(med[name], 2), "call_us_min": round(float(t.min()), 2),
                          "call_us_max": round(float(t.max()), 2)}), flush=True)
    print(json.dumps({"accepts_at_first_threshold": last["counts_only"][0].tolist(), "trials": trials.tolist(),
                      "max_abs_scores_minus_torch": err, "counts_differing_from_the_library": off,
                      "counts_only_over_torch_route": round(med["counts_only"] / med["torch_route"], 4),
                      "counts_only_over_torch_route_loop": round(med["counts_only"] / med["torch_route_loop"], 4),
                      "scores_alone_over_torch_scores": round(med["scores_alone"] / med["torch_scores"], 4),
                      "counts_only_staged_over_streamed": round(med["counts_only_staged"] / med["counts_only_streamed"], 4),
                      "scores_alone_staged_over_streamed": round(med["scores_alone_staged"] / med["scores_alone_streamed"], 4)}),
          flush=True)


if __name__ == "__main__":
    main()
