"""Forward + backward batches/s of the ragged loss kernel against its fixed-shape neighbours, event-timed on one GPU, at
R = 640 rows, D = 256, B = 4096 batches per launch (E and dE: 2.7 GB each, far beyond the Infinity Cache):
  (a) ragged_equal    ge2e_loss_fwd_bwd_ragged, 64 speakers x 10 utterances (what the dense kernels compute)
  (b) ragged_drawn    ge2e_loss_fwd_bwd_ragged, 64 speakers with a seeded draw of counts in 2..18 summing to 640,
                      another draw for every batch of the launch
  (c) generic         GE2E_IMPL_GENERIC   (the exact-fp32 VALU kernel of the same structure) on (a)'s data as (64, 10, 256)
  (d) fused_f32       GE2E_IMPL_FUSED_F32 (exact-fp32 MFMA, one workgroup per batch, LDS-resident) on the same data
all in one process.  Per point: warm-up launches, then `--launches` (>= 20) launches each between its own pair of events;
the median is reported.  One JSON line per point on stdout.

usage: python tools/bench_ragged.py [--launches 20] [--batches 4096]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

N, M, D = 64, 10, 256
R = N * M


def drawn_counts(rng):
    """N counts in 2..18 that sum to R: a uniform draw, then single steps at random speakers until the sum fits."""
    c = rng.integers(2, 19, size=N)
    while c.sum() != R:
        j = rng.integers(N)
        step = 1 if c.sum() < R else -1
        if 2 <= c[j] + step <= 18:
            c[j] += step
    return c


def timed(fn, launches, warmup=3):
    """Median seconds per launch over `launches` launches, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = np.array([e0.elapsed_time(e1) for e0, e1 in ev]) * 1e-3
    return float(np.median(t)), float(t.min()), float(t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batches", type=int, default=4096)
    args = ap.parse_args()
    if args.launches < 20:
        raise SystemExit("--launches must be at least 20 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    B = args.batches
    w, b = torch.tensor(10.0, device=dev), torch.tensor(-5.0, device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    E = torch.nn.functional.normalize(torch.randn(B, R, D, generator=g, device=dev), dim=-1)
    z = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = GF.LossOutputs(loss=z(B), per=None, dE=torch.empty_like(E), dw=z(B), db=z(B))
    out4 = GF.LossOutputs(loss=out.loss, per=None, dE=out.dE.view(B, N, M, D), dw=out.dw, db=out.db)
    rng = np.random.default_rng(1234)
    equal = GF.ragged_offsets([[M] * N] * B, R).to(dev)
    drawn = GF.ragged_offsets(np.stack([drawn_counts(rng) for _ in range(B)]), R).to(dev)
    points = [("ragged_equal", lambda: GF.loss_fwd_bwd_ragged(E, equal, w, b, out=out)),
              ("ragged_drawn", lambda: GF.loss_fwd_bwd_ragged(E, drawn, w, b, out=out)),
              ("generic", lambda: GF.loss_fwd_bwd(E.view(B, N, M, D), w, b, impl="generic", out=out4)),
              ("fused_f32", lambda: GF.loss_fwd_bwd(E.view(B, N, M, D), w, b, impl="fused_f32", out=out4))]
    rates = {}
    for name, fn in points:
        med, lo, hi = timed(fn, args.launches)
        rates[name] = B / med
        print(json.dumps({"point": name, "B": B, "R": R, "N": N, "D": D, "launches": args.launches,
                          "batches_per_s": round(B / med, 1), "launch_ms_median": round(med * 1e3, 3),
                          "launch_ms_min": round(lo * 1e3, 3), "launch_ms_max": round(hi * 1e3, 3),
                          "loss_batch0": float(out.loss[0])}), flush=True)
    print(json.dumps({"ragged_equal_over_generic": round(rates["ragged_equal"] / rates["generic"], 3),
                      "ragged_equal_over_fused_f32": round(rates["ragged_equal"] / rates["fused_f32"], 3),
                      "ragged_drawn_over_ragged_equal": round(rates["ragged_drawn"] / rates["ragged_equal"], 3)}), flush=True)


if __name__ == "__main__":
    main()
