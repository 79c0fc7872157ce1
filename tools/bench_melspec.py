"""Mel front end: functional.melspec -- one HIP launch -- against its own torch route on the same device (reflect pad,
unfold, torch.fft.rfft, abs, matmul, log10, clamp), which is what a caller without the kernel would write.

    python tools/bench_melspec.py [--seconds 1,60,3600] [--rounds 200,50,10] [--warmup 5]

The settings are the reference's: 16 kHz, n_fft 1024, hop 128, 80 Slaney mel channels, dB mode.  One utterance of about
1 s (the online case), 1 min and 1 h (bulk) of noise.  The layout tables and the output are made beforehand for both routes;
every call is timed between its own pair of HIP events on an idle queue, after the warm-ups; one JSON line per point with
the median, frames/s and, for the native call, what the algorithm needs over the call time: 5 H log2 H flops of a
512-point complex FFT, 12 H of the post-pass and magnitudes and 2 x 516 x 80 of the padded mel product per frame; 4 bytes per
sample read once plus 4 x 80 bytes per frame written.  The two routes' outputs are compared before anything is timed."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402
from speaker_embedding_ge2e_loss_amd.audio import MelFrontEnd  # noqa: E402


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="1,60,3600")
    ap.add_argument("--rounds", default="200,50,10")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", default="native,torch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fe = MelFrontEnd()                                   # the reference's settings
    tables = fe.tables(dev)
    n_fft, hop, n_mels, H = fe.n_fft, fe.hop_length, fe.n_mels, fe.n_fft // 2
    flops_per_frame = 5 * H * math.log2(H) + 12 * H + 2 * (H + 4) * n_mels
    for secs, rounds in zip((int(s) for s in args.seconds.split(",")), (int(r) for r in args.rounds.split(","))):
        n = secs * fe.sampling_rate
        torch.manual_seed(secs)
        wav = 0.1 * torch.randn(n, device=dev)
        lay = GF.melspec_layout([n], hop=hop, n_fft=n_fft, device=dev)
        frames = lay.frame_start[-1]
        out = {p: torch.empty(frames, n_mels, device=dev) for p in ("native", "torch")}
        calls = {"native": lambda: GF.melspec(tables, wav, hop=hop, layout=lay, out=out["native"], native=True),
                 "torch": lambda: GF.melspec(tables, wav, hop=hop, layout=lay, out=out["torch"], native=False)}
        for c in calls.values():
            c()
        torch.cuda.synchronize()
        diff = float((out["native"] - out["torch"]).abs().max())
        res = {}
        for point in args.points.split(","):
            us = timed(calls[point], rounds, args.warmup)
            med = statistics.median(us)
            res[point] = med
            line = {"seconds": secs, "samples": n, "frames": frames, "point": point, "rounds": rounds,
                    "call_us_median": round(med, 1), "call_us_min": round(min(us), 1), "call_us_max": round(max(us), 1),
                    "frames_per_s": round(frames / med * 1e6), "audio_seconds_per_s": round(secs / med * 1e6, 1)}
            if point == "native":
                line["algorithm_gflops"] = round(frames * flops_per_frame / med * 1e-3, 1)
                line["algorithm_gbytes_per_s"] = round((4 * n + 4 * n_mels * frames) / med * 1e-3, 1)
            print(json.dumps(line), flush=True)
        summary = {"seconds": secs, "native_against_torch_max_abs_db": float(f"{diff:.3e}")}
        if "native" in res and "torch" in res:
            summary["native_over_torch"] = round(res["native"] / res["torch"], 4)
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
