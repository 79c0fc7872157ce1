"""Encoder inference: SpeakerEncoder.embed(native=True) -- one HIP launch -- against the parent commit's route,
SpeakerEncoder.forward under no_grad (nn.LSTM through MIOpen, nn.Linear, three torch ops for the norm).

    python tools/bench_encoder.py [--rounds 10] [--warmup 3] [--shapes 16,640,8192]
    python tools/bench_encoder.py --diagnose 2048,8192

The model is the reference's: 80 mels -> 3 x LSTM(256) -> Linear 256, windows of T = 160 frames.  R = 16 is the online
case, R = 640 one N = 64, M = 10 batch, R = 8192 bulk (every CU holds a tile).  Every call is timed between its own pair of
HIP events on an idle queue, after the warm-ups; one JSON line per point with the median, windows/s and, for the native
call, its fraction of the exact-fp32 matrix ceiling: 155 TF / 445 MFLOP per window = 350 k windows/s."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder  # noqa: E402

CEILING = 350e3   # windows/s: 155e12 / (2 * 160 * 4 * 256 * ((80 + 256) + 2 * (256 + 256)) + 2 * 256 * 256)


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


def diagnose(model, R, T, dev):
    """Where the two routes disagree, who is right: 32 windows of one batch of R, encoded in the batch and alone, by both
    routes, against the module's float32 copy on the CPU."""
    import copy
    x = torch.rand(R, T, 80, device=dev) * 0.96
    with torch.no_grad():
        want = model(x)
    got = model.embed(x, native=True)
    cpu = copy.deepcopy(model).cpu()
    off = int(((got - want).norm(dim=1) > 1e-4).sum())
    print(json.dumps({"diagnose_R": R, "rows_where_the_routes_differ_by_more_than_1e-4": off}), flush=True)
    for a in (0, R // 2, R - 32):
        part = x[a:a + 32].contiguous()
        with torch.no_grad():
            t_alone = model(part)
            ref = cpu(part.cpu()).double()
        rel = lambda e: float(f"{float((e.cpu().double() - ref).norm() / ref.norm()):.3e}")   # noqa: E731
        print(json.dumps({"diagnose_R": R, "rows": [a, a + 32],
                          "native_alone_same_bits_as_in_batch": bool(torch.equal(model.embed(part, native=True), got[a:a + 32])),
                          "torch_alone_against_in_batch_max_abs": float(f"{float((t_alone - want[a:a + 32]).abs().max()):.3e}"),
                          "native_in_batch_against_cpu_rel": rel(got[a:a + 32]),
                          "torch_in_batch_against_cpu_rel": rel(want[a:a + 32])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="16,640,8192")
    ap.add_argument("--points", default="native,torch")
    ap.add_argument("--diagnose", default="", help="batch sizes at which to check both routes against the CPU module instead")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SpeakerEncoder(80, 256, 3, 256).to(dev).eval()
    T = 160
    if args.diagnose:
        for R in (int(s) for s in args.diagnose.split(",")):
            diagnose(model, R, T, dev)
        return
    for R in (int(s) for s in args.shapes.split(",")):
        x = torch.rand(R, T, 80, device=dev) * 0.96
        with torch.no_grad():
            want = model(x)
        got = model.embed(x, native=True)
        err = float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
        res = {}
        for point in args.points.split(","):
            if point == "native":
                us = timed(lambda: model.embed(x, native=True), args.rounds, args.warmup)
            else:
                def fwd():
                    with torch.no_grad():
                        return model(x)
                us = timed(fwd, args.rounds, args.warmup)
            med = statistics.median(us)
            res[point] = med
            line = {"R": R, "T": T, "point": point, "rounds": args.rounds, "call_us_median": round(med, 1),
                    "call_us_min": round(min(us), 1), "call_us_max": round(max(us), 1), "windows_per_s": round(R / med * 1e6)}
            if point == "native":
                line["fraction_of_fp32_matrix_ceiling"] = round(R / med * 1e6 / CEILING, 4)
            print(json.dumps(line), flush=True)
        summary = {"R": R, "native_against_torch_rel_err": float(f"{err:.3e}")}
        if "native" in res and "torch" in res:
            summary["native_over_torch"] = round(res["native"] / res["torch"], 4)
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
