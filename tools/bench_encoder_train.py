"""Encoder training, forward + backward: SpeakerEncoder(native_train=True) -- functional.encode_train, the tape forward and
the HIP backward through time -- against the parent commit's route, the same module with native_train=False (nn.LSTM
through MIOpen both ways, nn.Linear, three torch ops for the norm).  The baseline is torch's route, never the code under test.

    python tools/bench_encoder_train.py [--rounds 5] [--warmup 2] [--shapes 20,640,4096,8192] [--limit 240]

The model is the reference's: 80 mels -> 3 x LSTM(256) -> Linear 256, windows of T = 160 frames.  One step is
``(model(x) * G).sum().backward()`` on fixed x and G: for the native route that is both packs, the tape forward, the
recurrence, four weight-gradient GEMMs and the reduction, with their allocations.  Every point (a batch size and a route)
runs in a child process of its own under its own time limit; every step is timed between its own pair of HIP events after
the warm-ups; one JSON line per point with the median.  At R = 20 both routes' gradients are also compared with the module's
float64 copy on the CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, N_MELS, H, L, D = 160, 80, 256, 3, 256


def child(R, route, rounds, warmup):
    import copy

    import torch

    from speaker_embedding_ge2e_loss_amd import functional as GF
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SpeakerEncoder(N_MELS, H, L, D, native_train=route == "native").to(dev)
    x = torch.rand(R, T, N_MELS, device=dev) * 0.96
    G = torch.randn(R, D, device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        (model(x) * G).sum().backward()

    def timed(fn):
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

    try:
        us = timed(step)
        fwd = statistics.median(timed(lambda: model(x)))   # the forward alone, with its graph (the tape, or torch's reserve)
    except RuntimeError as e:   # an error the library reports (not a fault): the point is recorded and the run goes on
        print(json.dumps({"R": R, "T": T, "route": route, "error": str(e).splitlines()[0][:200]}), flush=True)
        return
    med = statistics.median(us)
    line = {"R": R, "T": T, "route": route, "rounds": rounds, "step_us_median": round(med, 1), "step_us_min": round(min(us), 1),
            "step_us_max": round(max(us), 1), "forward_us_median": round(fwd, 1), "windows_per_s": round(R / med * 1e6),
            "peak_device_MB": round(torch.cuda.max_memory_allocated() / 1e6)}
    if route == "native":
        line["tape_MB"] = round(GF.encode_train_tape_bytes(R, T, N_MELS, H, L, D) / 1e6, 1)
        line["workspace_MB"] = round(GF.encode_bwd_workspace_bytes(R, T, N_MELS, H, L, D) / 1e6, 1)
    if R <= 32:   # the distance of this route's gradients from the module's float64 copy on the CPU
        ref = copy.deepcopy(model).cpu().double()
        ref.zero_grad(set_to_none=True)
        h, _ = ref.LSTM_stack(x.cpu().double())           # (the module's own forward casts to float32, s2:28)
        y = ref.projection(h[:, T - 1])
        (y / torch.norm(y, dim=1).unsqueeze(1) * G.cpu().double()).sum().backward()
        num = sum(float((p.grad.cpu().double() - q.grad).norm() ** 2) for p, q in zip(model.parameters(), ref.parameters()))
        den = sum(float(q.grad.norm() ** 2) for q in ref.parameters())
        line["gradients_against_cpu_float64_rel"] = float(f"{(num / den) ** 0.5:.3e}")
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="20,640,4096,8192")
    ap.add_argument("--routes", default="native,torch")
    ap.add_argument("--limit", type=int, default=240, help="seconds a point may take before it is ended")
    ap.add_argument("--child", nargs=2, metavar=("R", "ROUTE"))
    args = ap.parse_args()
    if args.child:
        child(int(args.child[0]), args.child[1], args.rounds, args.warmup)
        return
    for R in (int(s) for s in args.shapes.split(",")):
        for route in args.routes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--warmup", str(args.warmup),
                   "--child", str(R), route]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = "time limit"
            if rc != 0:   # a point that failed ends the run: nothing more is started on the device
                print(json.dumps({"R": R, "route": route, "failed": rc}), flush=True)
                sys.exit(1)


if __name__ == "__main__":
    main()
