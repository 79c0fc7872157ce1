"""Resampling and gain: functional.resample -- one HIP launch -- against its own torch route on the same device (a strided
conv1d with `up` output channels over the zero-padded utterance), which is what a caller without the kernel would write; and
functional.volume_gain -- two launches -- against audio.volume_gain (float64 square and cumsum of the whole buffer).

    python tools/bench_resample.py [--rates 48000,44100] [--seconds 1,60,3600] [--rounds 100,30,5] [--warmup 3]
                                   [--batch 1000,10000] [--batch-rounds 10]

One utterance of noise of 1 s (the online case), 1 min and 1 h (bulk) at every source rate, to 16 kHz with kaiser_best, and
a batch of 1 000 utterances of 1 s in one call (the front end's usual shape); the gain at 16 kHz on the same lengths and on
a batch of 10 000 utterances of 1 s.  Every point runs in a child process of its own (a fresh allocator and library cache), one at
a time; the layout tables, the output and the gain's workspace are made beforehand for both routes; every call is timed
between its own pair of HIP events on an idle queue, after the warm-ups.  The two routes' outputs are compared before
anything is timed and must agree within twice the bound each has against the exact result; a point that misses is not timed.  One JSON line per point with the median and, for the native resampler, what the algorithm needs over the
call time: W FMAs per output; 4 bytes per sample read once and 4 per output written.  A route that cannot run a size (the
conv1d may want more memory than the device has) is reported as such, not timed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, rounds, warmup):
    import torch
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


def child(kind, rate, secs, utts, rounds, warmup):
    import torch
    from speaker_embedding_ge2e_loss_amd import _lib, audio
    from speaker_embedding_ge2e_loss_amd import functional as GF
    dev = torch.device("cuda:0")
    torch.manual_seed(secs)
    line = {"kind": kind, "source_rate": rate, "seconds": secs, "utterances": utts, "rounds": rounds}
    if kind == "resample":
        bank = audio.resample_bank(rate, 16000, "kaiser_best")
        t = GF.resample_pack(bank.taps.to(dev), bank.up, bank.down, bank.lead)
        n = secs * rate
        wav = 0.1 * torch.randn(n * utts, device=dev)
        lay = GF.resample_layout([n] * utts, bank.up, bank.down, device=dev)
        total = lay.out_start[-1]
        out = {p: torch.empty(total, device=dev) for p in ("native", "torch")}
        calls = {"native": lambda: GF.resample(t, wav, layout=lay, out=out["native"], native=True),
                 "torch": lambda: GF.resample(t, wav, layout=lay, out=out["torch"], native=False)}
        line.update(samples=n * utts, outputs=total, width=t.width,
                    plan=_lib.resample_plan(utts, total, bank.up, bank.down, bank.lead)[0])
    else:
        n = secs * 16000
        wav = 0.01 * torch.randn(n * utts, device=dev)
        lay = GF.resample_layout([n] * utts, 1, 1, device=dev)
        out = {"native": torch.empty(utts, device=dev)}
        ws = GF.volume_gain_workspace(n * utts, utts, dev)
        calls = {"native": lambda: GF.volume_gain(wav, layout=lay, out=out["native"], workspace=ws),
                 "torch": lambda: out.__setitem__("torch", audio.volume_gain(wav, [n] * utts))}
        line.update(samples=n * utts)
    res = {}
    for point, call in calls.items():
        try:
            call()
            torch.cuda.synchronize()
        except RuntimeError as ex:                        # (torch's out-of-memory error is a RuntimeError)
            res[point] = None
            line[point + "_failed"] = str(ex).splitlines()[0][:160]
    if not any(k.endswith("_failed") for k in line):
        # Both routes are within their bound of the exact result, so of each other within twice it.  Resampling: an output
        # is a W-term fp32 dot product, (W + 1) 2^-24 sum |taps x| in any order; that sum comes from the kernel itself on
        # |taps| and |x| (every term positive: its own error is a part in 10^5).  The gain: both are float32 roundings of a
        # double result.  A route that misses is not timed.
        diff = (out["native"] - out["torch"]).abs()
        if kind == "resample":
            mag, _ = GF.resample(GF.resample_pack(bank.taps.abs().to(dev), bank.up, bank.down, bank.lead), wav.abs(), layout=lay)
            bound = 2.0 * (t.width + 1) * 2.0 ** -24 * 1.001 * mag
        else:
            bound = 4.0 * 2.0 ** -24 * out["torch"].abs()
        line["native_against_torch_max_abs"] = float(f"{float(diff.max()):.3e}")
        line["native_against_torch_of_bound"] = float(f"{float((diff / bound.clamp_min(1e-30)).max()):.3f}")
        assert bool((diff <= bound).all()), f"the two routes differ by more than their bound: {line}"
        del diff, bound
    for point, call in calls.items():
        if point + "_failed" in line:
            continue
        us = timed(call, rounds, warmup)
        res[point] = statistics.median(us)
        line[point + "_us_median"] = round(res[point], 1)
        line[point + "_us_min"] = round(min(us), 1)
        line[point + "_us_max"] = round(max(us), 1)
    if res.get("native") and kind == "resample":
        line["algorithm_gfma_per_s"] = round(line["outputs"] * line["width"] / res["native"] * 1e-3, 1)
        line["algorithm_gbytes_per_s"] = round(4 * (line["samples"] + line["outputs"]) / res["native"] * 1e-3, 1)
    if res.get("native") and kind == "gain":
        line["algorithm_gbytes_per_s"] = round(4 * line["samples"] / res["native"] * 1e-3, 1)
    if res.get("native") and res.get("torch"):
        line["native_over_torch"] = round(res["native"] / res["torch"], 4)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", default="48000,44100")
    ap.add_argument("--seconds", default="1,60,3600")
    ap.add_argument("--rounds", default="100,30,5")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", default="1000,10000", help="utterances of 1 s in one call: resampling, gain (0: none)")
    ap.add_argument("--batch-rounds", type=int, default=10)
    ap.add_argument("--child", nargs=5, metavar=("KIND", "RATE", "SECONDS", "UTTERANCES", "ROUNDS"))
    args = ap.parse_args()
    if args.child:
        kind, rate, secs, utts, rounds = args.child
        return child(kind, int(rate), int(secs), int(utts), int(rounds), args.warmup)
    sizes = [(secs, "1", rounds) for secs, rounds in zip(args.seconds.split(","), args.rounds.split(","))]
    batch_resample, batch_gain = (int(v) for v in args.batch.split(","))
    points = []
    for r in args.rates.split(","):
        points += [("resample", r) + s for s in sizes]
        if batch_resample:
            points.append(("resample", r, "1", str(batch_resample), str(args.batch_rounds)))
    points += [("gain", "16000") + s for s in sizes]
    if batch_gain:
        points.append(("gain", "16000", "1", str(batch_gain), str(args.batch_rounds)))
    for point in points:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--child", *point],
                            timeout=600).returncode
        if rc != 0:                                       # nothing more is started on the device after a failed child
            print(json.dumps({"point": point, "child_exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
