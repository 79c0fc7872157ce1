"""Silence trimming: functional.vad_flags (two launches), vad_mask (one), the ge2e_vad_trim launch and trim_silences as a
whole (four launches and one read-back of U lengths) against their torch routes on the same device (native=False: the
windows as rows of an `unfold` view, int64 sums, a sliding minimum by doubling, `cumsum` masks, an indexed gather), which is
what a caller without the kernels would write.

    python tools/bench_vad.py [--hours 1] [--rounds 10] [--warmup 3] [--embed-utterances 64]

One hour of 16 kHz audio from a seeded generator -- noise of amplitude 0.1 for half a second, of 0.0003 for the next half,
and so on: half of it silence -- in three arrangements: 360 utterances of 10 s, 3 600 of 1 s, one utterance.  The
reference's settings: windows of 480 samples, moving average 8, max silence 6, and the detector's defaults.  Every
arrangement runs in a child process of its own, one at a time; the layout is made beforehand; the two routes' flags, ranks,
lengths and trimmed samples are compared for equality before anything is timed; the rounds alternate between the two
routes, every call between its own pair of HIP events on an idle queue, after the warm-ups.  One JSON line per arrangement:
medians in microseconds, native over torch, and for the kernels the bytes the algorithm needs over the call time (every
sample read once for the energies; every kept sample read and written once); trim_silences also with native=None ("auto":
the kernels, and torch's ops for the mask of a very long utterance).  A last child times
SpeakerEncoder.embed_audio on 64 utterances of 10 s with and without trim_silences: the cost of the stage and its read-back
in the pipeline."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR, S, A, SILENCE = 16000, 480, 8, 6


def make_audio(seconds, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seconds)
    n = seconds * SR
    level = torch.where((torch.arange(n, device=dev) // (SR // 2)) % 2 == 0, 0.1, 0.0003)
    return torch.randn(n, device=dev, generator=g) * level


def alternate(calls, rounds, warmup):
    """{name: [us]}: the calls in turn, round after round, each between its own events."""
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return us


def child_stages(utts, seconds, rounds, warmup):
    import torch
    from speaker_embedding_ge2e_loss_amd import _lib
    from speaker_embedding_ge2e_loss_amd import functional as GF
    dev = torch.device("cuda:0")
    n = seconds * SR // utts
    wav = make_audio(seconds, dev)
    lengths = [n] * utts
    lay = GF.vad_layout(lengths, S, device=dev)
    total = lay.total_windows
    line = {"utterances": utts, "seconds_each": n / SR, "samples": n * utts, "windows": total, "rounds": rounds,
            "plan": ",".join(_lib._plan(_lib.load().ge2e_vad_plan, utts, total, S, 100, A, SILENCE))}
    flags = {r: GF.vad_flags(wav, window=S, layout=lay, native=r) for r in (True, False)}
    masks = {r: GF.vad_mask(flags[r], lay, A, SILENCE, native=r) for r in (True, False)}
    whole = {r: GF.trim_silences(wav, window=S, avg_width=A, max_silence=SILENCE, layout=lay, native=r) for r in (True, False)}
    assert torch.equal(flags[True], flags[False]) and torch.equal(masks[True][0], masks[False][0])
    assert torch.equal(masks[True][1], masks[False][1]) and whole[True][1] == whole[False][1]
    assert torch.equal(whole[True][0].view(torch.int32), whole[False][0].view(torch.int32))
    dst, out_len = masks[True]
    kept = int(out_len.sum())
    line.update(voiced_windows=int(flags[True].sum()), kept_samples=kept)
    out = torch.empty(kept, device=dev)
    out_start = (torch.cumsum(out_len, 0) - out_len).contiguous()
    _, _, first = GF._vad_window_index(lay)
    ws = torch.empty(total, dtype=torch.int64, device=dev)
    stream = GF._stream_ptr(wav)
    stages = {
        "flags": {"native": lambda: GF.vad_flags(wav, window=S, layout=lay, native=True, workspace=ws),
                  "torch": lambda: GF.vad_flags(wav, window=S, layout=lay, native=False)},
        "mask": {"native": lambda: GF.vad_mask(flags[True], lay, A, SILENCE, native=True),
                 "torch": lambda: GF.vad_mask(flags[True], lay, A, SILENCE, native=False)},
        "trim": {"native": lambda: GF._launch("ge2e_vad_trim", dev, wav.data_ptr(), lay.utt_start.data_ptr(),
                                              lay.win_start_dev.data_ptr(), dst.data_ptr(), out_start.data_ptr(), utts, total,
                                              S, out.data_ptr(), stream),
                 "torch": lambda: wav.unfold(0, S, 1)[first[dst >= 0]].reshape(-1)},
        "trim_silences": {"native": lambda: GF.trim_silences(wav, window=S, avg_width=A, max_silence=SILENCE, layout=lay, native=True),
                          "torch": lambda: GF.trim_silences(wav, window=S, avg_width=A, max_silence=SILENCE, layout=lay, native=False),
                          # native=None: the kernels, and torch's ops for the mask of a very long utterance
                          "auto": lambda: GF.trim_silences(wav, window=S, avg_width=A, max_silence=SILENCE, layout=lay)},
    }
    need = {"flags": 4 * n * utts, "mask": None, "trim": 8 * kept, "trim_silences": 4 * n * utts + 8 * kept}
    for name, calls in stages.items():
        us = alternate(calls, rounds, warmup)
        med = {k: statistics.median(v) for k, v in us.items()}
        line[name] = {"native_us": round(med["native"], 1), "torch_us": round(med["torch"], 1),
                      "native_us_min_max": [round(min(us["native"]), 1), round(max(us["native"]), 1)],
                      "native_over_torch": round(med["native"] / med["torch"], 4)}
        if "auto" in med:
            line[name]["auto_us"] = round(med["auto"], 1)
        if need[name]:
            gbs = need[name] / med["native"] * 1e-3
            line[name].update(algorithm_gbytes_per_s=round(gbs, 1), of_hbm_peak_8tb=round(gbs / 8000.0, 4))
    print(json.dumps(line), flush=True)


def child_embed(utts, rounds, warmup):
    import torch
    from speaker_embedding_ge2e_loss_amd.audio import MelFrontEnd
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    fe = MelFrontEnd()
    m = SpeakerEncoder(80, 256, 3, 256).to(dev).eval()
    wavs = list(torch.split(make_audio(10 * utts, dev), 10 * SR))
    with torch.no_grad():
        calls = {"plain": lambda: m.embed_audio(wavs, fe), "trimmed": lambda: m.embed_audio(wavs, fe, trim_silences=True)}
        us = alternate(calls, rounds, warmup)
        _, lengths, _ = fe.preprocess(wavs, trim_silences=True)
    med = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps({"embed_audio_utterances": utts, "seconds_each": 10, "rounds": rounds, "kept_fraction": round(sum(lengths) / (10 * SR * utts), 3),
                      "plain_us": round(med["plain"], 1), "trim_silences_us": round(med["trimmed"], 1),
                      "difference_us": round(med["trimmed"] - med["plain"], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--embed-utterances", type=int, default=64)
    ap.add_argument("--child", nargs=2, metavar=("KIND", "UTTERANCES"))
    args = ap.parse_args()
    seconds = 3600 * args.hours
    if args.child:
        kind, utts = args.child
        if kind == "embed":
            return child_embed(int(utts), args.rounds, args.warmup)
        return child_stages(int(utts), seconds, args.rounds, args.warmup)
    points = [("stages", str(seconds // 10)), ("stages", str(seconds)), ("stages", "1")]
    if args.embed_utterances:
        points.append(("embed", str(args.embed_utterances)))
    for point in points:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--hours", str(args.hours), "--rounds", str(args.rounds),
                             "--warmup", str(args.warmup), "--child", *point], timeout=400).returncode
        if rc != 0:                                       # nothing more is started on the device after a failed child
            print(json.dumps({"point": point, "child_exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
