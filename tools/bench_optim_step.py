"""The training step's last statements, torch's route against the native call, on the same GPU in the same process.

    python tools/bench_optim_step.py [--rounds 30] [--calls 20] [--warmup 5] [--out profiles/optim_step_bench.txt]

torch:   flat_grad.div_(world); clip_grad_norm_(encoder, 3.0); clip_grad_norm_(loss, 1.0); torch.optim.SGD.step()
native:  functional.sgd_clip_step over the same kind of flat bucket (two HIP launches), and optim.ClipSGD.step() around it
         (the Optimizer's step hooks, the check that every .grad still lies in the bucket, the comparison of the host's
         hyper-parameters with the device table)

at two parameter lists: the reference encoder's (80 mels, 3 x 256 LSTM, 256-d projection: 1 464 576 elements)
plus the loss's (w, b), and the golden fixture trainer_tiny's (8 mels, 2 x 16, 16-d) plus (w, b).  Momentum and weight decay
are 0, the reference's settings.  Each route has its own copy of the parameters and its own bucket; the gradients are a
seeded draw whose norms exceed both thresholds, so both clips multiply.

Timing: after the warm-ups the rounds alternate between the routes.  A round of a route is `calls` calls back to back
between one pair of HIP events on an otherwise idle stream (the time a training loop sees per step: the larger of the
host's enqueue time and the device's run time), and the host clock around the same calls before the synchronise (the
enqueue time alone).  Medians over the rounds, per call, in microseconds.  The launch counts come from a profiler run of
three calls per route AFTER the timing (kernels on the device, per call); where the profiler gives no device events the
count is reported as null, not guessed.  One JSON line per parameter list."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLIP_MODEL, CLIP_LOSS, LR, WORLD = 3.0, 1.0, 1e-4, 1.0


def parameter_list(kind, dev):
    import torch
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    torch.manual_seed(0)
    enc = SpeakerEncoder(80, 256, 3, 256) if kind == "reference" else SpeakerEncoder(8, 16, 2, 16)
    model = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in enc.parameters()]
    loss = [torch.nn.Parameter(torch.tensor(v, device=dev)) for v in (10.0, -5.0)]
    return model, loss


def bucket(groups, dev, seed):
    """One flat gradient with every .grad a view of it, filled from a seeded generator."""
    import torch
    params = [p for g in groups for p in g]
    flat = torch.zeros(sum(p.numel() for p in params), device=dev)
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    fill = torch.randn(flat.numel(), device=dev, generator=g)
    return flat, fill


def launches_per_call(fn, calls=3):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        from torch.autograd import DeviceType
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        # (the range Optimizer.step opens around itself shows up among the device events as an annotation: no launch)
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower()
                 and "memset" not in e.name.lower() and not e.name.startswith("Optimizer.")]
        print(f"profiler: {len(names)} device events in {calls} calls: {sorted(set(names))}", file=sys.stderr)
        return round(len(names) / calls, 2) if names else None
    except Exception as ex:                               # no device tracing on this installation
        print(f"profiler: {type(ex).__name__}: {str(ex)[:120]}", file=sys.stderr)
        return None


def measure(kind, rounds, calls, warmup):
    import torch
    from speaker_embedding_ge2e_loss_amd import functional as GF
    from speaker_embedding_ge2e_loss_amd.optim import ClipSGD
    dev = torch.device("cuda:0")

    t_model, t_loss = parameter_list(kind, dev)
    t_flat, fill = bucket([t_model, t_loss], dev, 1)
    t_opt = torch.optim.SGD([{"params": t_model}, {"params": t_loss}], lr=LR)

    def torch_route():
        t_flat.div_(WORLD)
        torch.nn.utils.clip_grad_norm_(t_model, CLIP_MODEL)
        torch.nn.utils.clip_grad_norm_(t_loss, CLIP_LOSS)
        t_opt.step()

    n_model, n_loss = parameter_list(kind, dev)
    n_flat, _ = bucket([n_model, n_loss], dev, 1)
    offsets, off = [], 0
    for g in (n_model, n_loss):
        offsets.append([])
        for p in g:
            offsets[-1].append(off)
            off += p.numel()
    lay = GF.sgd_layout([n_model, n_loss], offsets)
    hyper = torch.tensor([[LR, CLIP_MODEL, 0, 0], [LR, CLIP_LOSS, 0, 0]], device=dev)

    def native_call():
        GF.sgd_clip_step(lay, n_flat, hyper, grad_scale=1.0 / WORLD)

    o_model, o_loss = parameter_list(kind, dev)
    o_opt = ClipSGD([{"params": o_model}, {"params": o_loss}], lr=LR, max_norm=(CLIP_MODEL, CLIP_LOSS), grad_scale=1.0 / WORLD)
    o_flat = o_opt.flat_grad

    routes = {"torch": (torch_route, t_flat), "native_call": (native_call, n_flat), "clip_sgd_step": (o_opt.step, o_flat)}
    # the same step from the same start on every route, compared before anything is timed
    for fn, flat in routes.values():
        flat.copy_(fill)
        fn()
    torch.cuda.synchronize()
    worst = 0.0
    for a, b, c in zip(t_model + t_loss, n_model + n_loss, o_model + o_loss):
        assert torch.equal(b, c), "functional.sgd_clip_step and ClipSGD.step disagree"
        # each route rounds p' once (2^-24 |p'| each) and has its step lr g good to 1e-5 (the coefficient's tolerance)
        bound = 2.0 ** -23 * a.detach().abs() + 2e-5 * LR * a.grad.abs().max()
        worst = max(worst, float(((a.detach() - b.detach()).abs() / bound).max()))
    assert worst <= 1.0, worst

    for _ in range(warmup):
        for fn, flat in routes.values():
            flat.copy_(fill)
            fn()
    torch.cuda.synchronize()
    event_us, host_us = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(rounds):
        for k, (fn, flat) in routes.items():
            flat.copy_(fill)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            event_us[k].append(a.elapsed_time(b) * 1e3 / calls)
            host_us[k].append((t1 - t0) * 1e6 / calls)
    line = {"parameters": kind, "tensors": len(t_model) + 2, "elements": int(t_flat.numel()), "chunks": lay.C,
            "plan": ",".join(GF.sgd_clip_plan(lay)), "rounds": rounds, "calls_per_round": calls,
            "update_disagreement_over_bound": round(worst, 4)}
    for k in routes:
        line[k] = {"event_us": round(statistics.median(event_us[k]), 2), "host_enqueue_us": round(statistics.median(host_us[k]), 2),
                   "event_us_min_max": [round(min(event_us[k]), 2), round(max(event_us[k]), 2)]}
    for k, (fn, flat) in routes.items():
        flat.copy_(fill)
        line[k]["launches_per_call"] = launches_per_call(fn)
    for k in ("native_call", "clip_sgd_step"):
        line[k]["over_torch"] = round(line[k]["event_us"] / line["torch"]["event_us"], 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_optim_step needs the GPU: a CPU run has no time to report")
    lines = [json.dumps(measure(kind, args.rounds, args.calls, args.warmup)) for kind in ("reference", "trainer_tiny")]
    for text in lines:
        print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
