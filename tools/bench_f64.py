"""Forward + backward batches/s of the double-precision loss against its two neighbours, event-timed on one GPU:
  (a) f64_kernel   ge2e_loss_fwd_bwd_f64 (functional.loss_fwd_bwd on float64 tensors)
  (b) torch_expand the reference-equivalent float64 expand form (oracle.expand_form_loss on device tensors + backward()):
                   what a float64 caller of the reference runs; it materialises the two (N M N, D) operands
  (c) generic_f32  the project's exact-fp32 VALU kernel (impl="generic"), for scale
at (N, M, D) = (4,5,256), (64,10,256), (256,10,256).  (a) and (c) are timed at B = 1 and at a B whose embeddings alone
exceed the 256 MiB Infinity Cache (E and dE stream from HBM); (b) takes one batch per call, so its rate is 1 / call time.
Per point: warm-up calls, then >= 20 timed calls between two events, repeated; the median is reported.
One JSON line per shape on stdout.

usage: python tools/bench_f64.py [--calls 20] [--repeats 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import ge2e_oracle as orc  # noqa: E402
from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

SHAPES = [(4, 5, 256), (64, 10, 256), (256, 10, 256)]
CACHE_BYTES = 256 << 20


def timed(fn, calls, repeats, warmup=3):
    """Median over `repeats` windows of `calls` calls each, in seconds per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / calls * 1e-3)
    return float(np.median(res))


def kernel_rate(E, w, b, impl, calls, repeats):
    B = E.shape[0]
    z = lambda *s: torch.empty(*s, dtype=E.dtype, device=E.device)  # noqa: E731
    out = GF.LossOutputs(loss=z(B), per=None, dE=torch.empty_like(E), dw=z(B), db=z(B))
    t = timed(lambda: GF.loss_fwd_bwd(E, w, b, impl=impl, out=out), calls, repeats)
    return B / t, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f64.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    w64 = torch.tensor(10.0, device=dev, dtype=torch.float64)
    b64 = torch.tensor(-5.0, device=dev, dtype=torch.float64)
    w32, b32 = w64.float(), b64.float()
    for (N, M, D) in SHAPES:
        big = -(-(CACHE_BYTES * 5 // 4) // (N * M * D * 8))     # float64 embeddings of 320 MiB
        g = torch.Generator(device=dev).manual_seed(1234)
        E64 = torch.nn.functional.normalize(torch.randn(big, N, M, D, generator=g, device=dev, dtype=torch.float64), dim=-1)
        E32 = E64.float()
        line = {"shape": [N, M, D], "large_B": big, "calls": args.calls, "repeats": args.repeats}
        for name, E, w, b, impl in (("f64_kernel", E64, w64, b64, "auto"), ("generic_f32", E32, w32, b32, "generic")):
            r1, t1 = kernel_rate(E[:1], w, b, impl, args.calls, args.repeats)
            rb, tb = kernel_rate(E, w, b, impl, args.calls, args.repeats)
            line[name] = {"B1_batches_per_s": round(r1, 1), "B1_call_us": round(t1 * 1e6, 1),
                          "large_B_batches_per_s": round(rb, 1), "large_B_call_ms": round(tb * 1e3, 3)}

        e1 = E64[0].clone().requires_grad_(True)
        wt, bt = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)

        def expand_step():
            e1.grad = wt.grad = bt.grad = None
            orc.expand_form_loss(e1, wt, bt)[0].backward()

        t = timed(expand_step, args.calls, args.repeats)
        line["torch_expand_f64"] = {"B1_batches_per_s": round(1.0 / t, 1), "B1_call_us": round(t * 1e6, 1)}
        # the three compute the same thing: the timed kernels' losses against the expand form's
        lk = GF.loss_fwd_bwd(E64[:1], w64, b64, need_grad=False).loss[0]
        le = orc.expand_form_loss(E64[0], w64, b64)[0]
        line["loss_rel_diff_f64_kernel_vs_expand"] = float((lk - le).abs() / le.abs())
        line["speedup_f64_kernel_over_expand_B1"] = round(line["f64_kernel"]["B1_batches_per_s"] / line["torch_expand_f64"]["B1_batches_per_s"], 2)
        line["speedup_f64_kernel_over_expand_large_B"] = round(
            line["f64_kernel"]["large_B_batches_per_s"] / line["torch_expand_f64"]["B1_batches_per_s"], 2)
        print(json.dumps(line), flush=True)
        del E64, E32


if __name__ == "__main__":
    main()
