"""What identification against a speaker bank (ge2e_identify) costs on one GPU, against the route a caller had before:
functional.verify_scores(need_scores=True) + torch.topk(k), chunked over R where the R x K matrix does not fit comfortably,
and against a plain F.normalize(e) @ models.T + topk.  All with D = 256, unit models, unit trial rows model + 0.5 noise:
  A  K = 1 251,   R = 16 384, k = 5        the shape of tools/bench_enroll_verify.py
  B  K = 262 144, R = 4 096,  k = 5        a production bank; the routes run in chunks of 512 rows (a 537 MB matrix each)
  C  K = 262 144, R = 16,     k = 5 and 32 the online case: one tile of rows, the split's reason to exist
Points per shape, all bare enqueues on the current stream:
  identify            functional.identify(k, labels): the product call (indices, scores, rank, hist)
  identify_S<n>       ge2e_selftest_identify_slices with n bank slices: n = 1 and the S that W = 256, 512 and 1024 workgroups
                      (one, two and four per CU) give at the shape
  verify_topk         the parent route (chunked at B)
  torch_topk          F.normalize(e) @ models.T + eps, topk (chunked at B)
  verify_scores       (A only) functional.verify_scores() without labels: the matrix alone, the floor of the contraction
Every identify point must return the same bits (asserted); the number of rows whose indices differ from verify_topk's is
reported (torch.topk does not promise the index order of equal scores).  All in one process, the points of a shape taken in
turn round after round, each call between its own pair of HIP events on an idle queue after 10 warm-up rounds; median / min /
max per point.  Every warm-up and every timed round runs under a watchdog (--step-timeout seconds) that ends the process.
One JSON line per point and one of ratios per shape on stdout.  profiles/identify_bench.txt holds a run.

usage: python tools/bench_identify.py [--rounds 100] [--step-timeout 120] [--shapes A,B,C]
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

D = 256
EPS, EPS_COS = GF.SMALL_ERR, GF.EPS_COS
SHAPES = {"A": (1251, 16384, (5,), 16384), "B": (262144, 4096, (5,), 512), "C": (262144, 16, (5, 32), 16)}   # K, R, ks, chunk
WS = (256, 512, 1024)


def slices_for(K, R, W):
    G, tiles = -(-K // 64), -(-R // 64)
    S = min(max(-(-W // tiles), 1), G)
    return -(-G // -(-G // S))


def make(dev, K, R):
    g = torch.Generator(device=dev).manual_seed(K + R)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1).contiguous()    # noqa: E731
    models = unit(torch.randn(K, D, generator=g, device=dev))
    lab = torch.randint(0, K, (R,), generator=g, device=dev)
    e = unit(models[lab] + 0.5 * unit(torch.randn(R, D, generator=g, device=dev)))
    return e, lab.to(torch.int32), models, torch.ones(K, dtype=torch.int32, device=dev)


def bench_shape(tag, K, R, k, chunk, rounds, step_timeout, dev):
    e, lab, models, cnt = make(dev, K, R)
    lib = _lib.load()
    last = {}
    idx = torch.empty(R, k, dtype=torch.int32, device=dev)
    score = torch.empty(R, k, device=dev)
    rank = torch.empty(R, dtype=torch.int32, device=dev)
    hist = torch.empty(k + 1, dtype=torch.int32, device=dev)

    def identify():
        last["identify"] = GF.identify(e, models, cnt, k=k, labels=lab)

    def forced(S):
        nbytes = int(lib.ge2e_selftest_identify_workspace_bytes(K, R, D, k, S))
        ws = GF.alloc_workspace(nbytes, dev, init=False)
        name = f"identify_S{S}"

        def run():
            _lib.check(lib.ge2e_selftest_identify_slices(e.data_ptr(), lab.data_ptr(), models.data_ptr(), cnt.data_ptr(), K, R, D, k,
                                                         EPS_COS, EPS, idx.data_ptr(), score.data_ptr(), rank.data_ptr(),
                                                         hist.data_ptr(), ws.data_ptr(), nbytes, None, S), name)
            last[name] = (idx, score, rank, hist)
        return name, run

    def verify_topk():
        vals, inds = [], []
        for r0 in range(0, R, chunk):
            s = GF.verify_scores(e[r0:r0 + chunk], models, cnt).scores
            v, i = torch.topk(s, k, dim=1)
            vals.append(v)
            inds.append(i)
        last["verify_topk"] = (torch.cat(vals), torch.cat(inds))

    def torch_topk():
        vals, inds = [], []
        for r0 in range(0, R, chunk):
            s = torch.nn.functional.normalize(e[r0:r0 + chunk], dim=-1, eps=EPS_COS) @ models.t() + EPS
            v, i = torch.topk(s, k, dim=1)
            vals.append(v)
            inds.append(i)
        last["torch_topk"] = (torch.cat(vals), torch.cat(inds))

    def verify_scores():
        last["verify_scores"] = GF.verify_scores(e, models, cnt).scores

    S_of = {W: slices_for(K, R, W) for W in WS}
    points = [("identify", identify)] + [forced(S) for S in sorted({1, *S_of.values()})]
    points += [("verify_topk", verify_topk), ("torch_topk", torch_topk)]
    if tag == "A":
        points.append(("verify_scores", verify_scores))
    want = None
    for name, fn in points:
        faulthandler.dump_traceback_later(step_timeout, exit=True)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        if name.startswith("identify_S"):                      # every split: the product call's bits
            o = last["identify"]
            want = want or [t.clone() for t in (o.indices, o.scores, o.rank, o.hist)]
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, last[name])), f"{name} differs"
    rows_off = int((last["identify"].indices.long() != last["verify_topk"][1]).any(dim=1).sum())
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for name, _ in points}
    for i in range(rounds):
        faulthandler.dump_traceback_later(step_timeout, exit=True)
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
        print(json.dumps({"shape": tag, "point": name, "K": K, "R": R, "D": D, "k": k, "rounds": rounds,
                          "call_us_median": round(med[name], 2), "call_us_min": round(float(t.min()), 2),
                          "call_us_max": round(float(t.max()), 2)}), flush=True)
    ratios = {"shape": tag, "k": k, "slices_at_W": S_of, "product_slices": slices_for(K, R, 512),
              "rows_whose_indices_differ_from_verify_topk": rows_off, "hist": last["identify"].hist.tolist(),
              "identify_over_verify_topk": round(med["identify"] / med["verify_topk"], 4),
              "identify_over_torch_topk": round(med["identify"] / med["torch_topk"], 4)}
    for W, S in S_of.items():
        ratios[f"S{S}_over_S1"] = round(med[f"identify_S{S}"] / med["identify_S1"], 4)
    if tag == "A":
        ratios["identify_S1_minus_verify_scores_us"] = round(med["identify_S1"] - med["verify_scores"], 2)
    print(json.dumps(ratios), flush=True)
    last.clear()
    del e, lab, models, cnt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--shapes", default="A,B,C")
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_identify.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    for tag in args.shapes.split(","):
        K, R, ks, chunk = SHAPES[tag]
        for k in ks:
            bench_shape(tag, K, R, k, chunk, args.rounds, args.step_timeout, dev)


if __name__ == "__main__":
    main()
