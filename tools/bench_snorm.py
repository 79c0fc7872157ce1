"""What adaptive score normalisation against a cohort (ge2e_cohort_stats + ge2e_verify_scores_normed) costs on one GPU,
against the route a caller had before: all of it in torch.  K = 1 251 enrolled models, R = 16 384 trial rows, D = 256, a
cohort of C = 5 994 speakers, n_top = 300, 50 thresholds spread over the normalised scores' range; unit models, unit
trial rows model + 0.5 noise, as tools/bench_enroll_verify.py makes them.

EXPECTATION, written before anything was measured: the fused route beats the torch route, because it writes neither the
[R][K] matrix nor the two boolean temporaries of every threshold's compare-and-sum, and holds [R][C] a chunk at a time.
What was measured stands in profiles/snorm_bench.txt and DESIGN.md 3.4j, whichever way it fell.

Points, all bare enqueues on the current stream:
  stats_rows          functional.cohort_stats on the trial rows (select = labels, 0): the product's chunk
  stats_models        functional.cohort_stats on the bank's models (select = cnt, 1)
  normed_counts       functional.verify_scores_normed(need_scores=False): counts and trials only
  normed_scores       the same with the [R][K] matrix written as well
  bank_verify         SpeakerBank.verify(normalize=True, need_scores=False): the trial rows' statistics and the normed
                      call; the model-side statistics are cached by the bank after the first call
  bank_verify_scores  the same with need_scores=True (the default)
  stats_rows_<m>MiB   ge2e_selftest_cohort_stats_chunk with the chunk that m = 8, 32, 128 MiB of keys give
  verify_counts       functional.verify_scores(need_scores=False): the raw call, what normalising adds to
  torch               two products against the cohort, two topk(300), mean / std, the broadcast normalisation of the
                      [R][K] product, and per threshold a compare, two masks and two sums
Every chunk must return the product call's bits (asserted); the torch route's counts are compared with the fused ones and
the number of (threshold, column) entries that differ is reported (other summation orders: scores next to a threshold
fall either way).  All in one process, the points taken in turn round after round, each call between its own pair of HIP
events on an idle queue after 10 warm-up rounds; median / min / max per point.  Every warm-up and every timed round runs
under a watchdog (--step-timeout seconds) that ends the process.  One JSON line per point and one of ratios on stdout.

usage: python tools/bench_snorm.py [--rounds 100] [--step-timeout 120]
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
from speaker_embedding_ge2e_loss_amd import evaluation as EV  # noqa: E402
from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

K, R, D, C, N_TOP, T = 1251, 16384, 256, 5994, 300, 50
EPS, EPS_COS, EPS_STD = GF.SMALL_ERR, GF.EPS_COS, GF.EPS_STD
CHUNKS_MIB = (8, 32, 128)


def chunk_rows(mib):
    return max((mib << 20) // (4 * C) // 64 * 64, 64)


def make(dev):
    g = torch.Generator(device=dev).manual_seed(K + R + C)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1).contiguous()    # noqa: E731
    models = unit(torch.randn(K, D, generator=g, device=dev))
    cohort = unit(torch.randn(C, D, generator=g, device=dev))
    lab = torch.randint(0, K, (R,), generator=g, device=dev)
    e = unit(models[lab] + 0.5 * unit(torch.randn(R, D, generator=g, device=dev)))
    return e, lab.to(torch.int32), models, cohort


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("--rounds must be at least 50 (the median of fewer is not a measurement)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_snorm.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    e, lab, models, cohort = make(dev)
    # banks whose models are the rows above: one row enrols a speaker, and the unit centroid of a unit row is that row
    bank, coh = EV.SpeakerBank(K, D, dev), EV.SpeakerBank(C, D, dev)
    bank.enroll(models, torch.arange(K, device=dev))
    coh.enroll(cohort, torch.arange(C, device=dev))
    bank.set_cohort(coh, n_top=N_TOP, eps_std=EPS_STD)
    bm, cm, cnt, ccnt = bank.models(), coh.models(), bank.cnt, coh.cnt
    ms = GF.cohort_stats(bm, cm, ccnt, n_top=N_TOP, select=cnt, select_min=1)
    rs = GF.cohort_stats(e, cm, ccnt, n_top=N_TOP, select=lab, select_min=0)
    normed = GF.verify_scores_normed(e, bm, cnt, rs, ms, labels=lab).scores
    q = torch.quantile(normed.flatten()[::37].float(), torch.tensor([0.001, 0.999], device=dev))
    thr = torch.linspace(float(q[0]), float(q[1]), T, device=dev)
    raw_thr = torch.linspace(0.0, 1.0, T, device=dev)
    del normed
    last = {}
    stats_out = torch.empty(R, 2, device=dev)

    def stats_rows():
        last["stats_rows"] = GF.cohort_stats(e, cm, ccnt, n_top=N_TOP, select=lab, select_min=0)

    def stats_models():
        last["stats_models"] = GF.cohort_stats(bm, cm, ccnt, n_top=N_TOP, select=cnt, select_min=1)

    def normed_counts():
        last["normed_counts"] = GF.verify_scores_normed(e, bm, cnt, rs, ms, labels=lab, thresholds=thr, need_scores=False)

    def normed_scores():
        last["normed_scores"] = GF.verify_scores_normed(e, bm, cnt, rs, ms, labels=lab, thresholds=thr)

    def bank_verify():
        last["bank_verify"] = bank.verify(e, lab, thresholds=thr, need_scores=False, normalize=True)

    def bank_verify_scores():
        last["bank_verify_scores"] = bank.verify(e, lab, thresholds=thr, normalize=True)

    def verify_counts():
        last["verify_counts"] = GF.verify_scores(e, bm, cnt, labels=lab, thresholds=raw_thr, need_scores=False)

    def forced(mib):
        rows = chunk_rows(mib)
        nbytes = int(lib.ge2e_selftest_cohort_stats_workspace_bytes(C, R, D, N_TOP, rows))
        ws = GF.alloc_workspace(nbytes, dev, init=False)
        name = f"stats_rows_{mib}MiB"

        def run():
            _lib.check(lib.ge2e_selftest_cohort_stats_chunk(e.data_ptr(), lab.data_ptr(), 0, cm.data_ptr(), ccnt.data_ptr(), C, R, D,
                                                            N_TOP, EPS_COS, EPS, EPS_STD, stats_out.data_ptr(), ws.data_ptr(),
                                                            nbytes, None, rows), name)
            last[name] = stats_out
        return name, run

    own = torch.zeros(R, K, dtype=torch.bool, device=dev)
    own[torch.arange(R, device=dev), lab.long()] = True

    def torch_route():
        en = torch.nn.functional.normalize(e, dim=-1, eps=EPS_COS)
        s = en @ bm.t() + EPS                                        # [R][K]
        te = torch.topk(en @ cm.t() + EPS, N_TOP, dim=1).values      # [R][C] -> [R][300]
        tm = torch.topk(bm @ cm.t() + EPS, N_TOP, dim=1).values      # [K][C] -> [K][300]
        mu_e, sd_e = te.mean(1), te.std(1, unbiased=False).clamp_min(EPS_STD)
        mu_m, sd_m = tm.mean(1), tm.std(1, unbiased=False).clamp_min(EPS_STD)
        z = 0.5 * ((s - mu_m[None, :]) / sd_m[None, :] + (s - mu_e[:, None]) / sd_e[:, None])
        counts = torch.empty(T, 2, dtype=torch.int64, device=dev)
        for t in range(T):
            acc = z > thr[t]
            counts[t, 0] = (acc & ~own).sum()
            counts[t, 1] = (acc & own).sum()
        last["torch"] = counts

    points = [("stats_rows", stats_rows), ("stats_models", stats_models), ("normed_counts", normed_counts),
              ("normed_scores", normed_scores), ("bank_verify", bank_verify), ("bank_verify_scores", bank_verify_scores)]
    points += [forced(m) for m in CHUNKS_MIB]
    points += [("verify_counts", verify_counts), ("torch", torch_route)]
    for name, fn in points:
        faulthandler.dump_traceback_later(args.step_timeout, exit=True)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        if name.startswith("stats_rows_"):                         # every chunk: the product call's bits
            assert torch.equal(last[name].view(torch.int32), last["stats_rows"].view(torch.int32)), f"{name} differs"
    assert torch.equal(last["bank_verify"].counts, last["normed_counts"].counts)
    differ = int((last["torch"] != last["normed_counts"].counts.long()).sum())
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
        print(json.dumps({"point": name, "K": K, "R": R, "D": D, "C": C, "n_top": N_TOP, "T": T, "rounds": args.rounds,
                          "call_us_median": round(med[name], 2), "call_us_min": round(float(t.min()), 2),
                          "call_us_max": round(float(t.max()), 2)}), flush=True)
    ratios = {"chunk_rows": {f"{m}MiB": chunk_rows(m) for m in CHUNKS_MIB},
              "count_entries_that_differ_from_torch": differ, "of": 2 * T,
              "trials": last["normed_counts"].trials.tolist(),
              "bank_verify_over_torch": round(med["bank_verify"] / med["torch"], 4),
              "torch_over_bank_verify": round(med["torch"] / med["bank_verify"], 2),
              "normed_counts_over_verify_counts": round(med["normed_counts"] / med["verify_counts"], 4)}
    for m in CHUNKS_MIB:
        ratios[f"chunk_{m}MiB_over_32MiB"] = round(med[f"stats_rows_{m}MiB"] / med["stats_rows_32MiB"], 4)
    print(json.dumps(ratios), flush=True)


if __name__ == "__main__":
    main()
