"""One sha256 per line over the bytes of every output of a call on seeded inputs -- for comparing two builds of the library
bit for bit on one GPU:

    GE2E_HIP_LIB=$PWD/speaker_embedding_ge2e_loss_amd/libge2e_hip_parent.so python tools/output_digest.py > a.txt
    python tools/output_digest.py > b.txt && diff a.txt b.txt

(tools/build_rev.sh builds the other revision's library.)  Seven sections:

  1. the fp32 matrix-core implementations: loss | per | dE | dw | db per (implementation, shape, variant), with and
     without the gradient.  A pair the library refuses prints SKIP.
  2. the exact kernels: impl="generic" and the float64 loss on dense shapes; the ragged loss, the labelled loss (plain,
     masked=True, wide=True) and the labelled evaluation (cos_sim_labeled with thresholds: cos | col | speakers | active |
     counts, the counts-only call, eer_counts_labeled) on row lists.  Both variants, with and without the gradient, per
     always.  The shapes are the smallest that reach every instantiation and edge of those kernels:
       D = 64, 128, 256, 260: the row kernels' 4, 8 and 16 register-resident steps and the plain loop; D = 37: scalar loads
       R = 200: four tiles of 64 positions, a last wave with 8 rows, two pieces of the GC contraction; R = 40: one of each
       67 and 65 speakers: a row of the cosine matrix is more than one pass of 16 and of 64 lanes and no multiple of 4
       (room for 12 beside it: the 16-byte stores of cos); a speaker of 68 rows that crosses a tile; one speaker
       alone (the other arm of contrast's N > 1)
       masked forms: ignored rows and lone speakers, and, of three batches, one without an active speaker
  3. the bank kernels, one line per call over every output: enroll_accumulate twice into one bank (sums | cnt after each;
     the second call leaves speakers untouched) and enroll_finalize; verify_scores without labels, with labels and
     thresholds, counts only, and both forms of the rows kernel through ge2e_selftest_verify_form; identify at k = 1, 5 and
     32 with and without labels; cohort_stats at two n_top with and without select; verify_scores_normed with labels and
     thresholds.  Banks of (K, D, R) as the tests have them:
       D = 36, 100, 256: the rows kernels' 4, 8 and 16 register-resident steps; D = 7 and 260: the plain loop
       K = 15, 16, 17, 67, 130: either side of the 16-model tile, of the group of 64 and of two groups; R = 1 .. 130: one
       wave with one row, a last wave with one row, three tiles
       speakers with 65, 64 and 1 rows in a call (the 64-index chunk of the speaker sum), speakers 4 mod 8 never enrolled
       (cnt = 0); labels with ignored rows (-1), a target that is not enrolled, and ids K and K + 5 past the bank
       cohorts of 2048, 2049 and 6145 at D = 36, R = 40: the three forms of the select kernel
  4. the index tables themselves, one line per call: label_index (offsets | order) and label_index_masked (offsets | order |
     speakers | active) at the smallest shapes that reach every path of the two kernels: B 1, N 67, R 300; B 3, N 1100,
     R 2200 (counters in the workspace, not in LDS); B 515, N 2, R 5 (past the grid); N 3, R 2500 with runs across 256-row
     chunks; and, masked only, a seeded draw at N 1100, R 300 with ignored rows, a lone and an absent speaker.  (The
     lone-speaker instantiation is reached by section 3's enroll_accumulate lines.)
  5. the tiled pipeline where section 1 does not reach (its shapes have sim, gc and ge on the 128 x 128 tile and the DMA-fed
     tile only inside simrows).  Every line prints the plan the library answers (ge2e_loss_plan, ge2e_cos_sim_plan).
     The five tiled PLAN_CASES of tests/bounds_cases.py, inputs made on the device from a seed as tests/test_gpu_plans.py
     makes them, loss | per | dE | dw | db with the gradient and forward only:
       (48, 257, 2, 288)  gc<C2>: the register-staged 256 x 256 tile (N M = 514 is no multiple of 32); sim<C3> walks 288 tiles
       (48, 272, 2, 264)  gc<C3>/1, 192 tiles     (65, 272, 2, 264)  gc<C3>/2, 520 tiles: a walk of more than one round
       (32, 528, 2, 264)  gc<C3>/4, 768 tiles     (25, 800, 3, 264)  gc<C3>/8, 1600 tiles; ge<C3> walks 500
     ge2e_cos_sim on its matrix-core route (prep, sim<C1>, tiled_cos) at (1, 16, 3, 64), (2, 65, 3, 128), (1, 300, 3, 768).
  6. the encoder through the C ABI, one line per buffer: the forward pack, the backward pack, ge2e_encode's out (normalised
     and raw), ge2e_encode_train's out | tape, ge2e_encode_bwd's d_flat | dZ [L][T][R][4H] | dY [R][D] -- the exact ranges:
     the workspace's round-to-64 gaps and unused slice partials are never written.  Shapes (R, T, n_mels, H, L, D):
       (33, 2, 40, 128, 2, 64)  both tile heights with pad rows     (17, 5, 20, 256, 4, 24)  H = 256, four layers
       (3, 2, 13, 128, 1, 37)   n_mels no multiple of 4: the scalar-load arm; D padding
       (73, 7, 12, 128, 1, 16)  one K-slice of the weight gradient  (33, 32, 12, 128, 1, 16)  three K-slices
       (33, 2, 40, 128, 2, 64) again through row_start: windows one frame apart, overlapping
  7. the audio front end through ``functional``, every call once with native=True and once with native=False, one line per
     call over its tensors and its Python lists (frame_start, out_lengths), seeded inputs:
       melspec at n_fft 512, hop 160, 40 mels, lengths [2500, 6500, 300] padded to [3200, 6500, 300], with a gain, both
       modes: 64 frames, four tiles, utterance boundaries inside tiles
       resample at (up, down) = (160, 441), (1, 3), (2, 1), banks audio.resample_bank(..., "kaiser_fast"), lengths
       [0, 5, 0, 0, 900, 0, 1]: empty utterances first, in a run and last but one; volume_gain on the resampled output,
       once with a layout and once with lengths
       vad_flags, vad_mask and trim_silences: a window of 480 at lengths [1000, 0, 479, 480, 961] with a gain; a window
       of 30 at [0, 4000, 0, 95, 0]; and that one again with voice_flags handed in
       MelFrontEnd.frames on waveforms of 0.3 s, 0.5 s and 0.31 s at 44100 Hz, source_rate=44100, normalize_volume,
       trim_silences, pad_to_partials

Exit status 1 if one of the fp32 matrix-core implementations appears in no line, or if the plan of a line of section 5 is
not the one its table claims.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bounds_cases as bc  # noqa: E402
import encoder_ref as enc  # noqa: E402
from oracle import ge2e_oracle as orc  # noqa: E402
from speaker_embedding_ge2e_loss_amd import _lib  # noqa: E402
from speaker_embedding_ge2e_loss_amd import functional as GF  # noqa: E402

IMPLS = ("fused_f32", "fused_split", "tiled", "team")
SHAPES = [                    # (B, N, M, D)
    (1, 6, 10, 256),          # fused: one tile, mostly pad rows
    (3, 64, 10, 256),         # fused: full tiles
    (2, 16, 8, 128),
    (1, 4, 16, 64),
    (2, 1, 4, 64),            # N = 1: the other arm of contrast's N > 1
    (3, 40, 2, 64),           # most speakers per tile: the speakers-per-tile caps
    (1, 65, 2, 33),           # D = 33: no matrix-core implementation takes it (SKIP lines)
    (1, 65, 2, 32),           # tiled rows<16>, 130 rows: a block with dead rows
    (2, 130, 3, 72),          # tiled rows<16>
    (1, 301, 3, 40),          # tiled rows<64>, 903 rows
    (1, 520, 2, 776),         # tiled rows<64>, three slot chunks
    (96, 129, 2, 32),         # tiled simrows, pad slots
    (96, 256, 2, 32),         # tiled simrows, every slot of the tile
]
# section 2, dense (generic and float64): more than 64 speakers with an odd D, a few, one, and D past the 16-wide tiles
EXACT_SHAPES = [(3, 67, 2, 37), (2, 6, 5, 64), (2, 1, 4, 64), (1, 20, 3, 260)]
# section 2, row lists: utterance counts per speaker (ids ascending); "big" has one speaker of 68 rows at positions 10 .. 77
COUNTS = {
    "big": [2] * 5 + [68] + [2] * 61,        # 67 speakers, R = 200
    "small": [2, 3, 9, 4, 2, 12, 8],         # 7 speakers, R = 40
    "one": [40],                             # 1 speaker, R = 40
}
BOUND = {"big": None, "small": 12, "one": None}  # num_speakers of the masked forms (None: the labels' distinct count)
ROW_CASES = [("big", 64), ("big", 128), ("big", 256), ("big", 260), ("big", 37), ("small", 64), ("small", 37), ("one", 64)]
B_ROWS = 3
THRESHOLDS = [0.02 * i - 0.2 for i in range(50)]
# section 3: (K, D, R, cohort size) -- the banks of tests/enroll_cases.py with the cohorts of tests/snorm_cases.py
BANK_CASES = [(1, 36, 1, 1), (15, 100, 16, 15), (16, 256, 17, 17), (17, 7, 63, 67), (67, 260, 64, 130), (130, 36, 65, 300),
              (130, 256, 130, 300), (16, 100, 130, 67)]
ENROLL_ROWS = ((65, 1, 2, 64, 0, 3, 0, 5), (0, 3, 0, 1, 0, 0, 2, 4))   # rows per speaker (id mod 8) in the two calls
SELECT_COHORTS = (2048, 2049, 6145)                                   # at D = 36, R = 40
N_TOPS = (5, 64)
# section 5: the five tiled PLAN_CASES of tests/bounds_cases.py (the atom a case is named for and every kernel PLAN_TILES
# counts more than 0 tiles for must be in the plan of its fwd+bwd line) ...
TILED_PLAN_CASES = [c for c in bc.PLAN_CASES if c[1] == "tiled"]
# ... and ge2e_cos_sim where its contraction runs on the matrix cores, with the plan the line must print
TILED_COS_CASES = [((1, 16, 3, 64), ["tiled_prep<10,1>", "tiled_sim<C1>", "tiled_cos"]),
                   ((2, 65, 3, 128), ["tiled_prep<10,1>", "tiled_sim<C1>", "tiled_cos"]),
                   ((1, 300, 3, 768), ["tiled_prep<10,3>", "tiled_sim<C1>", "tiled_cos"])]
# section 6: ((R, T, n_mels, H, L, D), windows through row_start)
ENCODER_CASES = [((33, 2, 40, 128, 2, 64), False), ((17, 5, 20, 256, 4, 24), False), ((3, 2, 13, 128, 1, 37), False),
                 ((73, 7, 12, 128, 1, 16), False), ((33, 32, 12, 128, 1, 16), False), ((33, 2, 40, 128, 2, 64), True)]


def digest(o, names=("loss", "per", "dE", "dw", "db")):
    h = hashlib.sha256()
    for name in names:
        t = getattr(o, name)
        h.update(name.encode() + b"|")
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def fused_section(dev, w, b):
    seen = set()
    for shape in SHAPES:
        e = torch.as_tensor(orc.synth_embeddings(shape, "raw", seed=sum(shape)), device=dev)
        for variant in ("softmax", "contrast"):
            for impl in IMPLS:
                tag = f"{impl} {shape} {variant}"
                try:
                    GF.resolve_impl(*shape, variant, impl)
                except RuntimeError:
                    print(tag, "SKIP")
                    continue
                for grad in (True, False):
                    o = GF.loss_fwd_bwd(e, w, b, variant=variant, impl=impl, need_grad=grad, need_per=True)
                    torch.cuda.synchronize()
                    print(tag, "fwd+bwd" if grad else "fwd", digest(o))
                seen.add(impl)
    return [i for i in IMPLS if i not in seen]


def masked_labels(kind, rng):
    """(B_ROWS, R) labels for the masked forms, rows in a seeded random order.  Batch 0: the counts of `kind` with the last
    speakers' rows given away -- two ignored rows (-1) and two lone speakers; batch 1: the same counts in another order, no
    row ignored; batch 2: no active speaker (three lone labels, the rest negative)."""
    counts = COUNTS[kind]
    ids = np.repeat(np.arange(len(counts)), counts)
    R = len(ids)
    first = ids.copy()
    if len(counts) > 1:
        first[-4:] = [-1, -1, len(counts) + 5, len(counts) + 9]
    else:
        first[-3:] = [-1, 7, 9]
    none = np.full(R, -1)
    none[:3] = [4, 0, 2]
    return np.stack([rng.permutation(first), rng.permutation(ids), none]).astype(np.int64)


def each_call(tag, call, names=("loss", "per", "dE", "dw", "db")):
    for variant in ("softmax", "contrast"):
        for grad in (True, False):
            o = call(variant, grad)
            torch.cuda.synchronize()
            print(tag, variant, "fwd+bwd" if grad else "fwd", digest(o, names))


def exact_section(dev, w, b):
    w64, b64 = w.double(), b.double()
    for shape in EXACT_SHAPES:
        x = orc.synth_embeddings(shape, "raw", seed=sum(shape) + 1)
        e = torch.as_tensor(x, device=dev)
        e64 = torch.as_tensor(x.astype(np.float64), device=dev)
        each_call(f"generic {shape}", lambda v, g: GF.loss_fwd_bwd(e, w, b, variant=v, impl="generic", need_grad=g, need_per=True))
        each_call(f"f64 {shape}", lambda v, g: GF.loss_fwd_bwd(e64, w64, b64, variant=v, need_grad=g, need_per=True))
    active = ("loss", "per", "dE", "dw", "db", "active")
    for kind, D in ROW_CASES:
        counts = COUNTS[kind]
        R = sum(counts)
        rng = np.random.default_rng(1000 * R + 10 * D + len(counts))
        e = torch.as_tensor(orc.synth_embeddings((B_ROWS, R, 1, D), "raw", seed=R + D).reshape(B_ROWS, R, D), device=dev)
        ids = np.repeat(np.arange(len(counts)), counts)
        plain = np.stack([rng.permutation(ids) for _ in range(B_ROWS)]).astype(np.int64)   # every speaker has >= 2 rows
        masked, bound = masked_labels(kind, rng), BOUND[kind]
        tag = f"{kind} R={R} D={D}"
        each_call(f"ragged {tag}", lambda v, g: GF.loss_fwd_bwd_ragged(e, counts, w, b, variant=v, need_grad=g, need_per=True))
        each_call(f"labeled {tag}", lambda v, g: GF.loss_fwd_bwd_labeled(e, plain, w, b, variant=v, need_grad=g, need_per=True))
        each_call(f"labeled_masked {tag}", lambda v, g: GF.loss_fwd_bwd_labeled(
            e, masked, w, b, num_speakers=bound, variant=v, need_grad=g, need_per=True, masked=True), active)
        each_call(f"labeled_wide {tag}", lambda v, g: GF.loss_fwd_bwd_labeled(
            e, masked, w, b, num_speakers=bound, variant=v, need_grad=g, need_per=True, wide=True), active)
        o = GF.cos_sim_labeled(e, masked, num_speakers=bound, thresholds=THRESHOLDS)
        torch.cuda.synchronize()
        print(f"cos_sim_labeled {tag}", digest(o, ("cos", "col", "speakers", "active", "counts")))
        c = GF.cos_sim_labeled(e, masked, num_speakers=bound, thresholds=THRESHOLDS, need_cos=False)
        n = GF.eer_counts_labeled(7.5 * o.cos - 2.0, o.col, o.active, THRESHOLDS)
        torch.cuda.synchronize()
        print(f"cos_sim_labeled counts only {tag}", digest(c, ("col", "speakers", "active", "counts")))
        print(f"eer_counts_labeled {tag}", hashlib.sha256(n.cpu().contiguous().numpy().tobytes()).hexdigest())


def line(tag, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"|")
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(tag, h.hexdigest())


def unit_rows(rng, centre, cls, dev):
    x = centre[cls] + 0.5 * rng.standard_normal((len(cls), centre.shape[1]))
    return torch.as_tensor((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), device=dev)


def make_cohort(rng, C, D, dev):
    """Unit models; member iff c % 8 != 4 (cnt 1 .. 3, else 0 or -1)."""
    c = np.arange(C)
    ccnt = np.where(c % 8 != 4, 1 + c % 3, -(c % 2)).astype(np.int32)
    return unit_rows(rng, rng.standard_normal((C, D)), c, dev), torch.as_tensor(ccnt, device=dev)


def cohort_lines(tag, rows, select, cohort, ccnt):
    for n_top in N_TOPS:
        line(f"{tag} n_top={n_top}", GF.cohort_stats(rows, cohort, ccnt, n_top=n_top))
        line(f"{tag} n_top={n_top} select", GF.cohort_stats(rows, cohort, ccnt, n_top=n_top, select=select, select_min=0))


def bank_section(dev):
    lib = _lib.load()
    thr = torch.as_tensor(THRESHOLDS, dtype=torch.float64).to(torch.float32).to(dev)
    T = thr.numel()
    for K, D, R, C in BANK_CASES:
        tag = f"K={K} D={D} R={R}"
        rng = np.random.default_rng(100000 * K + 1000 * D + R)
        centre = rng.standard_normal((K + 1, D))
        sums, cnt = torch.zeros(K, D, device=dev), torch.zeros(K, dtype=torch.int32, device=dev)
        for i, pattern in enumerate(ENROLL_ROWS):
            lab = np.concatenate([np.repeat(np.arange(K), [pattern[s % 8] for s in range(K)]), [-1, K, K + 5]])
            lab = lab[rng.permutation(len(lab))]
            e = unit_rows(rng, centre, np.clip(lab, 0, K), dev)
            GF.enroll_accumulate(sums, cnt, e, torch.as_tensor(lab.astype(np.int32), device=dev))
            line(f"enroll_accumulate {i + 1} {tag}", sums, cnt)
        models = GF.enroll_finalize(sums, cnt)
        line(f"enroll_finalize {tag}", models)
        # the trials: enrolled speakers in turn; rows 1 and (from 17 rows on) R - 1 ignored, row 3 the id K + 5, row 5 the
        # id K, row 6 a speaker that is not enrolled
        n = cnt.cpu().numpy()
        enrolled, absent = np.flatnonzero(n > 0), np.flatnonzero(n <= 0)
        lab = enrolled[np.arange(R) % len(enrolled)]
        for pos, v in ((1, -1), (3, K + 5), (5, K), (6, int(absent[0]) if len(absent) else K + 5)) + (((R - 1, -1),) if R >= 17 else ()):
            if pos < R:
                lab[pos] = v
        e = unit_rows(rng, centre, np.clip(lab, 0, K), dev)
        lab = torch.as_tensor(lab.astype(np.int32), device=dev)
        line(f"verify_scores {tag}", GF.verify_scores(e, models, cnt).scores)
        o = GF.verify_scores(e, models, cnt, labels=lab, thresholds=thr)
        line(f"verify_scores labels {tag}", o.scores, o.counts, o.trials)
        o = GF.verify_scores(e, models, cnt, labels=lab, thresholds=thr, need_scores=False)
        line(f"verify_scores counts only {tag}", o.counts, o.trials)
        for form, name in ((1, "staged"), (2, "streamed")):
            scores = torch.empty(R, K, device=dev)
            counts, trials = torch.empty(T, 2, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.ge2e_selftest_verify_form(
                    e.data_ptr(), lab.data_ptr(), models.data_ptr(), cnt.data_ptr(), K, R, D, GF.EPS_COS, GF.SMALL_ERR,
                    thr.data_ptr(), T, scores.data_ptr(), counts.data_ptr(), trials.data_ptr(),
                    torch.cuda.current_stream(dev).cuda_stream, form), "ge2e_selftest_verify_form")
            line(f"verify_form {name} {tag}", scores, counts, trials)
        for k in (1, 5, 32):
            o = GF.identify(e, models, cnt, k=k)
            line(f"identify k={k} {tag}", o.indices, o.scores)
            o = GF.identify(e, models, cnt, k=k, labels=lab)
            line(f"identify k={k} labels {tag}", o.indices, o.scores, o.rank, o.hist)
        cohort, ccnt = make_cohort(rng, C, D, dev)
        cohort_lines(f"cohort_stats C={C} {tag}", e, lab, cohort, ccnt)
        rs = GF.cohort_stats(e, cohort, ccnt, n_top=N_TOPS[0], select=lab, select_min=0)
        ms = GF.cohort_stats(models, cohort, ccnt, n_top=N_TOPS[0], select=cnt, select_min=1)
        o = GF.verify_scores_normed(e, models, cnt, rs, ms, labels=lab, thresholds=thr)
        line(f"verify_scores_normed C={C} {tag}", ms, o.scores, o.counts, o.trials)
    D, R = 36, 40
    for C in SELECT_COHORTS:
        rng = np.random.default_rng(C)
        cohort, ccnt = make_cohort(rng, C, D, dev)
        e = unit_rows(rng, rng.standard_normal((1, D)), np.zeros(R, dtype=np.int64), dev)
        select = torch.as_tensor((np.arange(R) % 7 - 1).astype(np.int32), device=dev)    # every seventh row is not scored
        cohort_lines(f"cohort_stats C={C} D={D} R={R}", e, select, cohort, ccnt)


def index_cases():
    """name -> (N, labels (B, R)): the shapes of the index tests (tests/test_gpu_labeled.py), every label inside [0, N)."""
    rng = np.random.default_rng(11)
    runs = np.concatenate([np.zeros(700), np.arange(900) % 3, np.full(300, 2), rng.integers(0, 3, 350), np.ones(250)])
    return {
        "B=1 N=67 R=300": (67, rng.integers(0, 67, (1, 300))),
        "B=3 N=1100 R=2200": (1100, np.stack([rng.permutation(np.repeat(np.arange(1100), 2)) for _ in range(3)])),
        "B=515 N=2 R=5": (2, rng.integers(0, 2, (515, 5))),
        "B=1 N=3 R=2500 runs": (3, runs[None]),
    }


def index_section(dev):
    for tag, (N, labels) in index_cases().items():
        lab = torch.as_tensor(labels.astype(np.int32), device=dev)
        line(f"label_index {tag}", *GF.label_index(lab, N))
        line(f"label_index_masked {tag}", *GF.label_index_masked(lab, N))
    # the masked form alone: ignored rows (negative, N and past it), a lone and an absent speaker among seeded draws
    N, R = 1100, 300
    rng = np.random.default_rng(N + R)
    labels = rng.integers(0, 120, (2, R))                # about 2.5 rows a speaker: lone ones and absent ones among them
    labels[:, ::17] = -1
    labels[0, 5], labels[0, 6], labels[1, 7] = N, N + 5, -2147483648
    labels[0, 100:103] = [N - 1, N - 1, 700]             # the last speaker active, 700 alone, 701 .. 1098 absent
    line(f"label_index_masked B=2 N={N} R={R} draw", *GF.label_index_masked(torch.as_tensor(labels.astype(np.int32), device=dev), N))


def tiled_section(dev, w, b):
    """Returns the lines whose plan, asked of the library under test, lacks an atom the tables claim for them."""
    wrong = []
    for case in TILED_PLAN_CASES:
        atom, impl, B, N, M, D, variant, _ = case
        g = torch.Generator(device=dev).manual_seed(B + N + M + D)
        e = torch.nn.functional.normalize(torch.randn(B, N, M, D, generator=g, device=dev), dim=-1)
        for grad in (True, False):
            plan = _lib.loss_plan(B, N, M, D, variant, impl, grad)
            tag = f"tiled plan {(B, N, M, D)} {variant} {'fwd+bwd' if grad else 'fwd'} [{' '.join(plan)}]"
            walked = [k for k, n in bc.PLAN_TILES[atom].items() if n > 0]
            if grad and not all(any(a.startswith(k) for a in plan) for k in [atom] + walked):
                wrong.append(tag)
            o = GF.loss_fwd_bwd(e, w, b, variant=variant, impl=impl, need_grad=grad, need_per=True)
            torch.cuda.synchronize()
            print(tag, digest(o))
        del e, o
    for shape, atoms in TILED_COS_CASES:
        plan = _lib.cos_sim_plan(*shape)
        tag = f"tiled cos_sim {shape} [{' '.join(plan)}]"
        if plan != atoms:
            wrong.append(tag)
        e = torch.as_tensor(orc.synth_embeddings(shape, "raw", seed=sum(shape)), device=dev)
        with torch.no_grad():
            line(tag, GF.cos_sim(e))
    return wrong


def encoder_section(dev):
    lib = _lib.load()
    for shape, windows in ENCODER_CASES:
        R, T, n_mels, H, L, D = shape
        tag = f"encoder {shape}" + (" row_start" if windows else "")
        rng = np.random.default_rng(sum(shape) + windows)
        flat = torch.as_tensor(enc.flat(enc.random_params(n_mels, H, L, D, seed=sum(shape))), device=dev)
        frames = R + T - 1 if windows else R * T                  # windows: row r starts at frame r
        mel = torch.as_tensor(rng.uniform(0.0, 0.96, (frames, n_mels)).astype(np.float32), device=dev)
        rs = torch.arange(R, dtype=torch.int64, device=dev) if windows else None
        rs_ptr = rs.data_ptr() if windows else None
        g = torch.as_tensor(rng.standard_normal((R, D)).astype(np.float32), device=dev)

        def floats(nbytes):
            return torch.full((nbytes // 4,), float("nan"), device=dev)
        packed = floats(lib.ge2e_encoder_packed_bytes(n_mels, H, L, D))
        packed_bwd = floats(lib.ge2e_encoder_packed_bwd_bytes(n_mels, H, L, D))
        tape, ws = floats(lib.ge2e_encode_train_tape_bytes(*shape)), floats(lib.ge2e_encode_bwd_workspace_bytes(*shape))
        out, d_flat = floats(4 * R * D), floats(4 * flat.numel())
        with torch.cuda.device(dev):
            _lib.check(lib.ge2e_encoder_pack(flat.data_ptr(), n_mels, H, L, D, packed.data_ptr(), None), "ge2e_encoder_pack")
            line(f"{tag} pack", packed)
            _lib.check(lib.ge2e_encoder_pack_bwd(flat.data_ptr(), n_mels, H, L, D, packed_bwd.data_ptr(), None), "ge2e_encoder_pack_bwd")
            line(f"{tag} pack_bwd", packed_bwd)
            for normalize in (1, 0):
                _lib.check(lib.ge2e_encode(packed.data_ptr(), mel.data_ptr(), rs_ptr, R, T, n_mels, H, L, D, normalize,
                                           out.data_ptr(), None), "ge2e_encode")
                line(f"{tag} encode {'normalised' if normalize else 'raw'}", out)
            _lib.check(lib.ge2e_encode_train(packed.data_ptr(), mel.data_ptr(), rs_ptr, R, T, n_mels, H, L, D, 1, out.data_ptr(),
                                             tape.data_ptr(), None), "ge2e_encode_train")
            line(f"{tag} encode_train", out, tape)
            _lib.check(lib.ge2e_encode_bwd(packed_bwd.data_ptr(), mel.data_ptr(), rs_ptr, R, T, n_mels, H, L, D, 1, tape.data_ptr(),
                                           g.data_ptr(), d_flat.data_ptr(), ws.data_ptr(), None), "ge2e_encode_bwd")
            n_dz = L * T * R * 4 * H
            dy = (n_dz + 63) // 64 * 64                           # offsets in the workspace are rounded up to 64 floats
            line(f"{tag} encode_bwd", d_flat, ws[:n_dz], ws[dy:dy + R * D])


RESAMPLE_RATIOS = [(160, 441), (1, 3), (2, 1)]
RESAMPLE_LENGTHS = [0, 5, 0, 0, 900, 0, 1]
VAD_CASES = [(480, [1000, 0, 479, 480, 961], [1.0, 2.0, 0.5, 0.25, 1.5]), (30, [0, 4000, 0, 95, 0], None)]
VAD_DETECTOR = dict(floor_span=5, ratio_db=3.0, min_level_dbfs=-50.0)
VAD_MASK = dict(avg_width=3, max_silence=2)


def bursts(n, seed, period, dev):
    """Noise that is loud (0.1) for `period` samples and quiet (0.0003) for the next, and so on."""
    x = np.random.default_rng(seed).standard_normal(n) * np.where((np.arange(n) // period) % 2 == 0, 0.1, 0.0003)
    return torch.as_tensor(x.astype(np.float32), device=dev)


def audio_section(dev):
    from speaker_embedding_ge2e_loss_amd import audio

    def both(tag, call):
        for native in (True, False):
            out = call(native)
            out = out if isinstance(out, tuple) else (out,)
            line(f"{tag} native={native}", *[t if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=torch.int64) for t in out])

    lengths, padded = [2500, 6500, 300], [3200, 6500, 300]
    tables = GF.melspec_pack(audio.hann_window(512).to(dev), audio.mel_filterbank(16000, 512, 40).to(dev))
    line("melspec_pack 512 40", tables.packed)
    wav, gain = bursts(sum(lengths), 1, 800, dev), torch.tensor([1.0, 0.5, 2.0], device=dev)
    for mode in ("db", "linear"):
        both(f"melspec {mode}", lambda native: GF.melspec(tables, wav, lengths, hop=160, padded_lengths=padded, gain=gain,
                                                         mode=mode, native=native))
    wav = bursts(sum(RESAMPLE_LENGTHS), 2, 100, dev)
    for up, down in RESAMPLE_RATIOS:
        bank = audio.resample_bank(down, up, "kaiser_fast")
        t = GF.resample_pack(bank.taps.to(dev), bank.up, bank.down, bank.lead)
        line(f"resample_pack {up}/{down}", t.packed)
        both(f"resample {up}/{down}", lambda native: GF.resample(t, wav, RESAMPLE_LENGTHS, native=native))
        out, out_lengths = GF.resample(t, wav, RESAMPLE_LENGTHS)
        lay = GF.resample_layout(out_lengths, 1, 1, device=dev)
        both(f"volume_gain {up}/{down} layout", lambda native: GF.volume_gain(out, out_lengths, native=native, layout=lay))
        both(f"volume_gain {up}/{down} lengths", lambda native: GF.volume_gain(out, out_lengths, native=native))
    for S, ls, gains in VAD_CASES:
        wav = bursts(sum(ls), S, 3 * S, dev)
        g = None if gains is None else torch.tensor(gains, device=dev)
        lay = GF.vad_layout(ls, S, device=dev)
        both(f"vad_flags {S}", lambda native: GF.vad_flags(wav, ls, g, window=S, native=native, **VAD_DETECTOR))
        flags = GF.vad_flags(wav, ls, g, window=S, **VAD_DETECTOR)
        both(f"vad_mask {S}", lambda native: GF.vad_mask(flags, lay, native=native, **VAD_MASK))
        both(f"trim_silences {S}", lambda native: GF.trim_silences(wav, ls, gain=g, window=S, native=native, **VAD_DETECTOR,
                                                                    **VAD_MASK))
    handed = (np.random.default_rng(7).random(lay.total_windows) < 0.4).astype(np.uint8)
    both(f"trim_silences {S} voice_flags", lambda native: GF.trim_silences(wav, ls, voice_flags=handed, window=S, native=native,
                                                                           **VAD_MASK))
    fe = audio.MelFrontEnd()
    wavs = [bursts(int(sec * 44100), 10 + i, 4410, dev) for i, sec in enumerate((0.3, 0.5, 0.31))]
    both("MelFrontEnd.frames", lambda native: fe.frames(wavs, normalize_volume=True, pad_to_partials=True, native=native,
                                                        source_rate=44100, trim_silences=True))


def main():
    dev = torch.device("cuda:0")
    w, b = torch.tensor(7.5, device=dev), torch.tensor(-2.0, device=dev)
    missing = fused_section(dev, w, b)
    exact_section(dev, w, b)
    bank_section(dev)
    index_section(dev)
    wrong = tiled_section(dev, w, b)
    encoder_section(dev)
    audio_section(dev)
    if missing:
        print("no line for:", " ".join(missing))
    for tag in wrong:
        print("plan is not the one claimed:", tag)
    return 1 if missing or wrong else 0


if __name__ == "__main__":
    sys.exit(main())
