"""One sha256 per line over the bytes of every output of a call on seeded inputs -- for comparing two builds of the library
bit for bit on one GPU:

    GE2E_HIP_LIB=$PWD/speaker_embedding_ge2e_loss_amd/libge2e_hip_parent.so python tools/output_digest.py > a.txt
    python tools/output_digest.py > b.txt && diff a.txt b.txt

(tools/build_rev.sh builds the other revision's library.)  Two sections:

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

Exit status 1 if one of the fp32 matrix-core implementations appears in no line.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ge2e_oracle as orc  # noqa: E402
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


def main():
    dev = torch.device("cuda:0")
    w, b = torch.tensor(7.5, device=dev), torch.tensor(-2.0, device=dev)
    missing = fused_section(dev, w, b)
    exact_section(dev, w, b)
    if missing:
        print("no line for:", " ".join(missing))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
