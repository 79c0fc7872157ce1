"""One sha256 per (implementation, shape, variant) over the bytes of loss | per | dE | dw | db, and one for the forward-only
call -- for comparing two builds of the library bit for bit on one GPU:

    GE2E_HIP_LIB=$PWD/speaker_embedding_ge2e_loss_amd/libge2e_hip_parent.so python tools/output_digest.py > a.txt
    python tools/output_digest.py > b.txt && diff a.txt b.txt

(tools/build_rev.sh builds the other revision's library.)  Inputs are seeded; a pair the library refuses prints SKIP.
Exit status 1 if one of the fp32 matrix-core implementations appears in no line.
"""
import hashlib
import os
import sys

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


def digest(o):
    h = hashlib.sha256()
    for name in ("loss", "per", "dE", "dw", "db"):
        t = getattr(o, name)
        h.update(name.encode() + b"|")
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    dev = torch.device("cuda:0")
    w, b = torch.tensor(7.5, device=dev), torch.tensor(-2.0, device=dev)
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
    missing = [i for i in IMPLS if i not in seen]
    if missing:
        print("no line for:", " ".join(missing))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
