"""Case tables of tests/test_gpu_bounds.py and tests/test_gpu_plans.py (a plain module: tests/test_bounds_cases.py and
tests/test_plan_cases.py check it without a GPU).

Every shape sits on a padding edge of the kernel it names.  The edges are those the library reports (ge2e_resolve_impl,
ge2e_raw_supported); test_bounds_cases.py scans those predicates and fails if a table misses one, so nothing here is
taken on trust.  Inputs and (w, b) are those of test_gpu_parity.test_ragged_shapes ("raw" rows, w = 7.5, b = -2).
B*N*M*D <= 6e6 keeps the fp64 closed form quick (the bound of test_gpu_fuzz.py).
"""
import functools

import numpy as np

from oracle import ge2e_oracle as orc

W, BIAS = 7.5, -2.0
MAX_ELEMS = 6e6
S, C = "softmax", "contrast"

# (impl, B, N, M, D, variant)
LOSS_CASES = [
    # generic: any shape.  D % 4 != 0 (rows of E not 16-byte aligned), N = 1, M = 2, N = 65 (more speakers than a wave)
    ("generic", 2, 1, 2, 1, S), ("generic", 1, 2, 2, 7, S), ("generic", 3, 5, 3, 7, C), ("generic", 1, 65, 2, 33, S),
    ("generic", 1, 65, 2, 33, C), ("generic", 2, 7, 4, 65, C), ("generic", 1, 1, 9, 33, S), ("generic", 2, 4, 5, 64, S),
    # fused_f32: N 1..64, M 2..64, D a multiple of 64 up to 256 (it takes none of 4, 36, 100, 200, 252); B = 300 > its grid
    ("fused_f32", 3, 1, 2, 64, S), ("fused_f32", 2, 64, 2, 256, C), ("fused_f32", 1, 64, 64, 64, S),
    ("fused_f32", 2, 1, 64, 128, S), ("fused_f32", 300, 2, 3, 64, C), ("fused_f32", 1, 64, 64, 256, C),
    ("fused_f32", 2, 33, 9, 192, C),
    # fused_split: the same N and M, D any multiple of 4 (padded to 64 inside the load / store stages)
    ("fused_split", 3, 1, 2, 4, S), ("fused_split", 2, 64, 2, 36, C), ("fused_split", 1, 64, 64, 100, S),
    ("fused_split", 2, 1, 64, 200, S), ("fused_split", 300, 2, 3, 252, C), ("fused_split", 1, 64, 64, 256, C),
    ("fused_split", 2, 33, 9, 200, S),
    # team: eight members share N speakers unevenly; (N + 7) / 8 * M = 80 is its largest image; B over and under the teams
    ("team", 1, 16, 16, 4, S), ("team", 2, 23, 7, 80, C), ("team", 9, 40, 16, 132, S), ("team", 70, 57, 5, 200, C),
    ("team", 1, 64, 10, 252, S), ("team", 9, 64, 10, 256, C), ("team", 2, 64, 10, 256, S), ("team", 70, 16, 2, 256, S),
    ("team", 1, 57, 10, 200, C),
    # tiled: npad = 64 ceil(N / 64) no multiple of N; N M no multiple of 64, 128, 256 (one with: 256); M > 64; D % 32 either way
    ("tiled", 3, 1, 2, 8, S), ("tiled", 1, 15, 70, 72, C), ("tiled", 3, 65, 3, 200, S), ("tiled", 1, 130, 5, 264, C),
    ("tiled", 1, 300, 3, 776, S), ("tiled", 1, 65, 7, 1024, C), ("tiled", 3, 130, 4, 1024, S), ("tiled", 1, 64, 4, 264, S),
    ("tiled", 3, 15, 3, 72, C),
    # ... and launches big enough for its 256-row tiles (>= 192 of them): similarity + row pass in one kernel (N = 256 has an
    # instantiation of its own), the 256 x 256 similarity and dE contractions fed by registers (D or N % 32 != 0) and by LDS-DMA.
    # Limits: the 256 x 256 centroid-gradient contraction (and its row split) needs >= 192 tiles with N, D >= 256, which does
    # not fit in MAX_ELEMS, so it never runs here (PLAN_CASES below has it); of the large launches only the fused similarity + row pass runs as contrast
    # (tens of thousands of contrast rows tie on most draws: SEEDS names draws that do not).
    ("tiled", 64, 130, 4, 32, S), ("tiled", 64, 256, 3, 32, S), ("tiled", 32, 257, 2, 8, S), ("tiled", 32, 257, 2, 32, S),
    ("tiled", 32, 130, 4, 264, S), ("tiled", 32, 128, 5, 264, S), ("tiled", 64, 130, 4, 32, C), ("tiled", 64, 256, 3, 32, C),
    # wave: every instantiated M at its largest register-only N and at its largest N; B = 2100 > the grid's 2048 waves
    ("wave", 5, 6, 2, 256, S), ("wave", 1, 12, 2, 4, C), ("wave", 2100, 5, 3, 36, S), ("wave", 5, 10, 3, 252, C),
    ("wave", 1, 4, 4, 256, S), ("wave", 5, 10, 4, 36, C), ("wave", 2100, 4, 5, 36, S), ("wave", 1, 8, 5, 256, C),
    ("wave", 5, 3, 6, 4, C), ("wave", 2100, 8, 6, 4, S), ("wave", 1, 3, 8, 252, S), ("wave", 5, 8, 8, 256, C),
    ("wave", 5, 2, 10, 256, S), ("wave", 1, 6, 10, 252, C), ("wave", 2100, 2, 16, 4, S), ("wave", 5, 3, 16, 36, C),
    ("wave", 2100, 2, 2, 256, S),
    # auto / auto_no_team: one case per implementation they resolve to
    ("auto", 1, 4, 5, 256, S), ("auto", 3, 64, 10, 256, C), ("auto", 210, 16, 2, 8, S), ("auto", 1, 130, 3, 72, C),
    ("auto", 1, 65, 2, 33, S),
    ("auto_no_team", 5, 2, 16, 36, C), ("auto_no_team", 3, 64, 10, 256, S), ("auto_no_team", 2, 100, 5, 40, S),
    ("auto_no_team", 2, 7, 4, 65, S),
]
AUTO_REACHES = {"auto": {"wave", "team", "fused_split", "tiled", "generic"},
                "auto_no_team": {"wave", "fused_split", "tiled", "generic"}}

# the edges the issue lists, per implementation: (field, values that must each appear in a case of that implementation)
REQUIRED = {
    "generic": {"D": {1, 7, 33, 65}, "N": {1, 65}, "M": {2}},
    "fused_f32": {"D": {64, 256}, "M": {2}},
    "fused_split": {"D": {4, 36, 100, 200, 252, 256}, "M": {2}},
    "team": {"N": {16, 23, 40, 57, 64}, "D": {4, 80, 132, 200, 252, 256}, "B": {1, 2, 9, 70}},
    "tiled": {"N": {1, 15, 65, 130, 300}, "D": {8, 72, 200, 264, 776, 1024}, "B": {1, 3}},
    "wave": {"D": {4, 36, 252, 256}, "B": {1, 5, 2100}},
}

# What LOSS_CASES, RAW_CASES and COS_CASES leave out, one level below ge2e_resolve_impl: every launcher picks again among
# kernels and template instantiations, and the library's plan queries (ge2e_loss_plan, ge2e_cos_sim_plan) name the pick.
# Each entry is there for ONE kernel name ("atom") that no case of the three tables above launches -- test_plan_cases.py
# holds the union over all four tables to ge2e_plan_atoms and fails naming the atom if an entry is taken out --, and
# tests/test_gpu_plans.py runs it:  (atom, impl, B, N, M, D, variant, grad)   grad False: forward only (dE = NULL).
#   team / team_fwd <NCH, MR, 0, variant>: NCH = ceil(D / 64), MR = 10 for M <= 10 else 16.  The tables above hold the D
#     edges and the M edges one at a time; these are the cells of the product they miss, with uneven members (N % 8 != 0),
#     D off the multiples of 64, one and several batches.  The variant is a template argument, so both run.
#   fused_split<3>: 128 < D <= 192.
#   tiled_gc<C2>, tiled_gc<C3>/S: the 256 x 256 centroid-gradient contraction needs N >= 256, D >= 256 and at least 192
#     tiles, B ceil(N / 256) ceil(D / 256) >= 192: more than MAX_ELEMS, so tests/test_gpu_plans.py makes these inputs on
#     the device.  Each shape is the one with the fewest elements at which the query names the atom (searched over N
#     256..1024, M 2..6, D in 256, 264, 288, 512, 520, B <= 130): D = 264 has two d tiles, N > 256 two slot tiles, so 48
#     batches fill 192 tiles.  gc<C2>: N M = 514 is no multiple of 32.  gc<C3>/1: 192 tiles fill three quarters of a round
#     and so do 384; /2: 260 tiles are half of two rounds, 520 two thirds of three; /4 and /8 need 8 K-steps of 32 rows per
#     piece, N M >= 1024 and 2048.  The query decides; PLAN_TILES keeps the counts.
#     Softmax: the variant is a run-time argument of gc, ge, sim and rows, and tens of thousands of contrast rows tie.
#   The DMA-fed kernels (C3) walk their tiles b, b + grid, ... with at most 256 workgroups: PLAN_TILES notes the tile count of
#     every C3 kernel of a case, and for each of sim<C3>, gc<C3>, ge<C3> one case has more than 256 (gc<C2>'s case takes
#     D = 288 instead of the smallest D = 264 for that: its similarity contraction then is sim<C3> with 288 tiles).
PLAN_CASES = [
    ("team<1,10,0,softmax>", "team", 3, 23, 7, 60, S, True), ("team_fwd<1,10,0,softmax>", "team", 3, 23, 7, 60, S, False),
    ("team<1,10,0,contrast>", "team", 2, 40, 10, 64, C, True), ("team_fwd<1,10,0,contrast>", "team", 2, 40, 10, 64, C, False),
    ("team<2,10,0,softmax>", "team", 3, 57, 5, 128, S, True), ("team_fwd<2,10,0,softmax>", "team", 3, 57, 5, 128, S, False),
    ("team<3,10,0,softmax>", "team", 5, 33, 9, 132, S, True), ("team_fwd<3,10,0,softmax>", "team", 5, 33, 9, 132, S, False),
    ("team<3,10,0,contrast>", "team", 2, 64, 10, 192, C, True), ("team_fwd<3,10,0,contrast>", "team", 2, 64, 10, 192, C, False),
    ("team<1,16,0,contrast>", "team", 3, 17, 11, 36, C, True), ("team_fwd<1,16,0,contrast>", "team", 3, 17, 11, 36, C, False),
    ("team<2,16,0,softmax>", "team", 2, 40, 16, 100, S, True), ("team_fwd<2,16,0,softmax>", "team", 2, 40, 16, 100, S, False),
    ("team<2,16,0,contrast>", "team", 5, 9, 13, 128, C, True), ("team_fwd<2,16,0,contrast>", "team", 5, 9, 13, 128, C, False),
    ("team<3,16,0,contrast>", "team", 3, 24, 12, 192, C, True), ("team_fwd<3,16,0,contrast>", "team", 3, 24, 12, 192, C, False),
    ("team<4,16,0,softmax>", "team", 2, 33, 16, 200, S, True), ("team_fwd<4,16,0,softmax>", "team", 2, 33, 16, 200, S, False),
    ("team<4,16,0,contrast>", "team", 3, 16, 11, 256, C, True), ("team_fwd<4,16,0,contrast>", "team", 3, 16, 11, 256, C, False),
    ("fused_split<3>", "fused_split", 2, 20, 5, 132, S, True),
    ("tiled_gc<C2>", "tiled", 48, 257, 2, 288, S, True), ("tiled_gc<C3>/1", "tiled", 48, 272, 2, 264, S, True),
    ("tiled_gc<C3>/2", "tiled", 65, 272, 2, 264, S, True), ("tiled_gc<C3>/4", "tiled", 32, 528, 2, 264, S, True),
    ("tiled_gc<C3>/8", "tiled", 25, 800, 3, 264, S, True),
]


def plan_id(c):
    return "{}-{}".format(c[0], case_id(c[1:7]))


def plan_is_small(c):
    """Small enough for the fp64 closed form on the CPU and for the guarded C-ABI route of test_gpu_bounds.py."""
    return c[2] * c[3] * c[4] * c[5] <= MAX_ELEMS


def c3_tiles(c):
    """Tiles of the 256 x 256 DMA-fed contractions of a tiled case, by kernel name (0: that kernel is not C3 here).  The
    tile counts are launch_tiled's grid arithmetic; WHICH kernels are C3 is read off the plan, not recomputed."""
    from speaker_embedding_ge2e_loss_amd import _lib
    _, impl, B, N, M, D, variant, grad = c
    t = lambda n: (n + 255) // 256  # noqa: E731
    plan = _lib.loss_plan(B, N, M, D, variant, impl, grad)
    split = next((int(a.split("/")[1]) for a in plan if a.startswith("tiled_gc<C3>")), 0)
    return {"tiled_sim<C3>": B * t(N * M) * t(N) if "tiled_sim<C3>" in plan else 0,
            "tiled_gc<C3>": B * t(N) * t(D) * split,
            "tiled_ge<C3>": B * t(N * M) * t(D) if "tiled_ge<C3>" in plan else 0}


# c3_tiles of the tiled PLAN_CASES as they stand (test_plan_cases.py keeps the note true): the walk runs more than one
# round wherever a count passes 256
PLAN_TILES = {
    "tiled_gc<C2>": {"tiled_sim<C3>": 288, "tiled_gc<C3>": 0, "tiled_ge<C3>": 0},
    "tiled_gc<C3>/1": {"tiled_sim<C3>": 0, "tiled_gc<C3>": 192, "tiled_ge<C3>": 0},
    "tiled_gc<C3>/2": {"tiled_sim<C3>": 0, "tiled_gc<C3>": 520, "tiled_ge<C3>": 0},
    "tiled_gc<C3>/4": {"tiled_sim<C3>": 0, "tiled_gc<C3>": 768, "tiled_ge<C3>": 0},
    "tiled_gc<C3>/8": {"tiled_sim<C3>": 0, "tiled_gc<C3>": 1600, "tiled_ge<C3>": 500},
}


def table_plans(lib):
    """{table: [(what, [atoms])]}: the plan of every call the GPU tests make from the four tables -- LOSS_CASES with and
    without gradients (COMBOS has forward-only calls), RAW_CASES likewise, COS_CASES on the full workspace, PLAN_CASES."""
    from speaker_embedding_ge2e_loss_amd import _lib
    out = {"LOSS_CASES": [], "RAW_CASES": [], "COS_CASES": [], "PLAN_CASES": []}
    for c in LOSS_CASES:
        impl, B, N, M, D, variant = c
        for grad in sorted({combo[2] for combo in COMBOS}):
            out["LOSS_CASES"].append((f"{case_id(c)}/{'grad' if grad else 'fwd'}", _lib.loss_plan(B, N, M, D, variant, impl, grad)))
    for c in RAW_CASES:
        B, N, M, D, variant = resolve_raw(lib, c)
        for grad in (True, False):
            out["RAW_CASES"].append((f"raw {raw_id(c)}/{'grad' if grad else 'fwd'}", _lib.loss_plan(B, N, M, D, variant, want_grad=grad, raw=True)))
    for c in COS_CASES:
        out["COS_CASES"].append((f"cos {c}", _lib.cos_sim_plan(*c)))
    for c in PLAN_CASES:
        _, impl, B, N, M, D, variant, grad = c
        out["PLAN_CASES"].append((plan_id(c), _lib.loss_plan(B, N, M, D, variant, impl, grad)))
    return out


# output combinations: (name, per, grads, misaligned)
COMBOS = [("all", True, True, False), ("no_per", False, True, False), ("fwd_per", True, False, False),
          ("fwd", False, False, False), ("misaligned", True, True, True)]

# ge2e_cos_sim: (B, N, M, D).  N = 16 with D % 64 == 0 is the header's edge of the matrix-core route; N M = 48, 195, 1050
# are no multiples of 64; (2, 15, 4, 64) stays on the VALU kernel whatever the workspace (N < 16).
# At (1, 16, 3, 64) and (1, 16, 3, 72) the generic size (control block included) is the LARGER of the two, so both
# workspaces are the same, the matrix-core route runs with slack behind its last region and the workspace guard cannot bite
# there: those two check the outputs' guards and the values only.  The exact-size property, and "the smaller workspace
# takes the VALU kernel", are carried by the cases where ge2e_cos_sim_workspace_bytes is the tiled size: (1, 16, 64, 256) --
# the header's edge again, with enough rows for that --, (3, 16, 16, 256), (2, 65, 3, 128), (1, 300, 3, 768).
COS_CASES = [(1, 16, 3, 64), (1, 16, 64, 256), (3, 16, 16, 256), (2, 65, 3, 128), (1, 15, 70, 64), (1, 300, 3, 768), (2, 15, 4, 64), (1, 16, 3, 72)]

# ge2e_loss_fwd_bwd_raw: (B, N or "max", M, D, variant); "max" = the largest N ge2e_raw_supported takes for that M.
# Every instantiated M, at its largest N and at N = 1, with B = 1, 3 and 2100 (more than the grid's 2048 waves): each
# <M, NX, RAW> is a kernel of its own.  D cycles through RAW_DS; where B rows D would pass MAX_ELEMS the next D that fits is
# taken (a wave holds at most 64 rows, the header's limit, so B = 2100 at the largest N runs at D = 4 and 36 only).
# Contrast wherever there is another speaker and B < 2100 (tens of thousands of contrast rows would tie, see above).
RAW_MS = (2, 3, 4, 5, 6, 8, 10, 16)
RAW_DS = (4, 36, 252, 256)
RAW_BS = (1, 3, 2100)


def _raw_cases():
    out = []
    for mi, M in enumerate(RAW_MS):
        for ni, N in enumerate(("max", 1)):
            for bi, B in enumerate(RAW_BS):
                rows = 64 if N == "max" else M
                k = mi + bi + 2 * ni
                D = next(RAW_DS[(k + i) % 4] for i in range(4) if B * rows * RAW_DS[(k + i) % 4] <= MAX_ELEMS)
                out.append((B, N, M, D, C if (N == "max" and B < 2100) else S))
    return out


RAW_CASES = _raw_cases()


def case_id(c):
    return "{}_B{}_N{}_M{}_D{}_{}".format(*c[:5], c[5][0])


def raw_id(c):
    return "B{}_N{}_M{}_D{}_{}".format(*c[:4], c[4][0])


def raw_max_n(lib, M, D):
    """The largest N ge2e_raw_supported accepts for (M, D); 0 if none."""
    n = 0
    while lib.ge2e_raw_supported(n + 1, M, D):
        n += 1
    return n


def resolve_raw(lib, case):
    B, N, M, D, variant = case
    return (B, raw_max_n(lib, M, D) if N == "max" else N, M, D, variant)


# draws chosen on the CPU (test_bounds_cases.py) because the default one ties two other-speaker similarities of a row
SEEDS = {("tiled", 64, 130, 4, 32, C): 2, ("tiled", 64, 256, 3, 32, C): 2}


def loss_inputs(case):
    _, B, N, M, D, _ = case
    return orc.synth_embeddings((B, N, M, D), "raw", seed=SEEDS.get(case, B + N + M + D))


@functools.lru_cache(maxsize=None)
def loss_reference(case):
    return orc.closed_form(loss_inputs(case), W, BIAS, variant=case[5])


def top2_gap_ok(ref, N):
    """test_gpu_fuzz.py's criterion: eq. 7's max over the other speakers must not tie within what fp32 resolves."""
    if N <= 2:
        return True
    Sm = W * np.asarray(ref["cos"], np.float64) + BIAS
    Sm = Sm.reshape((-1,) + Sm.shape[-3:])
    jj = np.arange(N)
    Sm[:, jj, :, jj] = -np.inf
    top2 = np.sort(Sm, axis=-1)[..., -2:]
    return float((top2[..., 1] - top2[..., 0]).min()) >= 5e-6 * max(1.0, float(np.abs(top2[..., 1]).max()))


def raw_inputs(case):
    """Y [B][N M][D] with rows of very different norm (as test_loss_raw_is_normalize_unperm_then_loss), and a different
    permutation per batch: src [B][N M] int32."""
    B, N, M, D, _ = case
    rng = np.random.default_rng(1000 * N + 100 * M + D + B)
    Y = rng.standard_normal((B, N * M, D)) * (0.5 + 2.0 * rng.random((B, N * M, 1)))
    src = np.stack([rng.permutation(N * M) for _ in range(B)]).astype(np.int32)
    return np.ascontiguousarray(Y, dtype=np.float32), src


def raw_reference(case, Y, src):
    """fp64: normalise and gather, the closed form, dE back through (g - e (e . g)) / |y|, scatter."""
    B, N, M, D, variant = case
    y = Y.astype(np.float64)
    norm = np.linalg.norm(y, axis=-1, keepdims=True)
    e = y / norm
    bi = np.arange(B)[:, None]
    idx = src if src is not None else np.broadcast_to(np.arange(N * M), (B, N * M))
    eg = e[bi, idx]                                             # row r of the block is Y[src[r]] / |Y[src[r]]|
    ref = orc.closed_form(eg.reshape(B, N, M, D), W, BIAS, variant=variant, dtype=np.float64)
    g = ref["dE"].reshape(B, N * M, D)
    gy = (g - eg * (eg * g).sum(axis=-1, keepdims=True)) / norm[bi, idx]
    dY = np.zeros_like(y)
    dY[bi, idx] = gy
    return dict(ref, dY=dY)
