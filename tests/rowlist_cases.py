"""Inputs and fp64 references of the row-list tests (ragged, labelled, masked, wide, labelled evaluation and its gradients): a
plain module, no GPU code; tests/test_rowlist_cases.py checks the last three groups without a GPU.

    EDGE / case(counts, D, seed, v)      the ragged kernel's edge shapes; one sorted batch and its ragged_ref reference
    inputs / draw / mixed_draw           unit rows for labels of any content; seeded labels; what every random draw must hold
    LOSS_CASES / loss_case(name, v)      the masked loss's batches and their masked_ref references
    INDEX_CASES / RANDOM_INDEX_CASES     label tables of the masked index kernel
    EDGE_CASES / edge_case(name)         the labelled evaluation's batches and their labeled_eval_ref references
    reference / cos_reference / host_ids one batch's masked_ref (labeled_eval_ref) reference; arbitrary host ids
    golden_rows(name)                    a golden (N, M, D) block as a shuffled row list with lone and ignored rows appended
    degenerate_case(kind, v)             ragged counts, one speaker with a zero / tiny row, equal rows, a zero (leave-one-out) centroid
    cases(n, seed)                       seeded random row lists: shapes, both variants, unit and raw rows, three scales, w and b

References are tests/ragged_ref.py and tests/masked_ref.py (torch autograd in float64), tests/labeled_eval_ref.py (numpy float64)
and the golden files' own float64 numbers.  Every draw is held, before anything is launched, to what its case is named for.
Whatever is expensive is computed once (functools.lru_cache), shared and read-only.
"""
import functools
import zlib

import numpy as np

import labeled_eval_ref as ler
import masked_ref as mr
import ragged_ref as rr
from conftest import load_golden
from rowlist_harness import BIAS, EPS, EPS_COS, KEYS, W

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the ragged kernel's edge shapes -------------------------------------------------------------------------------------------
EDGE = {
    "D20_long_and_2row_speakers": ([2, 17, 3, 65, 2], 20),     # D no multiple of 16 or 64, a speaker longer than a wave
    "N67": ([2] * 67, 36),                                     # more than 64 centroids
    "speaker_over_row_tiles": ([130, 2], 8),                   # one speaker over several 16-row tiles
    "N1": ([5], 12),                                           # one speaker: a vanishing gradient
    "many_short": (np.random.default_rng(0).integers(2, 12, size=33).tolist(), 100),
    "D1": ([3, 2], 1),
    "D5": ([2, 3, 4], 5),
}


@functools.lru_cache(maxsize=None)
def _case(counts, D, seed, variant):
    E = rr.ragged_inputs(counts, D, seed)
    E.setflags(write=False)
    ref = rr.ragged_loss(E, counts, W, BIAS, variant=variant)
    for v in ref.values():
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return E, ref


def case(counts, D, seed, variant):
    """Inputs and fp64 reference of one batch: computed once, shared, read-only."""
    return _case(tuple(int(c) for c in counts), int(D), int(seed), variant)


# ---- labels of any content: inputs, draws, the masked loss's and index kernel's cases --------------------------------------------
def inputs(labels, N, D, seed):
    """Unit rows centre[class] + 0.5 noise, float32 (R, D); class = the label where 0 <= label < N, one more class otherwise."""
    labels = np.asarray(labels, dtype=np.int64)
    rng = np.random.default_rng(seed)
    cls = np.where((labels >= 0) & (labels < N), labels, N)
    centre = rng.standard_normal((N + 1, D))
    x = centre[cls] + 0.5 * rng.standard_normal((len(labels), D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32)


def mixed_draw(idx, N):
    """Whether a draw holds what every random case must: >= 2 active speakers, a lone one, an absent one, an ignored row."""
    hist = np.bincount(idx["labels"][(idx["labels"] >= 0) & (idx["labels"] < N)], minlength=N)
    return (idx["active"][0] >= 2 and bool((hist == 1).any()) and bool((hist == 0).any())
            and bool(((idx["labels"] < 0) | (idx["labels"] >= N)).any()))


def draw(N, R, n_active, n_lone, n_ignored, seed, spread=None):
    """Seeded labels (R,): `n_active` speakers share the rows that are left (each >= 2), `n_lone` speakers have one row,
    `n_ignored` rows carry labels outside [0, N); the speakers are drawn from range(N) (or from `spread`), rows shuffled."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(N if spread is None else spread, size=n_active + n_lone, replace=False)
    rows = R - n_lone - n_ignored
    assert rows >= 2 * n_active and n_active + n_lone < N
    counts = np.full(n_active, 2)
    for _ in range(rows - 2 * n_active):
        counts[rng.integers(n_active)] += 1
    outside = rng.choice(np.array([-1, N, N + 5, -7, I32_MIN, I32_MAX]), size=n_ignored)
    lab = np.concatenate([np.repeat(ids[:n_active], counts), ids[n_active:], outside])
    return lab[rng.permutation(R)].astype(np.int32)


def _loss_cases():
    big = np.array([4] * 130 + [0, 1, 2, 6, -1, 8, 9], dtype=np.int32)           # one speaker of 130 rows among lone ones
    return {
        # name: (labels, N, D, random draw?)
        "nact1_D5": (np.array([3, 1, 3, -1], dtype=np.int32), 5, 5, False),      # one pair, one lone row, one ignored row
        "nact0": (np.array([0, 1, 2, -1, 7, 4, 3], dtype=np.int32), 4, 6, False),
        "nact17_of_N40_D36": (draw(40, 75, 17, 4, 5, 1), 40, 36, True),
        "ract33_in_R48": (draw(12, 48, 5, 6, 9, 2), 12, 20, True),
        "ract32_in_R45": (draw(12, 45, 6, 4, 9, 3), 12, 16, True),
        "one_of_130_among_lone_D8": (big[np.random.default_rng(4).permutation(len(big))], 8, 8, False),
        "N1251_bound_R80": (draw(1251, 80, 23, 9, 6, 5), 1251, 16, True),
    }


LOSS_CASES = _loss_cases()


@functools.lru_cache(maxsize=None)
def loss_case(name, variant):
    """(E, labels, N, fp64 reference) of one batch: computed once, shared, read-only."""
    labels, N, D, random = LOSS_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    ref = mr.masked_loss(E, labels, N, W, BIAS, variant=variant)
    ref["index"]["labels"] = labels
    assert not random or mixed_draw(ref["index"], N), f"{name}: the draw does not hold every kind of row"
    for v in [E] + [ref[k] for k in KEYS]:
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return E, labels, N, ref


def reference(E, labels, N, variant):
    """The fp64 reference of one batch, finite and read-only, with the labels beside the index tables."""
    ref = mr.masked_loss(E, labels, N, W, BIAS, variant=variant)
    ref["index"]["labels"] = np.asarray(labels)
    for k in KEYS:
        assert np.isfinite(ref[k]).all()
        ref[k].setflags(write=False)
    return ref


def _index_cases():
    rng = np.random.default_rng(21)
    n600 = np.concatenate([np.repeat([0, 255, 256, 511, 512, 599], [2, 3, 2, 4, 2, 3]), [1, 254, 257, 510, 513, 598, 600, -1]])
    # runs of ignored rows across the 256-row chunks and the 64-row waves, valid rows of 3 speakers in between
    runs = rng.integers(0, 3, 2500)
    for lo, hi in ((60, 70), (250, 262), (500, 520), (700, 1100), (1279, 1281), (1530, 1800), (2490, 2500)):
        runs[lo:hi] = rng.choice([-1, 3, I32_MAX], size=hi - lo)
    # the second batch: nine lone speakers and 31 labels outside the bound, nothing counts
    b3 = np.stack([draw(9, 40, 3, 2, 4, 31), np.concatenate([np.arange(9), 9 + np.arange(31) % 9]), draw(9, 40, 1, 5, 7, 32)])
    return {
        "every_row_ignored": (4, np.array([[-1, 4, 100, -1, I32_MIN, 4, I32_MAX]])),
        "every_speaker_lone": (8, rng.permutation(8)[None]),
        "wild_values_among_valid": (5, np.array([[2, -1, 0, 5, I32_MIN, 2, I32_MAX, 0, 4, 2, 5, -1, 3, 3]])),
        "N1": (1, np.array([[0, 0, -1, 0, 1]])),
        "N1_lone": (1, np.array([[1, 0, -1]])),
        "R1": (3, np.array([[2]])),
        "N600_across_the_scan_rounds": (600, n600[rng.permutation(len(n600))][None]),
        "N1100_R300": (1100, draw(1100, 300, 40, 60, 30, 22)[None]),           # counters in the workspace, most absent
        "N5000_R64": (5000, draw(5000, 64, 11, 20, 9, 23)[None]),
        "R2500_ignored_runs": (3, runs[None]),
        "B3_own_nact_one_empty": (9, b3),
        "B515_past_the_grid": (3, rng.integers(-1, 4, (515, 7))),
        "B3_N1100": (1100, np.stack([draw(1100, 90, 10 * i + 1, 7, 5, 24 + i) for i in range(3)])),
    }


INDEX_CASES = _index_cases()
# the batches of the seeded random cases that are drawn to hold >= 2 active speakers, a lone one, an absent one, an ignored row
RANDOM_INDEX_CASES = {"N1100_R300": (0,), "N5000_R64": (0,), "B3_own_nact_one_empty": (0,), "B3_N1100": (1, 2)}


# ---- the labelled evaluation's cases -------------------------------------------------------------------------------------------
def cos_reference(E, labels, N):
    """The float64 reference of one batch as a dict."""
    cos, col, speakers, active = ler.cos_ref(E, labels, N)
    return {"cos": cos, "col": col, "speakers": speakers, "active": active}


def _edge_cases():
    rng = np.random.default_rng(67)
    cases = {name: (labels, N, D) for name, (labels, N, D, _) in LOSS_CASES.items()}
    cases["nact67_of_2_rows_D36"] = (np.repeat(np.arange(67), 2)[rng.permutation(134)].astype(np.int32), 67, 36)   # five column tiles
    cases["D1"] = (draw(6, 20, 3, 1, 2, 61), 6, 1)
    cases["D37_scalar_loads"] = (draw(10, 40, 4, 2, 3, 62), 10, 37)
    cases["D260_past_the_held_rows"] = (draw(10, 40, 4, 2, 3, 63), 10, 260)     # vector loads, a partial 17th K step
    return cases


EDGE_CASES = _edge_cases()


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(E, labels, N, float64 reference) of one batch: computed once, shared, read-only."""
    labels, N, D = EDGE_CASES[name]
    E = inputs(labels, N, D, 4000 + len(labels) + D)
    ref = cos_reference(E, labels, N)
    for v in [E] + list(ref.values()):
        v.setflags(write=False)
    return E, labels, N, ref


def host_ids(labels, N, seed):
    """Arbitrary host ids for dense labels: the valid ones keep their order, every other row a negative id of its own."""
    ids = np.sort(np.random.default_rng(seed).choice(10 ** 6, size=N, replace=False))
    return np.where((labels >= 0) & (labels < N), ids[np.clip(labels, 0, N - 1)], -1 - np.arange(len(labels)))


# ---- what the row-list entry points had never been fed: golden blocks, degenerate rows, seeded random row lists ------------------
DS = (4, 5, 20, 36, 37, 64, 96, 128, 200, 256, 260)
SCALES = (1e-2, 1.0, 1e2)
KINDS = ("unit", "raw")
N_DEFAULT, SEED_DEFAULT = 48, 7


def wide_split(R):
    """csrc/ge2e_labeled_wide.hpp: the pieces GC's K loop is cut into."""
    return min(max((R + 127) // 128, 1), 8)


def frozen(ref):
    for k in KEYS:
        assert np.isfinite(ref[k]).all(), k
        ref[k].setflags(write=False)
    return ref


# ---- 1. golden fixtures as row lists -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_rows(name):
    """(E (R, D) float32, labels (R,) int32, bound, ref, w, b) of one golden block: its N M rows with labels
    repeat(arange(N), M), then two lone-speaker rows (labels N, N + 1) and three rows labelled -1, N + 2, INT32_MAX that hold
    NaN, +Inf, -Inf (N + 2 is inside the bound N + 3: one more lone speaker, whose only row is +Inf), all shuffled.  ref: the
    fixture's float64 numbers scattered through the permutation, 0 on the appended rows; "counted": the fixture's rows in the
    fixture's order; "index": masked_ref's tables."""
    g = load_golden(name)
    N, M, D = g["E"].shape
    R0, R = N * M, N * M + 5
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    tail = rng.standard_normal((5, D)).astype(np.float32)
    tail[2:] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[:, None]
    E_all = np.concatenate([np.asarray(g["E"], np.float32).reshape(R0, D), tail])
    lab_all = np.concatenate([np.repeat(np.arange(N), M), [N, N + 1, -1, N + 2, I32_MAX]])
    perm = rng.permutation(R)
    E, labels = np.ascontiguousarray(E_all[perm]), lab_all[perm].astype(np.int32)
    counted = np.argsort(perm)[:R0]                      # counted[i]: where the fixture's row i went
    per, dE = np.zeros(R), np.zeros((R, D))
    per[counted] = np.asarray(g["per64"], np.float64).reshape(R0)
    dE[counted] = np.asarray(g.get("dE64", g["dE"]), np.float64).reshape(R0, D)
    idx = mr.index_ref(labels, N + 3)
    assert idx["active"].tolist() == [N, R0] and np.array_equal(np.flatnonzero(idx["active_row"]), np.sort(counted))
    ref = {"loss": np.asarray(g["loss64"], np.float64), "per": per, "dE": dE, "dw": np.asarray(g["dw64"], np.float64),
           "db": np.asarray(g["db64"], np.float64), "index": idx, "counted": counted}
    for v in (E, labels, counted):
        v.setflags(write=False)
    return E, labels, N + 3, frozen(ref), float(g["w"]), float(g["b"])


# ---- 2. degenerate rows among ragged counts ------------------------------------------------------------------------------------
DEG_COUNTS, DEG_D = (3, 2, 4, 3, 70), 8                  # speaker 4 covers sorted positions 12 .. 81: it crosses a 64-row tile
DEG_KINDS = {"zero_row": 0, "tiny_row": 3, "identical_rows": 2, "loo_zero": 3, "zero_centroid": 1}   # kind: its speaker
# The kinds whose reference gradient is huge: a norm below eps_cos is clamped to eps_cos = 1e-8, so the cosine's slope in the
# clamped vector is 1 / eps_cos times the ordinary one.  (Equal rows are degenerate in another way: every leave-one-out centroid
# is the row itself, the own cosine is exactly 1 and its gradient vanishes.)
DEG_HUGE = ("zero_row", "tiny_row", "loo_zero", "zero_centroid")


@functools.lru_cache(maxsize=None)
def degenerate_case(kind, variant):
    """(E (R, D), labels (R,), N, ref, deg) for counts DEG_COUNTS + one ignored row, unit rows except for speaker
    DEG_KINDS[kind]; `deg` (R,) bool: the rows of that speaker.  w = 10, b = -5."""
    spk = DEG_KINDS[kind]
    N, D = len(DEG_COUNTS), DEG_D
    lab = np.concatenate([np.repeat(np.arange(N), DEG_COUNTS), [-1]])
    E = inputs(lab, N, D, 600 + sorted(DEG_KINDS).index(kind))
    rng = np.random.default_rng(77)
    rows = np.flatnonzero(lab == spk)
    assert len(rows) == DEG_COUNTS[spk] <= 4
    if kind == "zero_row":
        E[rows[1]] = 0.0
    elif kind == "tiny_row":                             # 0 < |e| < eps_cos, squares still normal fp32 numbers
        E[rows[2]] = (rng.standard_normal(D) * 1e-9).astype(np.float32)
    elif kind == "identical_rows":
        E[rows] = E[rows[0]]
    elif kind == "loo_zero":                             # x, y, -y in multiples of 1/64: x + y - y is x in fp32 in ANY order, so
        E[rows] = np.round(E[rows] * 64.0) / 64.0        # the first row's leave-one-out centroid is exactly 0 in a kernel too
        E[rows[2]] = -E[rows[1]]
    elif kind == "zero_centroid":                        # y, -y, rounded the same way: the centroid is exactly 0
        E[rows[0]] = np.round(E[rows[0]] * 64.0) / 64.0
        E[rows[1]] = -E[rows[0]]
    else:
        raise ValueError(kind)
    perm = np.random.default_rng(5).permutation(len(lab))
    E, labels = np.ascontiguousarray(E[perm]), lab[perm].astype(np.int32)
    deg = labels == spk
    ref = mr.masked_loss(E, labels, N, W, BIAS, variant=variant)
    idx = ref["index"]
    assert idx["active"].tolist() == [N, sum(DEG_COUNTS)] and idx["counts"].tolist() == list(DEG_COUNTS)
    assert idx["offsets"][4] < 64 < idx["offsets"][5] and int((~idx["active_row"]).sum()) == 1
    frozen(ref)
    rest = idx["active_row"] & ~deg
    big, plain = float(np.abs(ref["dE"][deg]).max()), float(np.abs(ref["dE"][rest]).max())
    assert plain < 50.0, f"{kind}/{variant}: a gradient of {plain:.3e} outside the degenerate speaker"
    assert (big > 1e6) == (kind in DEG_HUGE), f"{kind}/{variant}: {big:.3e} on the degenerate speaker's rows"
    for v in (E, labels, deg):
        v.setflags(write=False)
    return E, labels, N, ref, deg


# ---- 3. seeded random cases ----------------------------------------------------------------------------------------------------
def cases(n=N_DEFAULT, seed=SEED_DEFAULT):
    """n tuples (B, N, R, D, n_active, n_lone, n_ignored, variant, kind, scale, w, b, seed).  B 1..4 batches of one shape,
    each with labels of its own; bound N 2..90 (draw keeps one speaker absent, so 3 is the smallest that
    holds two active ones); R 4..330; n_active >= 2, from one of the ranges 2..16, 17..64, 65.. that N and R leave room for,
    so that the rows kernel's one, several and more than four column tiles all come up; contrast with probability 0.3.
    D = 1 and n_active = 1 are left out on purpose: the gradient vanishes there and a relative gate means nothing (the edge
    tests of test_gpu_masked.py and test_gpu_ragged.py hold both)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        B, N, R = int(rng.integers(1, 5)), int(rng.integers(2, 91)), int(rng.integers(4, 331))
        D = int(rng.choice(DS))
        top = min(N - 1, R // 2)
        if top < 2:
            continue
        ranges = [(lo, min(hi, top)) for lo, hi in ((2, 16), (17, 64), (65, 89)) if lo <= top]
        lo, hi = ranges[int(rng.integers(len(ranges)))]
        n_active = int(rng.integers(lo, hi + 1))
        spare = R - 2 * n_active
        n_lone = int(rng.integers(0, min(N - 1 - n_active, spare, 6) + 1))
        n_ignored = int(rng.integers(0, min(spare - n_lone, 8) + 1))
        variant = "contrast" if rng.random() < 0.3 else "softmax"
        kind, scale = KINDS[int(rng.integers(2))], SCALES[int(rng.integers(3))]
        out.append((B, N, R, D, n_active, n_lone, n_ignored, variant, kind, scale,
                    float(rng.uniform(-4, 14)), float(rng.uniform(-6, 3)), int(rng.integers(1 << 30))))
    return out


def case_id(c):
    return "B{}_N{}_R{}_D{}_a{}_{}_{}_{:g}".format(*c[:5], c[7][0], c[8], c[9])


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """E (B, R, D) float32, labels (B, R) int32 of a case; read-only."""
    B, N, R, D, n_active, n_lone, n_ignored, _, kind, scale, _, _, seed = c
    labels = np.stack([draw(N, R, n_active, n_lone, n_ignored, seed + i) for i in range(B)])
    if kind == "unit":
        E = np.stack([inputs(labels[i], N, D, seed + 100 + i) for i in range(B)])
    else:                                                # oracle.synth_embeddings' "raw": randn scaled per row by U(0.5, 1.5)
        rng = np.random.default_rng(seed + 100)
        E = rng.standard_normal((B, R, D)).astype(np.float32)
        E *= rng.uniform(0.5, 1.5, size=(B, R, 1)).astype(np.float32)
    E = np.ascontiguousarray(E * np.float32(scale), dtype=np.float32)
    E.setflags(write=False)
    labels.setflags(write=False)
    return E, labels


@functools.lru_cache(maxsize=None)
def case_references(c):
    """The float64 reference of every batch of a case, finite and read-only, the labels beside the index tables."""
    E, labels = case_inputs(c)
    refs = []
    for i in range(c[0]):
        ref = mr.masked_loss(E[i], labels[i], c[1], c[10], c[11], variant=c[7])
        ref["index"]["labels"] = labels[i]
        refs.append(frozen(ref))
    return tuple(refs)


def ties(E, idx, w, b):
    """test_gpu_fuzz.py's rule on one batch: whether some row's two largest similarities to OTHER speakers are closer than
    5e-6 max(1, max|S|).  There the contrast loss's max is not smooth: fp32 and fp64 may pick different speakers and the
    row's gradient moves to another centroid.  float64 numpy on the rows that count."""
    n_act, r_act = (int(v) for v in idx["active"])
    if n_act <= 2:
        return False
    e = np.asarray(E, np.float64)[idx["order"][:r_act]]
    own = np.repeat(np.arange(n_act), idx["counts"])
    cent = np.stack([e[own == k].mean(axis=0) for k in range(n_act)])
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), EPS_COS)  # noqa: E731
    S = w * (unit(e) @ unit(cent).T + EPS) + b
    S[np.arange(r_act), own] = -np.inf
    top2 = np.sort(S, axis=1)[:, -2:]
    return bool(float((top2[:, 1] - top2[:, 0]).min()) < 5e-6 * max(1.0, float(np.abs(top2[:, 1]).max())))


def tied_batches(c):
    """The batches of a contrast case that fall under the tie rule."""
    if c[7] != "contrast":
        return ()
    E, _ = case_inputs(c)
    return tuple(i for i, ref in enumerate(case_references(c)) if ties(E[i], ref["index"], c[10], c[11]))
