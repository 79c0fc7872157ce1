"""Reference for the static helpers of the C ABI on LOCAL ROWS (include/ge2e_hip.h: ge2e_cos_sim_rows, ge2e_calc_loss_rows,
ge2e_centroids, ge2e_utterance_centroids, ge2e_scale_grads and their backward passes): batched torch CPU functions whose
autograd gives the expected gradients.  TEST INFRASTRUCTURE, fp64 by default; the same functions run in fp32 where a test
needs the reference's own fp32 error.

Written from oracle/ge2e_oracle.py (expand_form_cos_sim, _softmax_rows, _contrast_rows) and the header's formulas, extended
to a slice of n speakers whose columns are j0 .. j0 + n - 1 of N centroids.  tests/test_helpers_ref.py anchors it: with
B = 1, n = N, j0 = 0 it IS the oracle's expand form.

Also the shape tables of tests/test_gpu_helpers.py and their seeded inputs, so that the CPU suite can check that the
reference is finite on every one of them.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS_COS = 1e-8
SMALL_ERR = 1e-6


def _own_mask(n, N, j0):
    m = torch.zeros(n, N, dtype=torch.bool)
    m[torch.arange(n), j0 + torch.arange(n)] = True
    return m


def cos_rows(E, C, j0, eps=SMALL_ERR, eps_cos=EPS_COS):
    """E (B,n,M,D), C (B,N,D) -> cos (B,n,M,N): F.cosine_similarity (the op the reference calls) of every row with the
    caller's centroids; column j0 + jl of local speaker jl = cosine with the leave-one-out centroid of the local rows;
    + eps on every entry."""
    B, n, M, D = E.shape
    N = C.shape[1]
    loo = (E.sum(dim=2, keepdim=True) - E) / (M - 1)
    own = F.cosine_similarity(E, loo, dim=-1, eps=eps_cos)                                  # (B,n,M)
    oth = F.cosine_similarity(E.unsqueeze(3), C.reshape(B, 1, 1, N, D), dim=-1, eps=eps_cos)  # (B,n,M,N)
    return torch.where(_own_mask(n, N, j0).view(1, n, 1, N), own.unsqueeze(-1), oth) + eps


def calc_loss_rows(S, j0, eps=SMALL_ERR, variant="softmax"):
    """S (B,n,M,N) -> (loss (B), per (B,n,M)).  softmax: oracle._softmax_rows (unstabilised, as the reference);
    contrast: oracle._contrast_rows with the max taken on S (sigmoid is monotonic; closed_form does the same).  With one
    speaker eq. 7 has no other column to take a maximum over: that term is absent (0), not -inf."""
    B, n, M, N = S.shape
    own = (j0 + torch.arange(n)).view(1, n, 1, 1).expand(B, n, M, 1)
    pos = S.gather(3, own).squeeze(3)
    if variant == "softmax":
        per = (torch.exp(S).sum(dim=3) + eps).log() - pos
    elif variant == "contrast":
        per = 1.0 - torch.sigmoid(pos)
        if N > 1:
            best = S.masked_fill(_own_mask(n, N, j0).view(1, n, 1, N), float("-inf")).max(dim=3).values
            per = per + torch.sigmoid(best)
    else:
        raise ValueError(variant)
    return per.sum(dim=(1, 2)), per


def centroids(E):
    """(B,N,M,D) -> (B,N,D): oracle.centroids per batch."""
    return E.mean(dim=2)


def utterance_centroids(E):
    """(B,N,M,D) -> (B,N,M,D): oracle._leave_one_out_centroids per batch."""
    return (E.sum(dim=2, keepdim=True) - E) / (E.shape[2] - 1)


def scale_grads(dE, dw, db, g):
    """numpy: g (1) or (B).  gE in fp32 exactly as one multiply per element gives it, gw / gb and their scale in fp64."""
    gv = np.broadcast_to(np.asarray(g, np.float32).reshape(-1), (dE.shape[0],))
    gE = dE.astype(np.float32) * gv.reshape(-1, *([1] * (dE.ndim - 1)))
    tw, tb = dw.astype(np.float64) * gv, db.astype(np.float64) * gv
    return gE, tw.sum(), tb.sum(), np.abs(tw).sum(), np.abs(tb).sum()


# ---- numpy in, numpy out: values and autograd gradients, chunked over the (independent) batches --------------------------
def _t(x, dtype, grad=False):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).clone().requires_grad_(grad)


def cos_rows_np(E, C, j0, g_cos=None, eps=SMALL_ERR, eps_cos=EPS_COS, dtype=torch.float64, chunk_bytes=1 << 28):
    """-> dict cos [, dE, dC (this slice's PARTIAL centroid gradient)] for incoming gradient g_cos."""
    B, n, M, D = E.shape
    N = C.shape[1]
    step = max(1, int(chunk_bytes // (8 * n * M * N * D)))
    out = {"cos": [], "dE": [], "dC": []}
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        e, c = _t(E[sl], dtype, g_cos is not None), _t(C[sl], dtype, g_cos is not None)
        cos = cos_rows(e, c, j0, eps, eps_cos)
        out["cos"].append(cos.detach().numpy())
        if g_cos is not None:
            cos.backward(_t(g_cos[sl], dtype))
            out["dE"].append(e.grad.numpy())
            out["dC"].append(c.grad.numpy())
    return {k: np.concatenate(v) for k, v in out.items() if v}


def calc_loss_rows_np(S, j0, eps, variant, g_loss=None, g_per=None, dtype=torch.float64):
    """-> dict loss, per [, dS for the incoming gradients g_loss (B) and / or g_per (B,n,M)]."""
    need = g_loss is not None or g_per is not None
    s = _t(S, dtype, need)
    with np.errstate(all="ignore"):
        loss, per = calc_loss_rows(s, j0, eps, variant)
    out = {"loss": loss.detach().numpy(), "per": per.detach().numpy()}
    if need:
        tot = 0.0
        if g_loss is not None:
            tot = tot + (loss * _t(g_loss, dtype)).sum()
        if g_per is not None:
            tot = tot + (per * _t(g_per, dtype)).sum()
        tot.backward()
        out["dS"] = s.grad.numpy()
    return out


# ---- the cases of tests/test_gpu_helpers.py ----------------------------------------------------------------------------
# (B, N, M, D, n, j0): B in {1, 3}; D in {1, 3, 63, 64, 65, 200, 1030}; N in {1, 2, 63, 64, 65, 130}; M = 2 and M = 17;
# slices: whole (N, 0), first (1, 0), last (1, N - 1), tail (n, N - n), middle -- several of them inside and across the
# last 64-column stripe of N = 130.
COS_CASES = [
    (1, 1, 2, 1, 1, 0), (3, 1, 2, 63, 1, 0), (3, 2, 2, 3, 2, 0), (3, 2, 17, 3, 1, 1), (1, 63, 2, 63, 63, 0),
    (1, 63, 2, 1, 63, 0), (3, 64, 2, 64, 1, 0), (1, 64, 17, 64, 64, 0), (1, 65, 17, 65, 20, 45), (3, 65, 2, 200, 7, 30),
    (1, 130, 2, 64, 130, 0), (3, 130, 2, 65, 1, 129), (1, 130, 3, 200, 5, 125), (1, 130, 2, 3, 40, 50),
    (1, 2, 2, 1030, 2, 0), (3, 5, 17, 1030, 2, 2), (1, 65, 2, 1, 3, 62),
]


def cos_inputs(case, seed=0):
    """Rows of mixed norms (0.5 .. 1.5), centroids that are NOT the mean of E, an incoming gradient of both signs."""
    B, N, M, D, n, j0 = case
    rng = np.random.default_rng(1000 + 7 * sum(case) + seed)
    E = (rng.standard_normal((B, n, M, D)) * rng.uniform(0.5, 1.5, (B, n, M, 1))).astype(np.float32)
    C = (rng.standard_normal((B, N, D)) * rng.uniform(0.3, 2.0, (B, N, 1))).astype(np.float32)
    g = rng.standard_normal((B, n, M, N)).astype(np.float32)
    return E, C, g


def degenerate_inputs(kind):
    """(E (1,N,M,D), C (1,N,D), g): one degenerate vector each, the rest ordinary.  N 3, D 8."""
    rng = np.random.default_rng(77)
    N, M, D = 3, 3, 8
    E = rng.standard_normal((1, N, M, D)).astype(np.float32)
    C = rng.standard_normal((1, N, D)).astype(np.float32)
    if kind == "zero_row":
        E[0, 1, 1] = 0.0
    elif kind == "zero_centroid":
        C[0, 2] = 0.0
    elif kind == "tiny_row":                          # 0 < |e| < eps_cos, squares still normal fp32 numbers
        E[0, 0, 2] = (rng.standard_normal(D) * 1e-9).astype(np.float32)
    elif kind == "tiny_centroid":
        C[0, 1] = (rng.standard_normal(D) * 1e-9).astype(np.float32)
    elif kind == "identical_rows":                    # the leave-one-out centroid of every row is the row itself
        E[0, 1, :] = E[0, 1, 0]
    elif kind == "loo_zero":                          # rows x, y, -y: the leave-one-out centroid of the first is exactly 0
        # (multiples of 1/64: x + y - y is x in fp32 in ANY summation order, so the centroid is 0 in the kernel too, not
        # a rounding residue of norm ~1e-8 whose direction is noise)
        E[0, 2] = np.round(E[0, 2] * 64.0) / 64.0
        E[0, 2, 2] = -E[0, 2, 1]
    else:
        raise ValueError(kind)
    g = rng.standard_normal((1, N, M, N)).astype(np.float32)
    return E, C, g


DEGENERATE = ["zero_row", "zero_centroid", "tiny_row", "tiny_centroid", "identical_rows", "loo_zero"]

# (B, N, M, n, j0, variant, eps, shift, incoming): N in {1, 2, 64, 65, 130}; n M above, at and below one wave;
# incoming gradient on the loss only, on the rows only, on both -- always non-uniform.
LOSS_CASES = [
    (3, 1, 17, 1, 0, "softmax", 1e-6, 0.0, "both"), (3, 1, 3, 1, 0, "softmax", 0.0, 0.0, "loss"),
    (3, 1, 3, 1, 0, "contrast", 1e-6, 0.0, "both"),
    (3, 2, 2, 2, 0, "softmax", 1e-6, 0.0, "per"), (3, 2, 17, 1, 1, "contrast", 1e-6, 0.0, "both"),
    (1, 64, 2, 64, 0, "softmax", 0.0, 0.0, "both"), (3, 64, 2, 32, 32, "softmax", 1e-6, 80.0, "loss"),
    (1, 64, 17, 5, 20, "contrast", 1e-6, 0.0, "per"), (3, 65, 2, 65, 0, "softmax", 1e-6, -80.0, "both"),
    (1, 65, 3, 1, 64, "softmax", 0.0, -80.0, "per"), (1, 65, 2, 65, 0, "contrast", 0.0, 0.0, "loss"),
    (3, 130, 2, 130, 0, "softmax", 1e-6, 0.0, "both"), (1, 130, 3, 4, 126, "softmax", 0.0, 80.0, "both"),
    (3, 130, 2, 1, 129, "contrast", 1e-6, 0.0, "both"), (1, 130, 2, 40, 50, "contrast", 1e-6, 0.0, "loss"),
    (1, 130, 17, 130, 0, "softmax", 1e-6, 0.0, "per"),
    # every entry below log(eps) - 88: without the log(eps) floor of the max-shift, exp(log_eps - mx) overflows fp32 and the
    # forward's log z is inf (a shift of -80 does not reach that: there the floor only rescales z).  In the backward the
    # overflow gives p = 0 where the true p is below 1e-38, so dropping the floor THERE changes no fp32 result.
    (3, 64, 2, 64, 0, "softmax", 1e-6, -120.0, "both"), (1, 130, 3, 4, 126, "softmax", 1e-6, -120.0, "per"),
]


def loss_inputs(case, seed=0):
    B, N, M, n, j0, variant, eps, shift, incoming = case
    rng = np.random.default_rng(2000 + B + 3 * N + 5 * M + 7 * n + 11 * j0 + seed)
    S = (rng.standard_normal((B, n, M, N)) * 3.0 + shift).astype(np.float32)
    gl = rng.standard_normal(B).astype(np.float32) if incoming in ("loss", "both") else None
    gp = rng.standard_normal((B, n, M)).astype(np.float32) if incoming in ("per", "both") else None
    return S, gl, gp


def tie_inputs():
    """contrast, N 6, whole batch: in every row the two largest OTHER-speaker entries are bit-equal."""
    rng = np.random.default_rng(5)
    B, N, M = 2, 6, 3
    S = (rng.standard_normal((B, N, M, N)) * 2.0).astype(np.float32)
    pairs = np.zeros((B, N, M, 2), dtype=np.int64)
    for b in range(B):
        for j in range(N):
            for i in range(M):
                others = [k for k in range(N) if k != j]
                k1, k2 = rng.choice(others, size=2, replace=False)
                S[b, j, i, k1] = S[b, j, i, k2] = np.float32(np.abs(S[b, j, i]).max() + 0.5)
                pairs[b, j, i] = (k1, k2)
    gl = rng.standard_normal(B).astype(np.float32)
    gp = rng.standard_normal((B, N, M)).astype(np.float32)
    return S, gl, gp, pairs
