"""The labelled evaluation call restated in numpy float64 on top of tests/masked_ref.index_ref (a plain helper module, no
fixtures, no GPU; never the code under test).

One batch: E (R, D), labels (R,) of ANY integers, the bound N.  With masked_ref's valid / active rows and speakers and the
active speakers numbered 0 .. n_act-1 by ascending label, for an active row r of compact speaker j and k < n_act
    c_k      = mean of the active rows of speaker k
    u_r      = (sum_j - e_r) / (m_j - 1)
    cos[r,k] = cossim(e_r, c_k) + eps  (k != j),   cos[r,j] = cossim(e_r, u_r) + eps
cossim(x, y) = x . y / (max(|x|, eps_cos) max(|y|, eps_cos)), F.cosine_similarity's clamp.  This is ragged_ref's `cos` on
the compacted batch, scattered back to the caller's rows; 0 on every row that is not active and every column >= n_act.
"""
import numpy as np

import masked_ref as mr

EPS, EPS_COS = 1e-6, 1e-8


def cossim(x, y, eps_cos=EPS_COS):
    """Row-wise over the last axis, float64."""
    nx = np.maximum(np.sqrt((x * x).sum(-1)), eps_cos)
    ny = np.maximum(np.sqrt((y * y).sum(-1)), eps_cos)
    return (x * y).sum(-1) / (nx * ny)


def cos_ref(E, labels, N, eps=EPS, eps_cos=EPS_COS):
    """E (R, D), labels (R,), bound N -> cos (R, N) float64, col (R,), speakers (N,), active (2,) int32.  The rows that are
    not active are never looked at (they may hold NaN)."""
    E = np.asarray(E)
    idx = mr.index_ref(labels, N)
    n_act, r_act = (int(v) for v in idx["active"])
    R = E.shape[0]
    cos = np.zeros((R, int(N)))
    col = np.full(R, -1, dtype=np.int32)
    if n_act:
        rows = idx["order"][:r_act]
        X = E[rows].astype(np.float64)
        counts = idx["counts"]
        spk = np.repeat(np.arange(n_act), counts)
        sums = np.zeros((n_act, E.shape[1]))
        np.add.at(sums, spk, X)
        cent = sums / counts[:, None]
        c = cossim(X[:, None, :], cent[None, :, :], eps_cos)                         # (r_act, n_act)
        loo = (sums[spk] - X) / (counts[spk] - 1)[:, None]
        c[np.arange(r_act), spk] = cossim(X, loo, eps_cos)
        cos[rows, :n_act] = c + eps
        col[rows] = spk
    return cos, col, idx["speakers"], idx["active"]


def counts_ref(sim, col, n_act, thr):
    """The calculate_ERR sweep on sim (R, N): counts (T, 2) int64 over the rows with col >= 0 and the columns < n_act,
    [t][0] = #{(r,k), k != col[r] : sim[r][k] > thr[t]}, [t][1] = #{r : sim[r][col[r]] > thr[t]}; numpy's fp32 `>`."""
    sim = np.asarray(sim).astype(np.float32)
    col = np.asarray(col)
    thr = np.asarray(thr, dtype=np.float64).astype(np.float32)
    rows = np.flatnonzero(col >= 0)
    s = sim[rows][:, :int(n_act)]
    own = np.zeros(s.shape, dtype=bool)
    own[np.arange(len(rows)), col[rows]] = True
    out = np.zeros((len(thr), 2), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t, th in enumerate(thr):
            acc = s > th
            out[t, 0] = int((acc & ~own).sum())
            out[t, 1] = int((acc & own).sum())
    return out


def margin(cos, col, n_act, thr):
    """The smallest distance of a counted entry of cos from any threshold."""
    rows = np.flatnonzero(np.asarray(col) >= 0)
    if not len(rows) or not n_act:
        return np.inf
    s = np.asarray(cos)[rows][:, :int(n_act)]
    thr = np.asarray(thr, dtype=np.float64).astype(np.float32).astype(np.float64)
    return float(np.abs(s[..., None] - thr).min())
