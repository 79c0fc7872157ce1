"""The differentiable labelled helpers restated with torch autograd in float64 on the CPU (a plain helper module, no
fixtures, no GPU; never the code under test).

One batch: E (R, D), labels (R,) of ANY integers, the bound N.  On tests/masked_ref.index_ref's active rows and speakers
(compact ids 0 .. n_act-1 by ascending label), with per-speaker slices and F.cosine_similarity as in tests/ragged_ref.py:
    c_k      = mean of the active rows of speaker k
    u_r      = (sum_j - e_r) / (m_j - 1)
    cos[r,k] = cossim(e_r, c_k) + eps  (k != j),   cos[r,j] = cossim(e_r, u_r) + eps          (R, N), 0 where nothing counts
and calc_loss_labeled on a caller-made sim (R, N) with col (R,) and n_act: ragged_ref.ragged_loss's two formulas
    softmax  per_r = -sim[r,j] + log(sum_{k < n_act} exp sim[r,k] + eps)
    contrast per_r = 1 - sigmoid(sim[r,j]) + max_{k != j} sigmoid(sim[r,k])   (0 when n_act = 1; torch.max: the first of a tie)
over the rows with 0 <= col < n_act; loss = sum of per.  The rows and columns that do not count are never looked at: they
may hold NaN, and every gradient is 0 there.  Gradients are autograd's.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import masked_ref as mr

EPS, EPS_COS = 1e-6, 1e-8


def cos_graph(E, labels, N, eps=EPS, eps_cos=EPS_COS, dtype=torch.float64):
    """-> (x, cos, idx, col): x (r_act, D) the leaf tensor of the active rows in sorted order (None when nothing counts), cos
    (R, N) built on it, masked_ref's index, col (R,) int32."""
    E = np.asarray(E)
    idx = mr.index_ref(labels, N)
    n_act, r_act = (int(v) for v in idx["active"])
    R = E.shape[0]
    col = np.full(R, -1, dtype=np.int32)
    if n_act == 0:
        return None, torch.zeros(R, int(N), dtype=dtype), idx, col
    rows = idx["order"][:r_act].astype(np.int64)
    counts = [int(c) for c in idx["counts"]]
    x = torch.as_tensor(np.ascontiguousarray(E[rows]), dtype=dtype).clone().requires_grad_(True)
    off = np.concatenate([[0], np.cumsum(counts)])
    parts = [x[off[j]:off[j + 1]] for j in range(n_act)]
    sums = [p.sum(dim=0) for p in parts]
    cent = torch.stack([sums[j] / counts[j] for j in range(n_act)])
    loo = torch.cat([(sums[j].unsqueeze(0) - parts[j]) / (counts[j] - 1) for j in range(n_act)])
    spk = np.repeat(np.arange(n_act), counts)
    own = torch.zeros(r_act, n_act, dtype=torch.bool)
    own[torch.arange(r_act), torch.as_tensor(spk)] = True
    c = F.cosine_similarity(x.unsqueeze(1), cent.unsqueeze(0), dim=2, eps=eps_cos)
    c_own = F.cosine_similarity(x, loo, dim=1, eps=eps_cos)
    c = torch.where(own, c_own.unsqueeze(1), c) + eps
    block = torch.zeros(r_act, int(N), dtype=dtype)
    block = torch.cat([c, block[:, n_act:]], dim=1)
    cos = torch.zeros(R, int(N), dtype=dtype).index_put((torch.as_tensor(rows),), block)
    col[rows] = spk
    return x, cos, idx, col


def scatter_rows(x, idx, shape):
    """The gradient of cos_graph's leaf, back in the caller's row order: 0 on every row that is not active."""
    out = np.zeros(shape)
    if x is not None and x.grad is not None:
        r_act = int(idx["active"][1])
        out[idx["order"][:r_act]] = x.grad.numpy()
    return out


def counted(col, n_act, N):
    """(R, N) bool: the entries of a (R, N) matrix that count."""
    col = np.asarray(col)
    m = np.zeros((len(col), int(N)), dtype=bool)
    m[(col >= 0) & (col < int(n_act)), :int(n_act)] = True
    return m


def cos_bwd(E, labels, N, g_cos, eps=EPS, eps_cos=EPS_COS):
    """dL/dE (R, D) float64 for L = sum over the counted entries of g_cos * cos; g_cos (R, N) may hold anything elsewhere."""
    x, cos, idx, col = cos_graph(E, labels, N, eps, eps_cos)
    E = np.asarray(E)
    if x is None:
        return np.zeros(E.shape)
    m = counted(col, idx["active"][0], N)
    g = torch.as_tensor(np.where(m, np.asarray(g_cos, dtype=np.float64), 0.0))
    (cos * g).sum().backward()
    return scatter_rows(x, idx, E.shape)


def calc_loss_labeled(sim, col, n_act, eps=EPS, variant="softmax"):
    """torch sim (R, N), col (R,), n_act -> (loss (), per (R,)) torch, differentiable in sim."""
    col = np.asarray(col).astype(np.int64)
    N = sim.shape[1]
    n_act = min(max(int(n_act), 0), N)
    R = sim.shape[0]
    rows = np.flatnonzero((col >= 0) & (col < n_act))
    per = torch.zeros(R, dtype=sim.dtype)
    if len(rows) == 0:
        return per.sum(), per
    s = sim[torch.as_tensor(rows)][:, :n_act]
    own = torch.zeros(len(rows), n_act, dtype=torch.bool)
    own[torch.arange(len(rows)), torch.as_tensor(col[rows])] = True
    pos = s[own]
    if variant == "softmax":
        lse = torch.logsumexp(s, dim=1)
        if eps > 0:
            lse = torch.logaddexp(lse, torch.full_like(lse, math.log(eps)))
        p = lse - pos
    elif variant == "contrast":
        sig = torch.sigmoid(s)
        neg = sig.masked_fill(own, float("-inf")).max(dim=1).values if n_act > 1 else torch.zeros_like(pos)
        p = 1.0 - torch.sigmoid(pos) + neg
    else:
        raise ValueError(variant)
    per = per.index_put((torch.as_tensor(rows),), p)
    return per.sum(), per


def calc_loss_ref(sim, col, n_act, eps=EPS, variant="softmax", g_loss=None, g_per=None, dtype=torch.float64):
    """numpy sim (R, N) -> dict of float64 numpy: loss (), per (R,), dS (R, N) = d(g_loss loss + sum g_per per) / d sim (a
    missing gradient counts as 0; entries of g_per on rows that do not count may hold anything).  `dtype`: float32 is only
    a yardstick of what plain fp32 arithmetic gives (as in ragged_ref.ragged_loss)."""
    sim = np.asarray(sim)
    col = np.asarray(col)
    N = sim.shape[1]
    n = min(max(int(n_act), 0), N)
    m = counted(col, n, N)
    s = torch.as_tensor(np.where(m, sim, 0.0), dtype=dtype).clone().requires_grad_(True)
    loss, per = calc_loss_labeled(s, col, n, eps, variant)
    row_ok = m.any(axis=1)
    gp = np.where(row_ok, np.zeros(len(col)) if g_per is None else np.asarray(g_per, dtype=np.float64), 0.0)
    total = float(0.0 if g_loss is None else g_loss) * loss + (per * torch.as_tensor(gp, dtype=dtype)).sum()
    if total.requires_grad:
        total.backward()
    dS = s.grad.numpy().astype(np.float64) if s.grad is not None else np.zeros(sim.shape)
    f64 = lambda t: t.detach().numpy().astype(np.float64)  # noqa: E731
    return {"loss": f64(loss), "per": f64(per), "dS": dS}


def composed(E, labels, N, w=10.0, b=-5.0, eps=EPS, eps_cos=EPS_COS, variant="softmax"):
    """Cosines, then w cos + b, then calc_loss_labeled: dict of float64 numpy loss (), per (R,), dE (R, D), dw (), db (), g_cos
    (R, N) = dL/dcos (0 where nothing counts), cos (R, N), col, active."""
    x, cos, idx, col = cos_graph(E, labels, N, eps, eps_cos)
    if cos.requires_grad:
        cos.retain_grad()
    wt = torch.tensor(float(w), dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(float(b), dtype=torch.float64, requires_grad=True)
    loss, per = calc_loss_labeled(wt * cos + bt, col, idx["active"][0], eps, variant)
    if loss.requires_grad:
        loss.backward()
    g = lambda t: np.zeros(()) if t.grad is None else t.grad.numpy().astype(np.float64)  # noqa: E731
    E = np.asarray(E)
    return {"loss": loss.detach().numpy().astype(np.float64), "per": per.detach().numpy().astype(np.float64),
            "dE": scatter_rows(x, idx, E.shape), "dw": g(wt), "db": g(bt),
            "g_cos": np.zeros(tuple(cos.shape)) if cos.grad is None else cos.grad.numpy().astype(np.float64),
            "cos": cos.detach().numpy().astype(np.float64), "col": col, "active": idx["active"], "index": idx}
