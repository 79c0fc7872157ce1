"""The ragged GE2E loss restated with torch autograd in float64 (a plain helper module, no fixtures, no GPU).

One batch: E (R, D) holds the rows of speaker j contiguously, `counts[j]` of them (>= 2).
    c_k      = mean of speaker k's rows                                   (s3:34-38 with M -> m_k)
    u_r      = (sum_j - e_r) / (m_j - 1)          r a row of speaker j    (s3:95-112)
    cos[r,k] = cossim(e_r, c_k) for k != j, cossim(e_r, u_r) for k = j, both with eps_cos, + eps on every entry
    S        = w cos + b
    softmax  per_r = -S[r,j] + log(sum_k exp S[r,k] + eps)
    contrast per_r = 1 - sigmoid(S[r,j]) + max_{k != j} sigmoid(S[r,k])    (the max term is 0 when N = 1)
    loss     = sum_r per_r
Per-speaker slices and F.cosine_similarity; the gradients are autograd's.  With all counts equal to M this is the dense
loss: tests/test_ragged_cpu.py holds it to oracle.closed_form there.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS, EPS_COS = 1e-6, 1e-8


def ragged_loss(E, counts, w=10.0, b=-5.0, eps=EPS, eps_cos=EPS_COS, variant="softmax", dtype=torch.float64):
    """numpy E (R, D), counts (N,) -> dict of float64 numpy: loss (), per (R,), dE (R, D), dw (), db ().
    `dtype`: the type the formulas are evaluated in; float64 is the reference, float32 only a yardstick of what plain
    fp32 arithmetic gives on an input (tests/test_gpu_rowlist_fuzz.py)."""
    counts = [int(c) for c in counts]
    n = len(counts)
    e = torch.as_tensor(np.ascontiguousarray(E), dtype=dtype).clone().requires_grad_(True)
    assert e.dim() == 2 and sum(counts) == e.shape[0] and min(counts) >= 2
    wt = torch.tensor(float(w), dtype=dtype, requires_grad=True)
    bt = torch.tensor(float(b), dtype=dtype, requires_grad=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    rows = [e[off[j]:off[j + 1]] for j in range(n)]
    sums = [r.sum(dim=0) for r in rows]
    cent = torch.stack([sums[j] / counts[j] for j in range(n)])                              # (N, D)
    loo = torch.cat([(sums[j].unsqueeze(0) - rows[j]) / (counts[j] - 1) for j in range(n)])   # (R, D)
    spk = torch.as_tensor(np.repeat(np.arange(n), counts))
    own = torch.zeros(e.shape[0], n, dtype=torch.bool)
    own[torch.arange(e.shape[0]), spk] = True
    cos = F.cosine_similarity(e.unsqueeze(1), cent.unsqueeze(0), dim=2, eps=eps_cos)         # (R, N)
    cos_own = F.cosine_similarity(e, loo, dim=1, eps=eps_cos)                                 # (R,)
    cos = torch.where(own, cos_own.unsqueeze(1), cos) + eps
    sim = wt * cos + bt
    pos = sim[own]
    if variant == "softmax":
        # log(sum_k exp S_k + eps), written so that large |S| cannot overflow: the same number
        lse = torch.logsumexp(sim, dim=1)
        if eps > 0:
            lse = torch.logaddexp(lse, torch.full_like(lse, math.log(eps)))
        per = lse - pos
    elif variant == "contrast":
        sig = torch.sigmoid(sim)
        neg = sig.masked_fill(own, float("-inf")).max(dim=1).values if n > 1 else torch.zeros_like(pos)
        per = 1.0 - torch.sigmoid(pos) + neg
    else:
        raise ValueError(variant)
    loss = per.sum()
    loss.backward()
    f64 = lambda t: t.detach().numpy().astype(np.float64)  # noqa: E731  (a copy)
    return {"loss": f64(loss), "per": f64(per), "dE": f64(e.grad), "dw": f64(wt.grad), "db": f64(bt.grad)}


def ragged_inputs(counts, D, seed):
    """Unit rows centre[speaker] + 0.5 * noise, float32 (R, D)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    centre = rng.standard_normal((len(counts), D))
    x = centre[np.repeat(np.arange(len(counts)), counts)] + 0.5 * rng.standard_normal((int(counts.sum()), D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32)
