"""The masked labelled GE2E loss restated in numpy on top of tests/ragged_ref.py (a plain helper module, no fixtures, no GPU).

One batch: labels (R,) of ANY integers and the bound N.
    valid row       0 <= labels[r] < N                               (nothing is clamped)
    active speaker  at least 2 valid rows carry its label
    active row      valid, and its speaker is active;  n_act / r_act count the active speakers / rows
    order    (R,)   the active rows sorted by (label, index), then every other row by index
                    = argsort(where(active_row, labels, N), kind="stable")
    offsets  (N+1,) offsets[k] = active rows of the active speakers before the k-th (ascending label), k <= n_act; r_act beyond
    speakers (N,)   the label of the k-th active speaker, k < n_act; -1 beyond
    active   (2,)   n_act, r_act
    loss            ragged_ref.ragged_loss of the n_act speakers on E[order[:r_act]]; per and dE scattered back to the
                    caller's rows and 0 on every other row; all zero when n_act = 0 (defined here, not by ragged_ref)
"""
import numpy as np
import torch

import ragged_ref as rr


def index_ref(labels, N):
    """labels (R,) -> dict of offsets (N+1,), order (R,), speakers (N,), active (2,) int32, and active_row (R,) bool,
    counts (n_act,)."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    N = int(N)
    valid = (labels >= 0) & (labels < N)
    hist = np.bincount(labels[valid], minlength=N)
    spk_active = hist >= 2
    active_row = valid.copy()
    active_row[valid] = spk_active[labels[valid]]
    order = np.argsort(np.where(active_row, labels, N), kind="stable")
    ids = np.flatnonzero(spk_active)
    n_act, r_act = len(ids), int(active_row.sum())
    offsets = np.full(N + 1, r_act, dtype=np.int64)
    offsets[:n_act + 1] = np.concatenate([[0], np.cumsum(hist[ids])])
    speakers = np.full(N, -1, dtype=np.int64)
    speakers[:n_act] = ids
    return {"offsets": offsets.astype(np.int32), "order": order.astype(np.int32), "speakers": speakers.astype(np.int32),
            "active": np.array([n_act, r_act], dtype=np.int32), "active_row": active_row, "counts": hist[ids].astype(np.int64)}


def index_ref_batched(labels, N):
    """labels (B, R) -> offsets (B, N+1), order (B, R), speakers (B, N), active (B, 2)."""
    refs = [index_ref(row, N) for row in np.asarray(labels)]
    return {k: np.stack([r[k] for r in refs]) for k in ("offsets", "order", "speakers", "active")}


def masked_loss(E, labels, N, w=10.0, b=-5.0, eps=rr.EPS, eps_cos=rr.EPS_COS, variant="softmax", dtype=torch.float64):
    """numpy E (R, D), labels (R,), bound N -> dict of float64 numpy: loss (), per (R,), dE (R, D), dw (), db () in the caller's
    row order, and the index reference under "index".  The rows that are not active are never looked at.  `dtype`: see
    ragged_ref.ragged_loss."""
    E = np.asarray(E)
    idx = index_ref(labels, N)
    n_act, r_act = (int(v) for v in idx["active"])
    R, D = E.shape
    out = {"loss": np.zeros(()), "per": np.zeros(R), "dE": np.zeros((R, D)), "dw": np.zeros(()), "db": np.zeros(()),
           "index": idx}
    if n_act == 0:
        return out
    rows = idx["order"][:r_act]
    ref = rr.ragged_loss(E[rows], idx["counts"], w, b, eps=eps, eps_cos=eps_cos, variant=variant, dtype=dtype)
    out["loss"], out["dw"], out["db"] = ref["loss"], ref["dw"], ref["db"]
    out["per"][rows] = ref["per"]
    out["dE"][rows] = ref["dE"]
    return out
