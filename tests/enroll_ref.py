"""Enrolment and verification restated in numpy float64 (a plain helper module, no fixtures, no GPU; never the code under
test): ge2e_enroll_accumulate, ge2e_enroll_finalize, ge2e_verify_scores and its counts.

A bank is sums (K, D) and cnt (K,).  A row is enrolled iff 0 <= label < K; a speaker is enrolled iff cnt > 0.  A trial row
with a negative label is ignored, every other row is scored; its target is its label if that is an enrolled speaker, and
it has none otherwise.  No leave-one-out anywhere: a trial row is no part of the model it is scored against.
    model_k      = c_k / max(|c_k|, eps_cos),  c_k = sums_k / cnt_k
    scores[r, k] = e_r . model_k / max(|e_r|, eps_cos) + eps    (k enrolled),  0 otherwise
"""
import numpy as np

EPS, EPS_COS = 1e-6, 1e-8


def valid_rows(labels, K):
    labels = np.asarray(labels, dtype=np.int64)
    return (labels >= 0) & (labels < K)


def accumulate_ref(sums, cnt, E, labels, dtype=np.float64):
    """One ge2e_enroll_accumulate call -> (sums, cnt), new arrays.  A speaker's partial sum starts from 0 and adds its rows
    in ascending row index, one after the other in `dtype`; then sums[s] = sums[s] + partial.  A speaker without a valid
    row keeps its row of sums untouched (NaN included); the ignored rows of E are never looked at."""
    sums = np.array(sums, dtype=dtype)
    cnt = np.array(cnt, dtype=np.int64)
    K = len(cnt)
    labels = np.asarray(labels, dtype=np.int64)
    ok = valid_rows(labels, K)
    for s in np.unique(labels[ok]):
        rows = np.flatnonzero(ok & (labels == s))
        part = np.zeros(sums.shape[1], dtype=dtype)
        for r in rows:
            part = part + np.asarray(E[r]).astype(dtype)
        sums[s] = sums[s] + part
        cnt[s] += len(rows)
    return sums, cnt


def sums_bound(calls, K, D):
    """(m - 1) 2^-24 sum_i |e_i[d]| per element over every valid row of every call: the first-order bound of any
    fixed-order fp32 summation of a speaker's m rows."""
    m = np.zeros(K)
    mag = np.zeros((K, D))
    for E, labels in calls:
        labels = np.asarray(labels, dtype=np.int64)
        ok = valid_rows(labels, K)
        np.add.at(m, labels[ok], 1)
        np.add.at(mag, labels[ok], np.abs(np.asarray(E)[ok].astype(np.float64)))
    return np.maximum(m - 1, 0)[:, None] * 2.0 ** -24 * mag


def finalize_ref(sums, cnt, eps_cos=EPS_COS):
    """-> models (K, D) float64; rows with cnt <= 0 are 0 and their sums are never looked at."""
    cnt = np.asarray(cnt)
    models = np.zeros(np.shape(sums))
    for s in np.flatnonzero(cnt > 0):
        c = np.asarray(sums[s], dtype=np.float64) / cnt[s]
        models[s] = c / max(np.sqrt((c * c).sum()), eps_cos)
    return models


def classes(labels, cnt, R):
    """-> scored (R,) bool, target (R,) int64 (-1: none), enrolled (K,) bool.  labels None: every row scored, no targets."""
    enrolled = np.asarray(cnt) > 0
    K = len(enrolled)
    if labels is None:
        return np.ones(R, dtype=bool), np.full(R, -1, dtype=np.int64), enrolled
    labels = np.asarray(labels, dtype=np.int64)
    scored = labels >= 0
    inside = scored & (labels < K)
    target = np.where(inside & enrolled[np.clip(labels, 0, K - 1)], labels, -1)
    return scored, target, enrolled


def scores_ref(E, labels, models, cnt, eps=EPS, eps_cos=EPS_COS):
    """-> scores (R, K) float64; the ignored rows are never looked at (they may hold NaN)."""
    E = np.asarray(E)
    scored, _, enrolled = classes(labels, cnt, len(E))
    out = np.zeros((len(E), len(enrolled)))
    X = E[scored].astype(np.float64)
    norm = np.maximum(np.sqrt((X * X).sum(-1)), eps_cos)
    s = X @ np.asarray(models, dtype=np.float64)[enrolled].T / norm[:, None] + eps
    block = np.zeros((len(X), len(enrolled)))
    block[:, enrolled] = s
    out[scored] = block
    return out


def counted(labels, cnt, R):
    """-> imp (R, K) bool: the impostor entries, tgt (R, K) bool: the target entries."""
    scored, target, enrolled = classes(labels, cnt, R)
    K = len(enrolled)
    own = np.zeros((R, K), dtype=bool)
    has = target >= 0
    own[np.flatnonzero(has), target[has]] = True
    base = scored[:, None] & enrolled[None, :]
    return base & ~own, base & own


def counts_ref(scores, labels, cnt, thr):
    """The sweep on scores (R, K) with numpy's fp32 `>` -> counts (T, 2) int64, trials (2,) int64.  NaN accepts nothing and
    is tallied in trials all the same."""
    s = np.asarray(scores).astype(np.float32)
    imp, tgt = counted(labels, cnt, len(s))
    thr = np.asarray(thr, dtype=np.float64).astype(np.float32)
    out = np.zeros((len(thr), 2), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t, th in enumerate(thr):
            acc = s > th
            out[t, 0] = int((acc & imp).sum())
            out[t, 1] = int((acc & tgt).sum())
    return out, np.array([imp.sum(), tgt.sum()], dtype=np.int64)


def margin(scores, labels, cnt, thr):
    """The smallest distance of a counted score from any threshold."""
    imp, tgt = counted(labels, cnt, len(scores))
    s = np.asarray(scores)[imp | tgt]
    if not s.size:
        return np.inf
    thr = np.asarray(thr, dtype=np.float64).astype(np.float32).astype(np.float64)
    return float(np.abs(s[:, None] - thr[None, :]).min())
