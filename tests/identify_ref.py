"""Identification restated in numpy (a plain helper module, no fixtures, no GPU; never the code under test): ge2e_identify's
lists, ranks and histogram from a score matrix.

Candidates of a scored row are the enrolled columns (cnt > 0) only.  The order is total: a stands before b iff
score_a > score_b; -0 and +0 are equal; a NaN stands behind every number; where the scores are equal, or both NaN, the lower
index stands first.  idx (R, k): the first k candidates, -1 past the enrolled count and on ignored rows (label < 0); score
(R, k): their scores in the matrix's dtype, -inf where idx is -1; rank (R,): the target's position, k when the row has a
target outside the list, -1 without target or on an ignored row; hist (k + 1,): rows per rank.
"""
import numpy as np

import enroll_ref as er


def order_of(row, enrolled):
    """The enrolled columns of one score row in the total order."""
    cols = np.flatnonzero(enrolled)
    s = np.asarray(row)[cols].astype(np.float64)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s) + 0.0             # -0.0 + 0.0 = +0.0: the two zeros are one value
    return cols[np.lexsort((cols, neg, nan))]      # (the last key is the primary one: NaN to the end, behind -inf too)


def topk_ref(scores, labels, cnt, k):
    """-> idx (R, k) int32, score (R, k) in scores' dtype, rank (R,) int32, hist (k + 1,) int64."""
    scores = np.asarray(scores)
    R = len(scores)
    scored, target, enrolled = er.classes(labels, cnt, R)
    idx = np.full((R, k), -1, dtype=np.int32)
    score = np.full((R, k), -np.inf, dtype=scores.dtype)
    rank = np.full(R, -1, dtype=np.int32)
    hist = np.zeros(k + 1, dtype=np.int64)
    for r in np.flatnonzero(scored):
        first = order_of(scores[r], enrolled)[:k]
        idx[r, :len(first)] = first
        score[r, :len(first)] = scores[r, first]
        if target[r] >= 0:
            at = np.flatnonzero(first == target[r])
            rank[r] = at[0] if len(at) else k
            hist[rank[r]] += 1
    return idx, score, rank, hist


def decided(scores, labels, cnt, margin):
    """(R,) bool: the rows with a target whose target's score keeps at least `margin` from every other enrolled speaker's."""
    scores = np.asarray(scores, dtype=np.float64)
    _, target, enrolled = er.classes(labels, cnt, len(scores))
    out = np.zeros(len(scores), dtype=bool)
    for r in np.flatnonzero(target >= 0):
        others = enrolled.copy()
        others[target[r]] = False
        gap = np.abs(scores[r, others] - scores[r, target[r]])
        out[r] = (not gap.size) or gap.min() >= margin
    return out


def hist_of(rank, rows, k):
    """The histogram of rank over `rows` (bool), rows without a target left out."""
    r = np.asarray(rank)[rows]
    return np.bincount(r[r >= 0], minlength=k + 1).astype(np.int64)
