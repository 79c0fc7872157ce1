"""Score normalisation against a cohort restated in numpy (a plain helper module, no fixtures, no GPU; never the code under
test): ge2e_cohort_stats in float64 and ge2e_verify_scores_normed's expression, once in float64 and once in float32
operation by operation.

    stats[r]  = (mean, max(std, eps_std)) of the n = min(n_top, members) largest member scores of row r, NaN behind every
                number, std the population one from the deviations from that mean; (0, 1) for a row that is not scored and
                for n = 0.  Only the multiset of the n values enters: ties need no index rule.
    out[r, k] = 0.5 ((v - mu_k) (1 / sd_k) + (v - mu_r) (1 / sd_r))
"""
import numpy as np

EPS_STD = 1e-5


def top_values(values, n):
    """The n largest of a 1-d array as float64, descending, NaN behind every number (a stable sort: equal values keep
    their order, which the multiset does not see)."""
    v = np.asarray(values, dtype=np.float64)
    nan = np.isnan(v)
    num = v[~nan]
    num = num[np.argsort(-num, kind="stable")]
    return np.concatenate([num, v[nan]])[:n]


def cohort_stats_ref(scores, member, n_top, scored=None, eps_std=EPS_STD):
    """scores (R, C) of any float dtype, member (C,) bool, scored (R,) bool or None -> stats (R, 2) float64.  A row that is
    not scored is never looked at."""
    scores = np.asarray(scores)
    member = np.asarray(member, dtype=bool)
    R = len(scores)
    scored = np.ones(R, dtype=bool) if scored is None else np.asarray(scored, dtype=bool)
    out = np.tile(np.array([0.0, 1.0]), (R, 1))
    n = min(int(n_top), int(member.sum()))
    if n == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for r in np.flatnonzero(scored):
            top = top_values(scores[r, member], n)
            mean = top.sum() / n
            std = np.sqrt(((top - mean) ** 2).sum() / n)
            out[r] = mean, (eps_std if std < eps_std else std)    # (a NaN stays)
    return out


def cut_through_tie(scores, member, n_top):
    """(R,) bool: the n-th largest value of the row occurs more often among the members than it is taken."""
    scores = np.asarray(scores, dtype=np.float64)
    member = np.asarray(member, dtype=bool)
    n = min(int(n_top), int(member.sum()))
    out = np.zeros(len(scores), dtype=bool)
    for r in range(len(scores)):
        vals = scores[r, member]
        if n == 0 or np.isnan(vals).any():
            continue
        top = top_values(vals, n)
        out[r] = (vals == top[-1]).sum() > (top == top[-1]).sum()
    return out


def normed_f32(v, row_stats, model_stats, scored, enrolled):
    """The kernel's expression in numpy float32, every operation rounded on its own; +0 on rows that are not scored and on
    columns that are not enrolled, whose statistics are never looked at."""
    f = np.float32
    v = np.asarray(v, dtype=f)
    rs, ms = np.asarray(row_stats, dtype=f), np.asarray(model_stats, dtype=f)
    out = np.zeros(v.shape, dtype=f)
    rows, cols = np.flatnonzero(scored), np.flatnonzero(enrolled)
    if not len(rows) or not len(cols):
        return out
    with np.errstate(all="ignore"):
        x = v[np.ix_(rows, cols)]
        mu_k, rk = ms[cols, 0][None, :], (f(1) / ms[cols, 1])[None, :]
        mu_r, rr = rs[rows, 0][:, None], (f(1) / rs[rows, 1])[:, None]
        a = ((x - mu_k).astype(f) * rk).astype(f)
        b = ((x - mu_r).astype(f) * rr).astype(f)
        out[np.ix_(rows, cols)] = (f(0.5) * (a + b).astype(f)).astype(f)
    return out


def normed_f64(v, row_stats, model_stats, scored, enrolled):
    """The same in float64 with true divisions: the reference of the comparison against float64."""
    v = np.asarray(v, dtype=np.float64)
    rs, ms = np.asarray(row_stats, dtype=np.float64), np.asarray(model_stats, dtype=np.float64)
    out = np.zeros(v.shape)
    rows, cols = np.flatnonzero(scored), np.flatnonzero(enrolled)
    if len(rows) and len(cols):
        x = v[np.ix_(rows, cols)]
        out[np.ix_(rows, cols)] = 0.5 * ((x - ms[cols, 0][None, :]) / ms[cols, 1][None, :]
                                         + (x - rs[rows, 0][:, None]) / rs[rows, 1][:, None])
    return out


def normed_bound(v, row_stats, model_stats, scored, enrolled, g):
    """The first-order propagation of |score - ref| <= g and |mean - ref|, |std - ref| <= 2 g through the expression:
    0.5 sum over both sides [3 g / sd + 2 g |v - mu| / (sd (sd - 2 g))] + 1e-6 (1 + |out|), elementwise (R, K); inf where
    nothing is compared."""
    v = np.asarray(v, dtype=np.float64)
    rs, ms = np.asarray(row_stats, dtype=np.float64), np.asarray(model_stats, dtype=np.float64)
    out = np.full(v.shape, np.inf)
    rows, cols = np.flatnonzero(scored), np.flatnonzero(enrolled)
    if len(rows) and len(cols):
        x = v[np.ix_(rows, cols)]
        side = lambda mu, sd: 3 * g / sd + 2 * g * np.abs(x - mu) / (sd * (sd - 2 * g))  # noqa: E731
        ref = normed_f64(v, rs, ms, scored, enrolled)[np.ix_(rows, cols)]
        out[np.ix_(rows, cols)] = 0.5 * (side(ms[cols, 0][None, :], ms[cols, 1][None, :])
                                         + side(rs[rows, 0][:, None], rs[rows, 1][:, None])) + 1e-6 * (1 + np.abs(ref))
    return out
