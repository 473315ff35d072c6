"""References for the ensemble member distances (include/idiff.h, idiff_ensemble_distances), shared by the CPU and the GPU tests.

emulate(x, y): the contract in numpy float64: the valid mask over all M rows, the matrix of squared distances over the valid pixels (one
  float64 subtraction of the float32 values, squares added by numpy's pairwise sum: the kernel's order differs, which the GPU test's
  bound allows for), and the picks with the contract's scan order.
picks(d2, S, has_target): the picks from a finished matrix, math.sqrt and Python floats, added in index order: what the kernel's last
  launch does, operation for operation.
summary(d2, valid, S, has_target): the host summary restated from the definitions (numpy, all pairs at once), independent of
  driftSDE.ensemble_distance_summary's loops.
x is [S, n] and y is [n] or None; both float32 arrays."""
import math

import numpy as np


def rows_of(x, y):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x if y is None else np.concatenate([x, np.ascontiguousarray(y, dtype=np.float32)[None]], axis=0)


def picks(d2, S, has_target):
    """(medoid, best) from an [M, M] matrix: first strict minimum scanning from 0; best is -1 without a target"""
    d2 = [[float(v) for v in row] for row in np.asarray(d2, dtype=np.float64)]
    sums = []
    for i in range(S):
        m = 0.0
        for j in range(S):
            if j != i:
                m = m + math.sqrt(d2[i][j])
        sums.append(m)
    medoid = 0
    for i in range(1, S):
        if sums[i] < sums[medoid]:
            medoid = i
    best = -1
    if has_target:
        best = 0
        for i in range(1, S):
            if d2[i][S] < d2[best][S]:
                best = i
    return medoid, best


def emulate(x, y=None):
    """-> dict(valid [n] bool, d2 [M, M] f64, counts (valid, invalid), pick (medoid, best))"""
    r = rows_of(x, y)
    M, n = r.shape
    S = M - (y is not None)
    valid = np.isfinite(r).all(axis=0)
    rv = r[:, valid].astype(np.float64)
    d2 = np.zeros((M, M), dtype=np.float64)
    for i in range(M):
        for j in range(i + 1, M):
            d = rv[i] - rv[j]
            d2[i, j] = d2[j, i] = float((d * d).sum())
    nv = int(valid.sum())
    return dict(valid=valid, d2=d2, counts=(nv, n - nv), pick=picks(d2, S, y is not None))


def exact_int(x, y=None):
    """the matrix of integer-valued rows in int64 arithmetic (all pixels taken as valid) -> [M, M] int64"""
    r = rows_of(x, y)
    ri = r.astype(np.int64)
    assert np.array_equal(ri.astype(np.float32), r), "exact_int: the rows are not integer-valued"
    d = ri[:, None, :] - ri[None, :, :]
    return (d * d).sum(axis=2)


def summary(d2, valid, S, has_target):
    """one image's scores from the definitions -> dict(ES, ES_FAIR, DIVERSITY, RMS_member, RMS_best, RMS_medoid)"""
    nan = float("nan")
    out = dict(ES=nan, ES_FAIR=nan, DIVERSITY=nan, RMS_member=nan, RMS_best=nan, RMS_medoid=nan)
    if valid == 0:
        return out
    dist = np.sqrt(np.asarray(d2, dtype=np.float64)) / math.sqrt(valid)
    mm = dist[:S, :S]
    pair_mean_all = mm.sum() / (S * S)                    # E|X - X'| under the empirical distribution (the zero diagonal counts)
    if S > 1:
        out["DIVERSITY"] = mm.sum() / (S * (S - 1))       # the same mean over the pairs i != j
    if has_target:
        to_truth = dist[:S, S]
        out["ES"] = to_truth.mean() - 0.5 * pair_mean_all
        if S > 1:
            out["ES_FAIR"] = to_truth.mean() - 0.5 * out["DIVERSITY"]
        out["RMS_member"] = to_truth.mean()
        out["RMS_best"] = to_truth.min()
        out["RMS_medoid"] = to_truth[int(np.argmin(mm.sum(axis=1)))]
    return out


def draw(S, n, seed, spread=0.1):
    """y ~ U(-1, 1), x_s = y + N(0, spread): members that differ by far less than their magnitude.  float32 [S, n], [n]."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1, 1, n).astype(np.float32)
    x = (y[None] + rng.normal(0, spread, (S, n))).astype(np.float32)
    return x, y


def draw_int(S, n, seed, lim=1024):
    """integer-valued float32 rows with |value| <= lim (2^10: differences <= 2^11, squares <= 2^22, exact in any order up to 2^31 pixels)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-lim, lim + 1, (S, n)).astype(np.float32), rng.integers(-lim, lim + 1, n).astype(np.float32))
