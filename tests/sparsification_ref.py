"""numpy emulation of idiff_sparsification's contract (include/idiff.h) and an independent restatement of the host summary
(models/SDEs/driftSDE.py: sparsification_summary).  The order is taken from np.sort of the mapped integer keys; the sums are float64
sums of the widened float32 squared errors (np.sum: an order of its own, which the GPU test's bound allows for)."""
import itertools
import math

import numpy as np

QNAN = np.uint32(0x7fc00000)


def key_map(key):
    """float32 keys -> uint32 keys of the same order, in integers: -0 -> +0 first, then u = sign ? ~b : b | 0x80000000"""
    b = np.ascontiguousarray(key, dtype=np.float32).view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = np.uint32(0)
    return np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_unmap(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.where((u >> np.uint32(31)) != 0, u & np.uint32(0x7fffffff), ~u).astype(np.uint32)


def squared_error(pred, target):
    """e = d*d, d = pred - target: each rounded once in float32"""
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32)
        return (d * d).astype(np.float32)


def emulate(key, pred, target, K):
    """one image: key [n] float32 or None (the oracle: key = e), pred, target [n] -> dict(sums float64 [K + 1, 2], counts int64 [K + 1, 2],
    tau uint32 [K] (the bits), m int64 [K], e, u, valid)"""
    e = squared_error(pred, target)
    key = e if key is None else np.asarray(key, dtype=np.float32)
    valid = ~np.isnan(key) & ~np.isnan(e)
    u = key_map(key)
    uv, ev = u[valid], e[valid].astype(np.float64)
    N = int(valid.sum())
    desc = np.sort(uv)[::-1]
    sums = np.zeros((K + 1, 2), dtype=np.float64)
    counts = np.zeros((K + 1, 2), dtype=np.int64)
    tau = np.full(K, QNAN, dtype=np.uint32)
    m = np.array([(k * N) // K for k in range(K)], dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(K):
            if m[k] == 0:
                continue
            t = desc[m[k] - 1]
            above, at = uv > t, uv == t
            counts[k] = (int(above.sum()), int(at.sum()))
            sums[k] = (ev[above].sum(), ev[at].sum())
            tau[k] = key_unmap(t)
        sums[K, 0] = ev.sum()
    counts[K] = (N, key.size - N)
    return dict(sums=sums, counts=counts, tau=tau, m=m, e=e, u=u, valid=valid)


def removed(rec, K):
    """one image's emulation (or any (sums, counts) pair as a dict) -> (R[k], m[k], total, N): R_k = A_k + (m_k - c_k) T_k / t_k"""
    sums, counts = np.asarray(rec["sums"], dtype=np.float64), np.asarray(rec["counts"], dtype=np.int64)
    N = int(counts[K, 0])
    R, m = np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        m[k] = (k * N) // K
        if m[k]:
            c, t = int(counts[k, 0]), int(counts[k, 1])
            assert c < m[k] <= c + t, (k, c, t, m[k])
            R[k] = sums[k, 0] + (m[k] - c) * sums[k, 1] / t
    return R, m, float(sums[K, 0]), N


def brute_force_removed(key, e, K):
    """the mean, over every order of the pixels that sorts the mapped keys descending (all orders inside the tie groups), of the error
    of the first m_k pixels: what a sort with a uniformly random tie-break removes on average.  Small arrays only."""
    u = key_map(key)
    e = np.asarray(e, dtype=np.float64)
    n = len(u)
    groups = [np.nonzero(u == v)[0].tolist() for v in sorted(set(u.tolist()), reverse=True)]
    m = [(k * n) // K for k in range(K)]
    acc, orders = np.zeros(K), 0
    for perm in itertools.product(*[list(itertools.permutations(g)) for g in groups]):
        order = [i for g in perm for i in g]
        for k in range(K):
            acc[k] += e[order[:m[k]]].sum()
        orders += 1
    return acc / orders


def summary(recs, recs_oracle, K):
    """the host summary restated: pooled curves (total - R_k)/(N - m_k) of the map, the oracle and random, their k = 0 normalisation,
    and the trapezoid areas over k/K on the curves and on their square roots"""
    def pool(rs):
        R, m, total, N = np.zeros(K), np.zeros(K, dtype=np.int64), 0.0, 0
        for r in rs:
            Ri, mi, ti, Ni = removed(r, K)
            if Ni:
                R, m, total, N = R + Ri, m + mi, total + ti, N + Ni
        return R, m, total, N

    nan = float("nan")
    with np.errstate(all="ignore"):
        R, m, total, N = pool(recs)
        Ro, mo, total_o, No = pool(recs_oracle)
        curve = (total - R) / (N - m) if N else np.full(K, nan)
        oracle = (total_o - Ro) / (No - mo) if No else np.full(K, nan)
        random = np.full(K, total / N if N else nan)
        x = np.arange(K) / K

        def norm(c):
            return c / c[0] if c[0] > 0 else np.full(K, nan)

        def area(d):
            return float(np.sum(0.5 * (d[1:] + d[:-1]) * np.diff(x))) if K > 1 else nan

        cn, on, rn = norm(curve), norm(oracle), norm(random)
        cr, orr, rr = norm(np.sqrt(curve)), norm(np.sqrt(oracle)), norm(np.sqrt(random))
    return dict(fractions=x, curve=curve, oracle=oracle, random=random, curve_norm=cn, oracle_norm=on, random_norm=rn, AUSE=area(cn - on),
                AURG=area(rn - cn), AUSE_RMSE=area(cr - orr), AURG_RMSE=area(rr - cr), N=N,
                invalid=int(sum(int(np.asarray(r["counts"])[K, 1]) for r in recs)))


def close(a, b, rel=1e-12):
    """two floats or arrays agree to rel, NaN matching NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))) | (a == b)))


def isnan(v):
    return isinstance(v, float) and math.isnan(v)
