"""References for the ensemble scores (include/idiff.h, idiff_ensemble_scores), shared by the CPU and the GPU tests.

emulate(x, y): the contract operation for operation in numpy float32 (numpy rounds every float32 operation once and contracts nothing;
  a float32 quotient is correctly rounded, as the kernel's quotient through fp64 is).
textbook(x, y): float64 from the textbook formulas: the double sum over pairs, np.var(ddof=1), (x < y).sum().
x is [S, n] and y is [n]; both take float32 arrays."""
import numpy as np

U = 2.0 ** -24


def emulate(x, y):
    """-> dict(d [S, n] f32, ranks [S, n] int, crps, e, v [n] f32, k [n] int, valid [n] bool): per pixel what the kernel computes"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    S, n = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - y[None]
        ranks = np.zeros((S, n), dtype=np.int64)
        for s in range(S):
            for j in range(S):
                ranks[s] += d[j] < d[s]
                if j < s:
                    ranks[s] += d[j] == d[s]
        c = (2 * ranks - S + 1).astype(np.float32)
        a, g, sd = np.abs(d[0]), c[0] * d[0], d[0].copy()
        for s in range(1, S):
            a = a + np.abs(d[s])
            g = g + c[s] * d[s]
            sd = sd + d[s]
        crps = a / np.float32(S) - g / np.float32(S * S)
        m = sd / np.float32(S)
        e = m * m
        t = d[0] - m
        ss = t * t
        for s in range(1, S):
            t = d[s] - m
            ss = ss + t * t
        v = ss / np.float32(S - 1) if S > 1 else np.zeros(n, dtype=np.float32)
        k = (d < 0).sum(axis=0)
    assert crps.dtype == e.dtype == v.dtype == np.float32
    return dict(d=d, ranks=ranks, crps=crps, e=e, v=v, k=k, valid=~np.isnan(d).any(axis=0))


def textbook(x, y):
    """-> dict(ranks [S, n] int, crps, e, v [n] f64, k [n] int), from the definitions, on the x themselves"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    S, n = x.shape
    pairs = np.zeros(n)
    ranks = np.zeros((S, n), dtype=np.int64)
    for i in range(S):
        for j in range(S):
            pairs += np.abs(x[i] - x[j])
            ranks[i] += x[j] < x[i]
            if j < i:
                ranks[i] += x[j] == x[i]
    crps = np.abs(x - y[None]).mean(axis=0) - pairs / (2.0 * S * S)
    e = (x.mean(axis=0) - y) ** 2
    v = np.var(x, axis=0, ddof=1) if S > 1 else np.zeros(n)
    return dict(ranks=ranks, crps=crps, e=e, v=v, k=(x < y[None]).sum(axis=0))


def image_record(em, S):
    """(sums float64 [3], counts int64 [S + 2]) of one image from emulate()'s output: float64 sums of the emulated per-pixel float32 values
    over the valid pixels, the rank histogram, the invalid count"""
    ok = em["valid"]
    sums = np.array([em[q][ok].astype(np.float64).sum() for q in ("crps", "e", "v")])
    counts = np.concatenate([np.bincount(em["k"][ok], minlength=S + 1), [int((~ok).sum())]]).astype(np.int64)
    return sums, counts


def draw(S, n, seed, spread=0.1):
    """the issue's inputs: y ~ U(-1, 1), x_s = y + N(0, spread); in a fifth of the pixels one member equals y, in another fifth two
    members are equal (S >= 2).  float32 [S, n], [n]."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1, 1, n).astype(np.float32)
    x = (y[None] + rng.normal(0, spread, (S, n))).astype(np.float32)
    which = rng.integers(0, 5, n)
    member = rng.integers(0, S, n)
    hit = np.nonzero(which == 0)[0]
    x[member[hit], hit] = y[hit]
    if S >= 2:
        dup = np.nonzero(which == 1)[0]
        x[(member[dup] + 1) % S, dup] = x[member[dup], dup]
    return x, y
