"""References for the region-wise ensemble scores (include/idiff.h, idiff_region_scores / idiff_band_labels), shared by the CPU and the GPU
tests.

pixel_record(x, y): ensemble_scores_ref.emulate's float32 per-pixel record plus the signed mean error m (the same operations as e's).
emulate(x, y, labels, L): that record grouped by label: float64 sums of the emulated float32 terms (math.fsum: the exact sum, rounded
  once), the rank histogram and the invalid count per region, the outside count, and sum |t| per region for the bound of a sum.
textbook(x, y, labels, L): float64 from the textbook formulas, grouped the same way.
The draw functions make the value and label populations of the tests.  x is [S, n], y is [n], labels is uint8 [n]."""
import math

import numpy as np

import ensemble_scores_ref as es

QUANT = ("crps", "e", "v", "m")
NAN, INF = float("nan"), float("inf")


def pixel_record(x, y):
    em = es.emulate(x, y)
    d = em["d"]
    S = d.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        sd = d[0].copy()
        for s in range(1, S):
            sd = sd + d[s]
        em["m"] = sd / np.float32(S)
    assert em["m"].dtype == np.float32
    return em


def _sum(t):
    """the float64 sum of float32 terms: exact (fsum) where every term is finite, else numpy's (inf or NaN either way)"""
    t = t.astype(np.float64)
    if np.isfinite(t).all():
        return math.fsum(t.tolist())
    with np.errstate(invalid="ignore"):
        return float(t.sum())


def group(rec, labels, L, S):
    """a per-pixel record (pixel_record's, or textbook's with `valid`) by label -> dict(sums [L, 4] f64, abs [L, 4] f64 (sum |t|), counts
    [L, S + 2] int64, outside int, n [L] valid pixels)"""
    labels = np.asarray(labels)
    sums, mags = np.zeros((L, 4)), np.zeros((L, 4))
    counts = np.zeros((L, S + 2), dtype=np.int64)
    ok = rec["valid"]
    for l in range(L):
        here = labels == l
        sel = here & ok
        for q, name in enumerate(QUANT):
            sums[l, q] = _sum(rec[name][sel])
            with np.errstate(invalid="ignore"):
                mags[l, q] = float(np.abs(rec[name][sel].astype(np.float64)).sum())
        counts[l, :S + 1] = np.bincount(rec["k"][sel], minlength=S + 1)
        counts[l, S + 1] = int((here & ~ok).sum())
    return dict(sums=sums, abs=mags, counts=counts, outside=int((labels >= L).sum()), n=counts[:, :S + 1].sum(axis=1))


def emulate(x, y, labels, L):
    return group(pixel_record(x, y), labels, L, np.asarray(x).shape[0])


def textbook(x, y, labels, L):
    tb = es.textbook(x, y)
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tb["m"] = xd.mean(axis=0) - yd
    tb["valid"] = ~(np.isnan(xd).any(axis=0) | np.isnan(yd))
    return group(tb, labels, L, xd.shape[0])


def same(got, want):
    """float64 equality that takes NaN = NaN and inf = inf of one sign"""
    return (math.isnan(got) and math.isnan(want)) or got == want


def sum_bound(n, mag):
    """two fp64 sums of n terms in different orders (here: any order against the exact sum, which is within the same bound) differ by
    at most 2 (n - 1) 2^-53 sum |t| to first order"""
    return 2 * max(n - 1, 0) * 2.0 ** -53 * mag


def every_partial_sum_is_exact(terms):
    """True if every sum of any subset of the float32 `terms`, in any order, is exactly representable in float64: all terms are multiples
    of the quantum q = the last bit of the smallest non-zero magnitude, and sum |t| / q < 2^53."""
    t = np.asarray(terms, dtype=np.float64)
    if not np.isfinite(t).all():
        return False
    nz = np.abs(t[t != 0])
    if nz.size == 0:
        return True
    q = 2.0 ** (math.frexp(float(nz.min()))[1] - 1 - 23)  # a float32's last bit at the smallest exponent present
    return float(nz.sum()) / q < 2.0 ** 53


# ---- values ---------------------------------------------------------------------------------------------------------------------------
def draw(S, n, seed, spread=0.1):
    return es.draw(S, n, seed, spread)


def spoil(x, y, seed, share=0.04):
    """NaN members, NaN targets and +-inf among the values, in about `share` of the pixels each kind a quarter -> copies"""
    rng = np.random.default_rng(seed)
    x, y = x.copy(), y.copy()
    S, n = x.shape
    kind = rng.integers(0, int(round(4 / share)), n)
    member = rng.integers(0, S, n)
    i = np.nonzero(kind == 0)[0]
    x[member[i], i] = NAN
    y[kind == 1] = NAN
    i = np.nonzero(kind == 2)[0]
    x[member[i], i] = INF
    i = np.nonzero(kind == 3)[0]
    x[member[i], i] = -INF
    return x, y


def draw_integers(S, n, seed, lo=-4, hi=4):
    """integer-valued x and y in [lo, hi]: every d_s is a small integer"""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, (S, n)).astype(np.float32), rng.integers(lo, hi + 1, n).astype(np.float32)


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def labels_constant(n, L, seed=0):
    return np.full(n, L - 1, dtype=np.uint8)


def labels_halves(n, L, seed=0):
    lab = np.zeros(n, dtype=np.uint8)
    lab[n // 2:] = min(1, L - 1)
    return lab


def labels_blobs(n, L, seed=0):
    """coherent runs of 3 .. 400 pixels, each of one random label: a wave holds one to three labels"""
    rng = np.random.default_rng(seed)
    lab = np.empty(n, dtype=np.uint8)
    i = 0
    while i < n:
        run = int(rng.integers(3, 401))
        lab[i:i + run] = rng.integers(0, L)
        i += run
    return lab


def labels_random(n, L, seed=0):
    """per pixel: from 64 L pixels on every wave holds every label"""
    return np.random.default_rng(seed).integers(0, L, n).astype(np.uint8)


def labels_single(n, L, seed=0):
    """label L - 1 on exactly one element (element 2 of one float4), label 0 elsewhere (for L = 1: all 0)"""
    lab = np.zeros(n, dtype=np.uint8)
    lab[(n // 8) * 4 + 2] = L - 1
    return lab


def labels_quad(n, L, seed=0):
    """four different labels inside every float4 (L >= 4; i mod L below that)"""
    i = np.arange(n)
    return ((i % 4 + i // 4) % L).astype(np.uint8)


def labels_outside(n, L, seed=0):
    """labels < L with labels >= L (L, 200 and the conventional 255) mixed in, a third of the pixels; the outside pixels are a multiple of
    four, so that the inside ones can be handed to idiff_ensemble_scores as an image of their own"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, L, n).astype(np.uint8)
    out = np.nonzero(rng.random(n) < 1 / 3)[0]
    out = out[:len(out) - len(out) % 4]
    lab[out] = rng.choice(np.array([L, 200, 255], dtype=np.uint8), len(out))
    return lab


LABELS = dict(constant=labels_constant, halves=labels_halves, blobs=labels_blobs, random=labels_random, single=labels_single,
              quad=labels_quad, outside=labels_outside)
