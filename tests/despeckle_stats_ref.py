"""References for the no-reference despeckling statistics (include/idiff.h, idiff_despeckle_stats), shared by the CPU and the GPU tests.

pixel_terms(x, ref, scale, shift, floor): the contract's per-pixel fp32 arithmetic in numpy float32 (every operation rounded once): a, y,
  rho, La, Ly and the three masks valid / ratio / stencil of one row x [P, H, W] against ref [P, H, W].
emulate(x, ref, labels, L, ...): the 12 terms per pixel converted to float64 (products formed in float64: exact), summed per region
  with math.fsum (the exact sum, rounded once), sum |t| per region and quantity for the bound of a sum, the four counts and the outside
  count.
textbook(x, ref, labels, L, ...): float64 throughout from the textbook formulas, grouped the same way.
sum_bound, same and every_partial_sum_is_exact are region_scores_ref's."""
import math

import numpy as np

from region_scores_ref import every_partial_sum_is_exact, same, sum_bound  # noqa: F401

QUANT = ("a", "aa", "y", "yy", "ay", "rho", "rho2", "la", "ly", "lala", "lyly", "laly")
NEED = (0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2)  # the count a quantity runs over: 0 valid, 1 ratio, 2 stencil
NAN, INF = float("nan"), float("inf")


def _shift(v, dy, dx):
    """v[p, r + dy, c + dx] where that lies in the plane, else 0, and the mask of where it does"""
    P, H, W = v.shape
    out, inside = np.zeros_like(v), np.zeros(v.shape, dtype=bool)
    r0, r1 = max(0, -dy), min(H, H - dy)
    c0, c1 = max(0, -dx), min(W, W - dx)
    if r0 < r1 and c0 < c1:
        out[:, r0:r1, c0:c1] = v[:, r0 + dy:r1 + dy, c0 + dx:c1 + dx]
        inside[:, r0:r1, c0:c1] = True
    return out, inside


def _terms(x, ref, scale, shift, floor, dt):
    x, ref = np.asarray(x, dtype=dt), np.asarray(ref, dtype=dt)
    assert x.ndim == 3 and x.shape == ref.shape
    with np.errstate(all="ignore"):
        a = x * dt(scale) + dt(shift)  # numpy rounds the product, then the sum
        y = ref * dt(scale) + dt(shift)
        valid = np.isfinite(a) & np.isfinite(y)
        if dt is np.float64:  # the textbook takes the pixels the contract takes: validity is decided on the fp32 values
            a32 = np.asarray(x, np.float32) * np.float32(scale) + np.float32(shift)
            y32 = np.asarray(ref, np.float32) * np.float32(scale) + np.float32(shift)
            valid = np.isfinite(a32) & np.isfinite(y32)
            ratio = valid & (a32 >= np.float32(floor))
        else:
            ratio = valid & (a >= dt(floor))
        rho = np.where(ratio, y / np.where(ratio, a, dt(1)), dt(0)).astype(dt)
        sten = valid.copy()
        nb = {}
        for name, (dy, dx) in dict(N=(-1, 0), S=(1, 0), W=(0, -1), E=(0, 1)).items():
            an, inside = _shift(a, dy, dx)
            yn, _ = _shift(y, dy, dx)
            vn, _ = _shift(valid, dy, dx)
            sten &= inside & vn
            nb[name] = (np.where(vn, an, dt(0)), np.where(vn, yn, dt(0)))
        ac, yc = np.where(valid, a, dt(0)), np.where(valid, y, dt(0))
        la = ((nb["N"][0] + nb["S"][0]) + (nb["W"][0] + nb["E"][0])) - dt(4) * ac
        ly = ((nb["N"][1] + nb["S"][1]) + (nb["W"][1] + nb["E"][1])) - dt(4) * yc
    for v in (a, y, rho, la, ly):
        assert v.dtype == dt
    return dict(a=a, y=y, rho=rho, la=np.where(sten, la, dt(0)), ly=np.where(sten, ly, dt(0)), valid=valid, ratio=ratio, stencil=sten)


def pixel_terms(x, ref, scale=0.5, shift=0.5, floor=2.0 ** -8):
    return _terms(x, ref, scale, shift, floor, np.float32)


def _twelve(t):
    """the 12 per-pixel terms in float64; a product of two float32 values is exact in float64"""
    a, y, rho, la, ly = (t[k].astype(np.float64) for k in ("a", "y", "rho", "la", "ly"))
    with np.errstate(all="ignore"):
        return [a, a * a, y, y * y, a * y, rho, rho * rho, la, ly, la * la, ly * ly, la * ly]


def _sum(t, exact):
    if exact and np.isfinite(t).all():
        return math.fsum(t.tolist()) + 0.0  # + 0.0: the device starts every sum from +0.0, so an all -0.0 region gives +0.0
    with np.errstate(all="ignore"):
        return float(t.sum()) + 0.0


def group(t, labels, L, exact=True):
    """per-pixel terms by label -> dict(sums [L, 12], abs [L, 12] (sum |t|), counts [L, 4] = valid, ratio, stencil, invalid, outside,
    n [L, 3] = the three counts a quantity can run over, terms: the 12 float64 term arrays, masks: the 3 masks)"""
    labels = np.asarray(labels)
    assert labels.shape == t["a"].shape and labels.dtype == np.uint8
    terms = _twelve(t)
    masks = (t["valid"], t["ratio"], t["stencil"])
    sums, mags = np.zeros((L, 12)), np.zeros((L, 12))
    counts = np.zeros((L, 4), dtype=np.int64)
    counts[:, 3] = np.bincount(labels[~t["valid"]], minlength=256)[:L]
    for k, m in enumerate(masks):  # the pixels a quantity runs over, sorted by label once (stable: raster order inside a region)
        labs = labels[m]
        order = np.argsort(labs, kind="stable")
        cuts = np.searchsorted(labs[order], np.arange(L + 1))
        counts[:, k] = np.diff(cuts)
        for q in (q for q in range(12) if NEED[q] == k):
            vals = terms[q][m][order]
            for l in range(L):
                seg = vals[cuts[l]:cuts[l + 1]]
                sums[l, q] = _sum(seg, exact)
                mags[l, q] = float(np.abs(seg).sum())
    return dict(sums=sums, abs=mags, counts=counts, outside=int((labels >= L).sum()), n=counts[:, :3], terms=terms, masks=masks)


def emulate(x, ref, labels, L, scale=0.5, shift=0.5, floor=2.0 ** -8):
    return group(pixel_terms(x, ref, scale, shift, floor), labels, L)


def textbook(x, ref, labels, L, scale=0.5, shift=0.5, floor=2.0 ** -8):
    return group(_terms(x, ref, scale, shift, floor, np.float64), labels, L, exact=False)


# ---- values ---------------------------------------------------------------------------------------------------------------------------
def draw(P, H, W, seed, looks=4):
    """a smooth positive scene times gamma speckle of `looks` looks, and a lightly smoothed copy as the restoration, both on [-1, 1]
    -> (x, ref) float32 [P, H, W]"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    scene = 0.45 + 0.25 * np.sin(0.37 * r + seed)[None] * np.cos(0.23 * c)[None] + np.zeros((P, 1, 1))
    noisy = np.clip(scene * rng.gamma(looks, 1.0 / looks, (P, H, W)), 0.0, 1.0)
    clean = np.clip(scene * (1.0 + 0.05 * rng.standard_normal((P, H, W))), 0.0, 1.0)
    return (2.0 * clean - 1.0).astype(np.float32), (2.0 * noisy - 1.0).astype(np.float32)


def draw_integers(P, H, W, seed, factor=None):
    """x integers in 1 .. 8 and ref = x * {1, 2, 4} (per pixel, or `factor` everywhere): with scale = 1, shift = 0 every term is an integer
    (rho in {1, 2, 4}) and every partial sum exact"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 9, (P, H, W)).astype(np.float32)
    f = rng.choice(np.array([1.0, 2.0, 4.0], dtype=np.float32), (P, H, W)) if factor is None else np.float32(factor)
    return x, (x * f).astype(np.float32)


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def labels_blocks(P, H, W, L, seed=0):
    """coherent rectangles: a coarse random grid of labels, different per plane"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, L, (P, (H + 5) // 6, (W + 7) // 8))
    return np.repeat(np.repeat(coarse, 6, axis=1), 8, axis=2)[:, :H, :W].astype(np.uint8)


def labels_random(P, H, W, L, seed=0):
    return np.random.default_rng(seed).integers(0, L, (P, H, W)).astype(np.uint8)


def labels_checker(P, H, W, L=2, seed=0):
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (((r + c) % 2)[None] + np.zeros((P, 1, 1), dtype=np.int64)).astype(np.uint8)


def labels_outside(P, H, W, L, seed=0):
    """random labels < L with a fifth of the pixels outside (L, 200, 255)"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, L, (P, H, W)).astype(np.uint8)
    out = rng.random((P, H, W)) < 0.2
    lab[out] = rng.choice(np.array([L, 200, 255], dtype=np.uint8), int(out.sum()))
    return lab
