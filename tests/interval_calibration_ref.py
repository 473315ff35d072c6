"""Reference for the conformal calibration of interval maps, used by tests/test_interval_calibration_cpu.py: a numpy float32
statement of the contract a device implementation has to meet.  Per pixel, every operation rounded once, nothing fused:
    dl = center - lo ;  du = hi - center ;  lo_out = center - (lam * dl) ;  hi_out = center + (lam * du)
and the counts are the histogram of the first entry of an ascending table at which target lies inside [lo_out, hi_out], from a LINEAR
scan -- the definition; a search by bisection gives the same counts because the predicate is monotone along the table (checked in
the CPU tests)."""
import functools

import numpy as np

F = np.float32


def scale(lo, hi, center, lam):
    """(lo_out, hi_out): dl = c - lo, du = hi - c, lo_out = c - lam*dl, hi_out = c + lam*du"""
    lo, hi, center, lam = np.asarray(lo, F), np.asarray(hi, F), np.asarray(center, F), F(lam)
    with np.errstate(all="ignore"):
        dl = center - lo
        du = hi - center
        return center - lam * dl, center + lam * du


def valid_mask(lo, hi, center, target):
    with np.errstate(all="ignore"):
        return (lo <= center) & (center <= hi) & ~np.isnan(target)  # a NaN lo / center / hi fails a comparison by itself


def covered(lo, hi, center, target, lam):
    """the predicate of bin g: target inside the interval scaled by lam"""
    a, b = scale(lo, hi, center, lam)
    with np.errstate(all="ignore"):
        return (target >= a) & (target <= b)


def bins(lo, hi, center, target, lams):
    """per pixel the bin: the first g that covers, G if none does, G + 1 if invalid (a NaN among the four, or not lo <= center <= hi)"""
    lams = np.asarray(lams, F).reshape(-1)
    G = lams.size
    lo, hi, center, target = (np.asarray(a, F) for a in (lo, hi, center, target))
    out = np.full(lo.shape, G, dtype=np.int64)
    for g in range(G - 1, -1, -1):  # descending, so that the smallest covering g is written last
        out[covered(lo, hi, center, target, lams[g])] = g
    out[~valid_mask(lo, hi, center, target)] = G + 1
    return out


def counts(lo, hi, center, target, lams):
    """int32 [B][G + 2] of maps [B, ...]"""
    G = np.asarray(lams).size
    b = bins(lo, hi, center, target, lams)
    return np.stack([np.bincount(b[i].reshape(-1), minlength=G + 2) for i in range(b.shape[0])]).astype(np.int32)


def inside_count(lo, hi, target):
    """idiff_interval_coverage's middle count per image: the pixels with lo <= target <= hi"""
    with np.errstate(all="ignore"):
        ok = ~(np.isnan(lo) | np.isnan(hi) | np.isnan(target))
        return ((target >= lo) & (target <= hi) & ok).reshape(lo.shape[0], -1).sum(1)


def table(G, lam_max=8.0):
    """the tables the tests use: one entry, or g * lam_max / (G - 1) in double rounded to float32 (driftSDE.calibration_grid's rule)"""
    if G == 1:
        return np.array([1.5], F)
    return (np.arange(G, dtype=np.float64) * lam_max / (G - 1)).astype(F)


@functools.lru_cache(maxsize=None)
def draw(shape, kind, G, B=2):
    """(lo, hi, center, target, lams) float32, maps [B, *shape]; computed once per case and shared, never modified.
    normal: center ~ N(0, 1), half widths 0.3 |N(0, 1)| on each side, target = center + 0.6 N(0, 1): bins from 0 to G at lam_max = 8
    ties:   the same, and every third pixel's target placed exactly on lo_out(lam_g) or hi_out(lam_g) of a g drawn per pixel
    zero:   lo = center = hi; every other target equals the centre (bin 0 at any lam), the rest differ (bin G)"""
    rng = np.random.default_rng(1000 * G + shape[1] + {"normal": 0, "ties": 7, "zero": 13}[kind])
    full = (B,) + tuple(shape)
    lams = table(G)
    center = rng.standard_normal(full).astype(F)
    lo = center - (F(0.3) * np.abs(rng.standard_normal(full))).astype(F)
    hi = center + (F(0.3) * np.abs(rng.standard_normal(full))).astype(F)
    target = center + (F(0.6) * rng.standard_normal(full)).astype(F)
    if kind == "ties":
        g = rng.integers(0, G, size=full)
        lam = lams[g]
        a, b = scale(lo, hi, center, lam)
        on_lo = rng.integers(0, 2, size=full).astype(bool)
        pick = (np.arange(center.size).reshape(full) % 3) == 0
        target = np.where(pick, np.where(on_lo, a, b), target).astype(F)
    if kind == "zero":
        lo = center.copy()
        hi = center.copy()
        same = (np.arange(center.size).reshape(full) % 2) == 0
        target = np.where(same, center, target).astype(F)
        assert (target[~same] != center[~same]).all()
    for a in (lo, hi, center, target, lams):
        a.setflags(write=False)
    return lo, hi, center, target, lams


def guarantee_case(seed, N=19, M=200, S=4, hw=16):
    """The seeded check of the guarantee: truth y ~ N(0, 1), members y + e + 0.5 n with a shared error e ~ N(0, 1) per pixel and member
    noise n ~ N(0, 1); y, e and n are each drawn for all N + M images at once, in that order.  lo = min, hi = max, median = 0.5 x_(1) +
    0.5 x_(2) of the S = 4 members.  -> (lo, hi, median, y), each [N + M, hw, hw] float32: the first N are the calibration images."""
    rng = np.random.default_rng(seed)
    n_img = N + M
    y = rng.standard_normal((n_img, hw, hw)).astype(F)
    e = rng.standard_normal((n_img, hw, hw)).astype(F)
    n = rng.standard_normal((n_img, S, hw, hw)).astype(F)
    x = np.sort(y[:, None] + e[:, None] + F(0.5) * n, axis=1)
    med = F(0.5) * x[:, (S - 1) // 2] + F(0.5) * x[:, S // 2]
    return x[:, 0], x[:, -1], med, y
