"""numpy float64 emulation of idiff_radial_power_spectrum's contract (include/idiff.h), an independent reference from np.fft.rfft2, the
inputs the CPU and GPU tests share, and the two tolerances they hold the results to."""
import functools

import numpy as np

from instancediff_amd import ops

# (H, W) -> rows R of the plain case: inside one MFMA tile; non-square, both even; both odd (no Nyquist column, tails in both GEMMs);
# K loops and strips that are no multiple of the tile; several tiles; the real size
SHAPES = {(1, 1): 3, (8, 8): 5, (6, 10): 3, (17, 23): 5, (16, 40): 1, (80, 48): 3, (64, 64): 5, (224, 224): 2}
SMALL = [s for s in SHAPES if s != (224, 224)]
MODES = ("plain", "sub1", "sub3")  # no sub with R rows; sub_rep = 1 with R = 3; sub_rep = 3 with R = 6

# The emulation's own largest relative error per bin against np.fft.rfft2 over every zero-mean white-noise case below (all SHAPES, all
# MODES), measured on the CPU with measure_emulation(): 6.61e-15 (the issue expected 3e-14 or below).  The GPU test allows REL_MARGIN times it: the
# margin is for another summation order, not for another precision.
EMULATION_MAX_REL = 6.7e-15
REL_MARGIN = 64.0


def weights(W):
    v = np.arange(W // 2 + 1)
    return np.where((v == 0) | (2 * v == W), 1.0, 2.0)


def twiddle(N):
    """(cos, sin)(2 pi m / N), m < N: the kernel's table"""
    ang = 2.0 * np.arange(N) / N
    return np.cos(np.pi * ang), np.sin(np.pi * ang)


def derived_bound(H, W, counts, sumsq):
    """|out[r, k] - ref[r, k]| <= 8 (H + W + 8) 2^-53 counts[k] sum a^2: the worst case of an fp64 direct DFT (gamma over the two sum
    lengths) carried through |X|^2 and Cauchy-Schwarz; counts [nb], sumsq [R] -> [R, nb]"""
    return 8.0 * (H + W + 8) * 2.0 ** -53 * np.asarray(counts, dtype=np.float64)[None, :] * np.asarray(sumsq, dtype=np.float64)[:, None]


def parseval_bound(H, W, sumsq):
    """|sum_k out[r, k] - sum a^2| on the device, to first order in u = 2^-53, relative to sum a^2.  A pass Y = a F computed as a matrix
    product has |dY| <= gamma_K |a| |F| entrywise (K the sum length); in Frobenius norm |a||F| is at most |a|_F K (every |F| entry
    is 1) while |Y|_F = sqrt(K) |a|_F, so the pass moves the plane's norm by at most K^1.5 u relatively, and a table whose entries
    are 2 u off by another 2 sqrt(K) u.  The power doubles a norm's relative error: 2 (W^1.5 + H^1.5) + 4 (sqrt W + sqrt H).  Then 8
    roundings per point (squares, their sum, the division, the weight) and the bins' sums: a wave adds at most 128 ceil(n / 2048)
    points one after the other and 16 waves are added, n = H (W/2 + 1) the points of the plane."""
    n = H * (W // 2 + 1)
    terms = 2.0 * (W ** 1.5 + H ** 1.5) + 4.0 * (W ** 0.5 + H ** 0.5) + 8.0 + 128.0 * -(-n // 2048) + 16.0
    return terms * 2.0 ** -53 * np.asarray(sumsq, dtype=np.float64)


def row_images(x, sub=None, sub_rep=1):
    a = np.asarray(x, dtype=np.float32).astype(np.float64)
    if sub is not None:
        a = a - np.repeat(np.asarray(sub, dtype=np.float32).astype(np.float64), sub_rep, axis=0)
    return a


def bin_power(P, W, bins, nb, finite):
    """P [R, H, Wh] -> [R, nb]: w_v P added per bin in (u, v) order; an entry outside [0, nb) drops its point; NaN rows where not finite"""
    R = P.shape[0]
    flat = np.asarray(bins).reshape(-1).astype(np.int64)
    keep = (flat >= 0) & (flat < nb)
    out = np.empty((R, nb))
    for r in range(R):
        wp = (P[r] * weights(W)[None, :]).reshape(-1)
        out[r] = np.bincount(flat[keep], weights=wp[keep], minlength=nb) if finite[r] else np.nan
    return out


def _tables(H, W, bins, nb):
    if bins is None:
        table, counts, _ = ops.radial_bins(H, W)
        return table.numpy(), int(counts.numel())
    return np.asarray(bins), nb


def emulate(x, sub=None, sub_rep=1, bins=None, nb=None):
    """x [R, H, W] float32 (sub [R / sub_rep, H, W]) -> float64 [R, nb]: the direct DFT as two matrix products, rows then columns, with
    the table's twiddles at integer-reduced indices"""
    a = row_images(x, sub, sub_rep)
    R, H, W = a.shape
    Wh = W // 2 + 1
    bins, nb = _tables(H, W, bins, nb)
    finite = np.isfinite(a).all(axis=(1, 2))
    a = np.where(finite[:, None, None], a, 0.0)
    cw, sw = twiddle(W)
    ch, sh = twiddle(H)
    iw = (np.arange(W)[:, None] * np.arange(Wh)[None, :]) % W  # [x, v]
    ih = (np.arange(H)[:, None] * np.arange(H)[None, :]) % H   # [u, y]
    Yr, Yi = a @ cw[iw], a @ -sw[iw]                             # [R, y, v]
    Xr = ch[ih] @ Yr + sh[ih] @ Yi
    Xi = ch[ih] @ Yi - sh[ih] @ Yr
    return bin_power((Xr * Xr + Xi * Xi) / float(H * W), W, bins, nb, finite)


def reference(x, sub=None, sub_rep=1, bins=None, nb=None):
    """the same quantity from np.fft.rfft2"""
    a = row_images(x, sub, sub_rep)
    R, H, W = a.shape
    bins, nb = _tables(H, W, bins, nb)
    finite = np.isfinite(a).all(axis=(1, 2))
    X = np.fft.rfft2(np.where(finite[:, None, None], a, 0.0), axes=(1, 2))
    return bin_power((X.real ** 2 + X.imag ** 2) / float(H * W), W, bins, nb, finite)


@functools.lru_cache(maxsize=None)
def case(shape, mode, kind="white"):
    """the shared inputs -> (x [R, H, W] float32, sub or None, sub_rep): kind "white" = N(0, 1), every bin holds comparable power;
    "dc" = 0.5 + 0.3 N(0, 1), bin 0 holds most of it"""
    H, W = shape
    R = {"plain": SHAPES[shape], "sub1": 3, "sub3": 6}[mode]
    sub_rep = 3 if mode == "sub3" else 1
    rng = np.random.default_rng(1000 * H + W + 7 * MODES.index(mode) + (0 if kind == "white" else 500000))

    def draw(n):
        g = rng.standard_normal((n, H, W))
        return (g if kind == "white" else 0.5 + 0.3 * g).astype(np.float32)

    x = draw(R)
    sub = None if mode == "plain" else draw(R // sub_rep)
    for arr in (x, sub):
        if arr is not None:
            arr.setflags(write=False)
    return x, sub, sub_rep


@functools.lru_cache(maxsize=None)
def case_reference(shape, mode, kind="white"):
    x, sub, sub_rep = case(shape, mode, kind)
    ref = reference(x, sub, sub_rep)
    ref.setflags(write=False)
    return ref


def all_cases():
    return [(s, m) for s in SHAPES for m in MODES if m == "plain" or s != (224, 224)]


def max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / ref))


def measure_emulation():
    """the emulation's largest relative error per bin against np.fft.rfft2 on the white-noise cases: EMULATION_MAX_REL"""
    return max(max_rel(emulate(*case(s, m)), case_reference(s, m)) for s, m in all_cases())
