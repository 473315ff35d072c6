"""The F(4x4,3x3) input transform on a nearest x2 upsampled source, restated without the library (numpy, float32), and Python mirrors of
pos(), pos_live() and quad_live() of csrc/wino_common.h.  Shared by test_wino_upsample_cpu.py; pure data and arithmetic.

The claim of csrc/wino_common.h (pos_live): the 6x6 input tile of a 4x4 output tile starts at an odd row and column of the x2 grid, so tile
rows 1 and 2 are the same low-resolution row and so are rows 3 and 4 (columns alike); Winograd row 2 = fma(-1, Y, X) with X and Y the
same bits and column 2 = p - q of bt6 with p and q the same bits are exactly +0: the 11 positions (u, v) with u == 2 or v == 2.

fma(a, b, c) is evaluated as float32(float64(a) * float64(b) + float64(c)): the product is exact in float64, the sum is rounded twice,
which can differ from a fused multiply-add in the last bit -- but it is a function of (a, b, c), which is all the argument needs: equal
operands give equal bits."""
import numpy as np

F32 = np.float32


# ---- csrc/wino_common.h ---------------------------------------------------------------------------------------------------------------
def PF(u):
    return (3 * u + 1) // 2


def PH(u):
    return 1 + 3 * (u // 2)


def pos(u, v):
    return 4 * PF(u) + v if v < 4 else 4 * PH(u) + 2 * (u & 1) + (v - 4)


def pos_live(u, v, upsampled=True):
    return not upsampled or (u != 2 and v != 2)


def quad_live(quad, upsampled=True):
    m = 0
    for u in range(6):
        for v in range(6):
            if pos_live(u, v, upsampled) and pos(u, v) // 4 == quad:
                m |= 1 << (pos(u, v) & 3)
    return m


# the table of the kernel's comment, by hand: quad -> live components
QUAD_TABLE = {0: {0, 1, 3}, 1: {0, 1, 2, 3}, 2: {0, 1, 3}, 3: set(), 4: {2, 3}, 5: {0, 1, 3}, 6: {0, 1, 3}, 7: {0, 1, 2, 3}, 8: {0, 1, 3}}


# ---- the transform, as conv_wino4.hip computes it --------------------------------------------------------------------------------------
def fma(a, b, c):
    return (np.float64(a) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def row_fold(d):
    """B^T d along the rows: d [..., 6 rows, 6 cols] float32 -> [..., 6 Winograd rows, 6 cols] (tr_piece: the light waves' rows 0 and 5,
    the heavy waves' pairs (1, 2) with al = -4, be = 1 and (3, 4) with al = -1, be = 2)"""
    d = np.asarray(d, F32)
    r = [d[..., i, :] for i in range(6)]
    out = np.empty_like(d)
    out[..., 0, :] = fma(4.0, r[0], F32(-5.0) * r[2]) + r[4]
    out[..., 5, :] = fma(4.0, r[1], F32(-5.0) * r[3]) + r[5]
    for u, al, be in ((1, -4.0, 1.0), (3, -1.0, 2.0)):
        X, Y = fma(al, r[2], r[4]), fma(al, r[1], r[3])
        out[..., u, :] = fma(be, Y, X)
        out[..., u + 1, :] = fma(-be, Y, X)
    return out


def bt6(x):
    """bt6 of csrc/wino_common.h along the last axis"""
    x = np.asarray(x, F32)
    c_ = [x[..., i] for i in range(6)]
    o = np.empty_like(x)
    o[..., 0] = fma(4.0, c_[0], fma(-5.0, c_[2], c_[4]))
    p, q = fma(-4.0, c_[2], c_[4]), fma(-4.0, c_[1], c_[3])
    o[..., 1] = p + q
    o[..., 2] = p - q
    c, e = c_[4] - c_[2], c_[3] - c_[1]
    o[..., 3] = fma(2.0, e, c)
    o[..., 4] = fma(-2.0, e, c)
    o[..., 5] = fma(4.0, c_[1], fma(-5.0, c_[3], c_[5]))
    return o


def input_transform(d):
    """B^T d B of tiles d [..., 6, 6]"""
    return bt6(row_fold(d))


def upsampled_tiles(src):
    """every 6x6 input tile of the conv over the nearest x2 upsample of src [Hin, Win]: [tiles_y, tiles_x, 6, 6], element (r, c) of tile
    (ty, tx) = the x2 image at (4 ty - 1 + r, 4 tx - 1 + c), zero outside it (gather_decode: source (oy >> 1, ox >> 1)).  The tile grid is
    that of the kernel's 16x32 patches, so tiles that lie partly or wholly below / right of the image are included."""
    src = np.asarray(src, F32)
    Hin, Win = src.shape
    Hout, Wout = 2 * Hin, 2 * Win
    tiles_y, tiles_x = -(-Hout // 16) * 4, -(-Wout // 32) * 8
    oy = 4 * np.arange(tiles_y)[:, None] - 1 + np.arange(6)[None, :]  # [ty, r]
    ox = 4 * np.arange(tiles_x)[:, None] - 1 + np.arange(6)[None, :]  # [tx, c]
    iny, inx = (oy >= 0) & (oy < Hout), (ox >= 0) & (ox < Wout)
    sy, sx = np.clip(oy >> 1, 0, Hin - 1), np.clip(ox >> 1, 0, Win - 1)
    t = src[sy[:, None, :, None], sx[None, :, None, :]]
    return np.where(iny[:, None, :, None] & inx[None, :, None, :], t, F32(0))
