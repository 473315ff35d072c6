"""Inputs and the plain torch reference of the rows of conv_branch_rows.py (CPU only; any dtype).  The formula, as include/idiff.h
states it:  cat(src0, src1) -> prologue silu(a*x+b) on src0 -> nearest x2 / pixel_unshuffle(2) -> conv2d(padding = ks // 2) + bias
-> + res + vec + silu(aa * aux + ab); the GroupNorm partials are per-tile sums and sums of squares of conv + bias."""
import math

import torch
import torch.nn.functional as F

from conv_branch_rows import N, S, U, out_size, pick_twl, tile_shape


def silu(x):
    return x / (1 + torch.exp(-x))


def make_inputs(row, seed):
    """seeded fp32 CPU tensors of a row: randn, weights scaled by 1/sqrt(Cin*ks*ks), `dc` inputs with mean 3 and spread 0.5"""
    g = torch.Generator().manual_seed(seed)
    B, C0, C1, Cout, Hin, Win, ks = (row[k] for k in ("B", "C0", "C1", "Cout", "Hin", "Win", "ks"))
    Hout, Wout = out_size(row)

    def rnd(*shape, image=False):
        t = torch.randn(*shape, generator=g)
        return t * 0.5 + 3.0 if (image and row["dc"]) else t

    inp = dict(src0=rnd(B, C0, Hin, Win, image=True))
    inp["src1"] = rnd(B, C1, Hin, Win, image=True) if C1 else None
    Cin = (4 * C0 if row["mode"] == S else C0) + C1
    inp["w"] = rnd(Cout, Cin, ks, ks) / math.sqrt(Cin * ks * ks)
    inp["bias"] = rnd(Cout) if row["bias"] else None
    inp["pro"] = (rnd(B, C0), rnd(B, C0)) if row["pro"] else None
    inp["res"] = rnd(B, Cout, Hout, Wout, image=True) if row["res"] else None
    inp["vec"] = rnd(B, Cout) if row["vec"] else None
    inp["aux"] = (rnd(B, Cout, Hout, Wout, image=True), rnd(B, Cout), rnd(B, Cout)) if row["aux"] else None
    if row["gn"]:
        inp["gamma"], inp["beta"] = rnd(Cout), rnd(Cout)
    return inp


def reference(row, inp, dtype=torch.float64):
    """(out, raw): the call's result and conv + bias (what the statistics are taken of), evaluated in `dtype` on the CPU"""
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    x = c(inp["src0"])
    if inp["pro"] is not None:
        pa, pb = (c(t)[:, :, None, None] for t in inp["pro"])
        x = silu(pa * x + pb)
    if inp["src1"] is not None:
        x = torch.cat([x, c(inp["src1"])], 1)
    if row["mode"] == U:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    elif row["mode"] == S:
        x = F.pixel_unshuffle(x, 2)
    raw = F.conv2d(x, c(inp["w"]), c(inp["bias"]), padding=row["ks"] // 2)
    out = raw
    if inp["res"] is not None:
        out = out + c(inp["res"])
    if inp["vec"] is not None:
        out = out + c(inp["vec"])[:, :, None, None]
    if inp["aux"] is not None:
        t, aa, ab = (c(v) for v in inp["aux"])
        out = out + silu(aa[:, :, None, None] * t + ab[:, :, None, None])
    return out, raw


def tile_stats(raw):
    """[B][ntiles][Cout][2] (sum, sum of squares) over the tile grid idiff_conv2d_num_tiles describes: 8x32, 16x16 or 32x8 patches by the
    output width, row-major over the grid, border patches cut at the image -- tile by tile, in raw's dtype"""
    B, Cc, H, W = raw.shape
    TH, TW = tile_shape(pick_twl(W))
    ty, tx = -(-H // TH), -(-W // TW)
    st = torch.zeros(B, ty * tx, Cc, 2, dtype=raw.dtype)
    for i in range(ty):
        for j in range(tx):
            p = raw[:, :, i * TH:(i + 1) * TH, j * TW:(j + 1) * TW]
            st[:, i * tx + j, :, 0] = p.sum(dim=(2, 3))
            st[:, i * tx + j, :, 1] = (p * p).sum(dim=(2, 3))
    return st


def gn_affine(raw, groups, gamma, beta, eps=1e-5):
    """(a, b) [B, Cout] with GroupNorm(raw) = a * raw + b, in raw's dtype"""
    B, Cc = raw.shape[:2]
    rg = raw.reshape(B, groups, -1)
    mean, var = rg.mean(-1), rg.var(-1, unbiased=False)
    rstd = (1 / torch.sqrt(var + eps)).repeat_interleave(Cc // groups, dim=1)
    mean = mean.repeat_interleave(Cc // groups, dim=1)
    a = gamma.to(raw.dtype)[None] * rstd
    return a, beta.to(raw.dtype)[None] - mean * a
