"""The Winograd minimal-filtering form of a 3x3 convolution in plain torch on the CPU, in any dtype: the conditioning floor of the
Winograd forward rows (test_wino_fwd_gpu.py).  Evaluated in fp32 it is the error the FORM itself costs against the fp64 direct
convolution on a row's own inputs, whatever the kernel's order of summation; a Winograd row's tolerance is max(project tolerance,
4 x that).  It serves no other purpose: no kernel is compared with it.

    Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A        per (m+2)x(m+2) input tile d, stride m, of the image padded by one pixel

with the matrices the kernels' comments state (csrc/wino_common.h: bt6 / at6 / g6; csrc/conv_wino.hip: pack_wino_kernel):
F(4x4,3x3) on the interpolation points 0, +-1, +-2, inf; F(2x2,3x3) with G rows (1,0,0), (.5,.5,.5), (.5,-.5,.5), (0,0,1)."""
import torch
import torch.nn.functional as F

from conv_branch_rows import U
from conv_branch_ref import silu

MATRICES = {
    2: dict(
        BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        G=[[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
        AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: dict(
        BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
        G=[[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
        AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}


def winograd_conv3x3(x, w, m):
    """conv2d(x, w, padding=1) of x [B, Cin, H, W] with w [Cout, Cin, 3, 3] by F(m x m, 3x3), m = 2 or 4, in x's dtype"""
    dt = x.dtype
    BT, G, AT = (torch.tensor(MATRICES[m][k], dtype=torch.float64).to(dt) for k in ("BT", "G", "AT"))
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    ty, tx = -(-H // m), -(-W // m)
    xp = F.pad(x, (1, tx * m + 1 - W, 1, ty * m + 1 - H))                       # one pixel of padding, then up to whole tiles
    d = xp.unfold(2, m + 2, m).unfold(3, m + 2, m)                               # [B, Cin, ty, tx, m+2, m+2]
    V = torch.einsum("ui,bcyxij,vj->bcyxuv", BT, d, BT)                          # B^T d B
    Ug = torch.einsum("ui,ocij,vj->ocuv", G, w.to(dt), G)                        # G g G^T
    M = torch.einsum("ocuv,bcyxuv->boyxuv", Ug, V)                               # sum over ci, position by position
    Y = torch.einsum("pu,boyxuv,qv->boyxpq", AT, M, AT)                          # A^T M A: [B, Cout, ty, tx, m, m]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, Cout, ty * m, tx * m)[:, :, :H, :W].contiguous()


def form_reference(row, inp, m, dtype=torch.float32):
    """(out, raw) of conv_branch_ref.reference with the convolution evaluated in the Winograd form F(m x m, 3x3)"""
    assert row["ks"] == 3
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    x = c(inp["src0"])
    if inp["pro"] is not None:
        pa, pb = (c(t)[:, :, None, None] for t in inp["pro"])
        x = silu(pa * x + pb)
    if inp["src1"] is not None:
        x = torch.cat([x, c(inp["src1"])], 1)
    if row["mode"] == U:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    raw = winograd_conv3x3(x, c(inp["w"]), m)
    if inp["bias"] is not None:
        raw = raw + c(inp["bias"])[None, :, None, None]
    out = raw
    if inp["res"] is not None:
        out = out + c(inp["res"])
    if inp["vec"] is not None:
        out = out + c(inp["vec"])[:, :, None, None]
    if inp["aux"] is not None:
        t, aa, ab = (c(v) for v in inp["aux"])
        out = out + silu(aa[:, :, None, None] * t + ab[:, :, None, None])
    return out, raw
