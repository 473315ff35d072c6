"""Inputs and the plain torch reference of the rows of wgrad_wino_rows.py (CPU only; any dtype).  The formula, as include/idiff.h states
it: prologue silu(a x + b) per (sample, channel) on src0 -> cat(src0, src1) -> nearest x2 upsample -> dW = autograd of
F.conv2d(., w, padding = 1) against dY (zero padding applies to the activated tensor); an accumulate row adds the prefilled dW."""
import torch
import torch.nn.functional as F

from wgrad_wino_rows import ROWS, U, out_size

SEED0 = 7000


def silu(x):
    return x / (1 + torch.exp(-x))


def make_inputs(row):
    """seeded fp32 CPU tensors of a row: randn; `dc` inputs with mean 3 and spread 0.5; prologue tables that differ by O(1) between the
    samples (a = 1 + 0.75 b, b = 0.5 - 0.6 b for sample b, each + 0.05 randn per channel), so that a table of the wrong sample shows"""
    g = torch.Generator().manual_seed(SEED0 + [r["name"] for r in ROWS].index(row["name"]))
    B, C0, C1, Cout, Hin, Win = (row[k] for k in ("B", "C0", "C1", "Cout", "Hin", "Win"))
    Hout, Wout = out_size(row)

    def image(*shape):
        t = torch.randn(*shape, generator=g)
        return t * 0.5 + 3.0 if row["dc"] else t

    inp = dict(src0=image(B, C0, Hin, Win), src1=image(B, C1, Hin, Win) if C1 else None, pro=None, dw0=None)
    inp["dy"] = torch.randn(B, Cout, Hout, Wout, generator=g)
    if row["pro"]:
        b = torch.arange(B, dtype=torch.float32)[:, None]
        inp["pro"] = (1.0 + 0.75 * b + 0.05 * torch.randn(B, C0, generator=g), 0.5 - 0.6 * b + 0.05 * torch.randn(B, C0, generator=g))
    if row["acc"]:
        inp["dw0"] = torch.randn(Cout, C0 + C1, 3, 3, generator=g)
    return inp


def gathered(row, inp, dtype):
    """the conv's input as the forward gathers it, materialised"""
    x = inp["src0"].to(dtype)
    if inp["pro"] is not None:
        pa, pb = (t.to(dtype)[:, :, None, None] for t in inp["pro"])
        x = silu(pa * x + pb)
    if inp["src1"] is not None:
        x = torch.cat([x, inp["src1"].to(dtype)], 1)
    if row["mode"] == U:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return x


def reference(row, inp, dtype=torch.float64):
    """dW [Cout, Cin, 3, 3] in `dtype` on the CPU"""
    x = gathered(row, inp, dtype)
    w = torch.zeros(row["Cout"], x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
    F.conv2d(x, w, None, padding=1).backward(inp["dy"].to(dtype))
    dw = w.grad
    return dw + inp["dw0"].to(dtype) if inp["dw0"] is not None else dw
