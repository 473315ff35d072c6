"""Sentinel-guarded device operands and the error metric of the convolution branch tables (test_conv_branches_gpu.py,
test_wino_fwd_gpu.py): operands that are slices of sentinel-filled buffers, the bit-exact check that nothing around them was written,
and the normwise + elementwise comparison against an fp64 reference."""
import math

import torch

from conv_branch_rows import SLICE_LO

DEV = "cuda"
SENT = -777.25  # guard-band fill


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _floor(tol, f32, ref):
    """max(project tolerance, 4 x the fp32-on-the-CPU error of the same formula against fp64)"""
    return max(tol, 4 * _rel(f32, ref))


def _check(row, name, got, ref, tol, tails=(), base=None):
    """normwise max error of one output; every region of `tails` (indices into both) also element by element against tol * max|ref|"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (row, name, got.shape, ref.shape)
    scale = float(ref.abs().max().clamp_min(1e-12))
    e = float((got - ref).abs().max()) / scale
    msg = f"{row} {name}: rel {e:.2e} (tol {tol:.2e}" + (f", project tol {base:.1e}" if base is not None and base != tol else "") + ")"
    worst = []
    for what, t in tails:
        assert got[t].numel() > 0, (row, name, what, "empty tail")
        worst.append((what, float((got[t] - ref[t]).abs().max()) / scale))
        msg += f", {what} {worst[-1][1]:.2e}"
    print(msg)
    assert math.isfinite(e) and e <= tol, msg
    for what, et in worst:
        assert et <= tol, msg


def _buf(shape, extra=0, odd=False, src=None):
    """(flat, view): a device tensor of `shape` [B, C, ...] that is the channel slice [SLICE_LO : SLICE_LO + C] of a buffer with `extra`
    more channels (batch stride above the dense one) and starts one float past a 16-byte boundary when `odd`; everything around it
    holds the sentinel"""
    B, Cc = shape[:2]
    plane = 1
    for n in shape[2:]:
        plane *= n
    n = B * (Cc + extra) * plane
    flat = torch.full((n + 8,), SENT, device=DEV, dtype=torch.float32)
    assert flat.data_ptr() % 16 == 0
    o = 1 if odd else 0
    full = flat[o:o + n].view(B, Cc + extra, *shape[2:])
    view = full[:, SLICE_LO:SLICE_LO + Cc] if extra else full
    if src is not None:
        view.copy_(src)
    return flat, view


def _pad(shape, src=None):
    """(flat, view): a contiguous device tensor of `shape` 32 floats inside a sentinel buffer"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 64,), SENT, device=DEV, dtype=torch.float32)
    view = flat[32:32 + n].view(*shape)
    if src is not None:
        view.copy_(src)
    return flat, view


def _guard_intact(flat, view, what):
    """every element of `flat` outside `view` still holds the sentinel, bit for bit"""
    cur = flat.clone()
    cur.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    ok = torch.equal(cur.view(torch.int32), torch.full_like(cur, SENT).view(torch.int32))
    assert ok, f"{what}: elements outside the operand were written"
