"""The Winograd weight-gradient kernels (wino_wgrad_kernel, F(2x2,3x3), csrc/conv_wino_wgrad.hip; wino4_wgrad_kernel, F(4x4,3x3),
csrc/conv_wino4_wgrad.hip) on shapes whose splits own SEVERAL chunks: the double-buffered steady state, the look-ahead loads, the
prologue-table reload where a share crosses into the next sample, uneven last shares and empty splits (wgrad_wino_rows.ROWS, mirrored
without a GPU by test_wgrad_wino_cpu.py), plus the dY-alignment rungs of the ladder down to the direct kernel.

Every row calls the raw idiff_conv2d_wgrad with a workspace of exactly idiff_conv2d_wgrad_ws_floats floats, prefilled with NaN (an
unwritten partial of an empty split would poison the sum), ws and dW inside sentinel guard bands that must stay bit-intact, and
compares dW with autograd of F.conv2d in float64 on the CPU over the plainly gathered input (wgrad_wino_ref.py).  No row's reference
is another kernel of this library.  idiff_conv2d_wgrad_last_algo() after the call equals the row's claim.  The split geometry is read
from what the launch wrote: exactly the claimed nsplit leading images of the workspace are free of NaN, the rest still all NaN, and the
all-zero images are exactly the claimed empty splits -- nsplit and empty give per = ceil(total / nsplit) and the shares, for both
kernels.  (ncob and ncib leave no trace in the workspace; a wrong one shows as wrong or unwritten blocks of dW.)

Metric: max|got - ref| / max|ref| over dW; the last 64-co block and the last (partial) ci block also element by element against
tol * max|ref of that block|, which is at most tol * max|ref|.  Tolerances are test_conv_wgrad_winograd_vs_fp64's: 1e-5 for F(2x2,3x3), 2e-5 for F(4x4,3x3) (1e-5 for the direct rows,
test_conv_wgrad's).  Prologue (silu_fast) and DC-offset rows take max(that, 4 x the error of the SAME formula evaluated in fp32 torch
on the CPU against the fp64 one); both numbers are printed.  No bound was chosen from what the kernels return.  The core rows are called
twice and must give bit-equal dW: the reduction order is fixed."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib  # noqa: E402
from instancediff_amd._lib import ConvDesc  # noqa: E402
from instancediff_amd.ops import _bs, _stream  # noqa: E402

from wgrad_wino_ref import make_inputs, reference  # noqa: E402
from wgrad_wino_rows import ROWS, SLICE_LO, TOL, dy_bstride, dy_offset_floats, expected, geometry, out_size, ws_splits  # noqa: E402

DEV = "cuda"
SENT = -777.25  # guard-band fill
IDS = [r["name"] for r in ROWS]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _pad(shape, fill=None):
    """(flat, view): a contiguous device tensor of `shape` 32 floats inside a sentinel buffer"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 64,), SENT, device=DEV, dtype=torch.float32)
    view = flat[32:32 + n].view(*shape)
    if fill is not None:
        view.fill_(fill)
    return flat, view


def _guard_intact(flat, view, what):
    """every element of `flat` outside `view` still holds the sentinel, bit for bit"""
    cur = flat.clone()
    cur.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    ok = torch.equal(cur.view(torch.int32), torch.full_like(cur, SENT).view(torch.int32))
    assert ok, f"{what}: elements outside the operand were written"


def _partials(ws, img):
    """(written, zero): the indices of the img-sized images of the NaN-prefilled workspace that hold no NaN at all, and of those that
    are all zero; an image that holds numbers AND NaN belongs to neither list and fails the caller's comparison"""
    v = ws.view(-1, img)
    nan = torch.isnan(v)
    clean, dirty = ~nan.any(1), nan.all(1)
    assert bool((clean | dirty).all()), "a partial image of the workspace was written in part"
    written = torch.nonzero(clean).flatten().tolist()
    zero = torch.nonzero(clean & (v == 0).all(1)).flatten().tolist()
    return written, zero


def _operand(t, extra, off=0):
    """t (a host tensor [B, C, H, W]) on the device: the channel slice [SLICE_LO, SLICE_LO + C) of a buffer with `extra` more channels
    whose other channels hold other values, starting `off` floats past a 16-byte boundary"""
    B, Cc, H, W = t.shape
    n = B * (Cc + extra) * H * W
    flat = torch.randn(n + 8, generator=torch.Generator().manual_seed(12345)).add_(5.0).to(DEV)
    assert flat.data_ptr() % 16 == 0
    full = flat[off:off + n].view(B, Cc + extra, H, W)
    v = full[:, SLICE_LO:SLICE_LO + Cc] if extra else full
    v.copy_(t)
    return v


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_wgrad_multi_chunk_row(row):
    lib = _lib.load()
    name = row["name"]
    assert row["claim"] == expected(row)
    g = geometry(row)
    algo, per, empty = g["algo"], g["per"], g["empty"]
    B, C0, C1, Cout = (row[k] for k in ("B", "C0", "C1", "Cout"))
    Cin = C0 + C1
    Hout, Wout = out_size(row)
    inp = make_inputs(row)
    ref = reference(row, inp)

    x0 = _operand(inp["src0"], row["slc"])
    x1 = _operand(inp["src1"], row["slc"]) if C1 else None
    dy = _operand(inp["dy"], row["slc"], row["dyoff"])
    assert (dy.data_ptr() % 16) // 4 == dy_offset_floats(row) % 4 and _bs(dy) == dy_bstride(row)
    keep = []
    d = ConvDesc()
    d.src0, d.src0_bstride, d.C0 = x0.data_ptr(), _bs(x0), C0
    if C1:
        d.src1, d.src1_bstride, d.C1 = x1.data_ptr(), _bs(x1), C1
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = B, row["Hin"], row["Win"], row["mode"], 3, Cout
    if row["pro"]:
        keep = [t.to(DEV).contiguous() for t in inp["pro"]]
        d.pro_a, d.pro_b = keep[0].data_ptr(), keep[1].data_ptr()

    # the workspace holds at least the nsplit partial images of the form the row claims (the query is an upper bound over the forms the
    # shape could get); what the launch really wrote is read from the NaN-prefilled workspace after the call (_partials)
    nws = lib.idiff_conv2d_wgrad_ws_floats(ctypes.byref(d))
    img = 9 * Cin * Cout
    assert nws % img == 0 and nws == ws_splits(row) * img and nws >= g["nsplit"] * img, (name, nws, ws_splits(row), g)

    def call():
        wsflat, ws = _pad((nws,), float("nan"))
        dwflat, dw = _pad((Cout, Cin, 3, 3))
        if row["acc"]:
            dw.copy_(inp["dw0"])
        rc = lib.idiff_conv2d_wgrad(ctypes.byref(d), ctypes.c_void_p(dy.data_ptr()), _bs(dy), ctypes.c_void_p(dw.data_ptr()), 1 if row["acc"] else 0,
                                    ctypes.c_void_p(ws.data_ptr()), _stream())
        assert rc == 0, (name, rc, lib.idiff_last_error())
        assert lib.idiff_conv2d_wgrad_last_algo() == algo == row["claim"][0], "the row no longer reaches the kernel it names"
        torch.cuda.synchronize()
        _guard_intact(wsflat, ws, f"{name} ws")
        _guard_intact(dwflat, dw, f"{name} dW")
        return dw.cpu(), _partials(ws, img)

    got, (written, zero) = call()
    # the split geometry, from what the launch wrote: exactly the first nsplit images of the workspace hold numbers, the rest is still
    # NaN; the all-zero images are exactly the partials of the empty splits, which are the last ones (a share that owns chunks sums
    # thousands of random products to something else than 0 in all 9 Cin Cout places)
    print(f"{name}: algo {algo}, claimed grid {g['ncob']} x {g['ncib']} x {g['nsplit']} splits, per {per}, empty {empty}, last share "
          f"{g['last_share']}, crossings {g['crossings']}; written: {len(written)} partial images, {len(zero)} of them all zero")
    assert written == list(range(g["nsplit"])), (name, "partial images written", written, "claimed nsplit", g["nsplit"])
    assert zero == list(range(g["used"], g["nsplit"])) and len(zero) == empty, (name, "all-zero partials", zero, "claimed empty", empty)
    base = TOL[algo]
    tol = base
    e32 = None
    if row["pro"] or row["dc"]:
        e32 = _rel(reference(row, inp, torch.float32), ref)
        tol = max(base, 4 * e32)
    got64 = got.double()
    scale = float(ref.abs().max())
    e = float((got64 - ref).abs().max()) / scale
    tails = [("last co block", (slice(Cout - 64, None),)), (f"last ci block ({Cin - (Cin - 1) // g['cib'] * g['cib']} of {g['cib']})",
                                                            (slice(None), slice((Cin - 1) // g["cib"] * g["cib"], None)))]
    msg = f"{name} dW: rel {e:.2e} (tol {tol:.2e}, project tol {base:.0e}" + (f", fp32-CPU error {e32:.2e}" if e32 is not None else "") + ")"
    worst = []
    for what, t in tails:  # against the block's OWN range (<= the tensor's, so this implies the bound on tol * max|ref| and asks more)
        assert got64[t].numel() > 0
        worst.append(float((got64[t] - ref[t]).abs().max()) / float(ref[t].abs().max()))
        msg += f", {what} {worst[-1]:.2e}"
    print(msg)
    assert math.isfinite(e) and e <= tol, msg
    assert all(w <= tol for w in worst), msg
    if row["core"]:
        assert torch.equal(call()[0].view(torch.int32), got.view(torch.int32)), f"{name}: two calls differ (the reduction order is fixed)"
