"""Training-path building blocks, one table row per launch branch of their host launchers: every row runs the HIP kernel through its
autograd Function or train_ops wrapper (the raw idiff_* entry point only where the wrapper hides a flag: accumulate, a null dfilm) and
compares it with torch's own float64 kernels of the plain formula.  Each row proves that it reached the branch its id names through a
query the library already exposes (the wgrad algorithm, the bgemm workspace size, the chan-LN workgroup count) or, where none exists,
cites the launcher condition it satisfies.

Metric: max|got - ref| / max|ref| per output tensor (_rel); on the rows with a tail (a size that is not a multiple of the tile or lane
width) also elementwise |got - ref| <= tol * max|ref| on the last partial tile alone, so that a wrong tail cannot hide behind a large
interior.  Tolerances come from fp32 accumulation: 1e-5 for elementwise maps and short reductions, 5e-5 for reductions over >= 65 536
terms; a row that needs more says why."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops, train_ops as T  # noqa: E402
from instancediff_amd._lib import check  # noqa: E402
from instancediff_amd.ops import _bs, _p, _stream  # noqa: E402

DEV = "cuda"
EPS = 1e-5
RED = 5e-5  # reductions over >= 65 536 terms


def _cond(tol, off, spr):
    """the large-magnitude rows (values offset +- spread): x - mean loses log2(offset / spread) bits, so every fp32 rounding of the
    normalisation is amplified by offset / spread; four such roundings (mean, variance, x - mean, the product with rstd)"""
    return max(tol, 4 * (abs(off) / spr) * 2.0 ** -24) if off else tol


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, g, offset=0.0, spread=1.0):
    return torch.randn(shape, generator=g) * spread + offset


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _check(row, name, got, ref, tol, tail=None):
    """normwise max error of one output; with `tail` (an index into both) also every element of that region against tol * max|ref|"""
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    scale = float(ref.abs().max().clamp_min(1e-12))
    e = float((got - ref).abs().max()) / scale
    msg = f"{row} {name}: rel {e:.2e} (tol {tol:.0e})"
    et = None
    if tail is not None:
        et = float((got[tail] - ref[tail]).abs().max()) / scale
        msg += f", tail {et:.2e}"
    print(msg)
    assert e <= tol, msg
    if tail is not None:
        assert et <= tol, msg


def _slice(shape, extra, g, offset=0.0, spread=1.0):
    """an NCHW tensor whose samples are a channel slice [1:1+C] of a bigger buffer when extra > 0 (batch stride > C*H*W)"""
    B, Cc = shape[:2]
    if not extra:
        return _rand(shape, g, offset, spread).to(DEV)
    big = _rand((B, Cc + extra) + tuple(shape[2:]), g, offset, spread).to(DEV)
    return big[:, 1:1 + Cc]


def _in_slice(t, extra):
    """t (a host tensor) on the device, as channels [1, 1 + C) of a wider buffer whose other channels hold other values when extra > 0
    (batch stride (C + extra) * H * W; offset H * W floats from the buffer's start)"""
    if not extra:
        return t.to(DEV)
    B, Cc = t.shape[:2]
    big = _rand((B, Cc + extra) + tuple(t.shape[2:]), _g(12345), 5.0).to(DEV)
    v = big[:, 1:1 + Cc]
    v.copy_(t)
    return v


# =====================================================================================================
# channel LayerNorm backward (idiff_chan_layernorm_bwd via ChanLayerNormFn)
#   C <= 256 with parameter gradients: chan_ln_bwd_fused_kernel<JMAX> (JMAX = 32 for C <= 128, 64 above), tpw = CLN_TPW = 8 tiles
#   of 64 pixels per workgroup once the sample has >= 64 tiles (HW > 4032), G = ceil(ntiles / tpw) workgroups per sample;
#   C > 256: chan_ln_bwd_dx_kernel + chan_ln_bwd_param_kernel + pair_batch_sum_kernel.
# =====================================================================================================
CLN_ROWS = [
    # id, B, C, H, W, extra channels (x is a channel slice), offset, spread, expected G, tpw
    ("cln_bwd-fused32-tpw1-single-partial-tile-B1", 1, 100, 7, 9, 0, 0.0, 1.0, 1, 1),
    ("cln_bwd-fused32-tpw1-B3-slice", 3, 32, 12, 20, 5, 0.0, 1.0, 4, 1),
    ("cln_bwd-fused32-tpw8-partial", 3, 64, 65, 67, 0, 0.0, 1.0, 9, 8),
    ("cln_bwd-fused64-tpw8-partial", 1, 200, 65, 67, 0, 0.0, 1.0, 9, 8),
    ("cln_bwd-fused64-tpw8-partial-B3-slice", 3, 256, 63, 69, 3, 0.0, 1.0, 9, 8),
    ("cln_bwd-fused64-tpw8-product-C256-HW65536", 2, 256, 256, 256, 0, 0.0, 1.0, 128, 8),
    ("cln_bwd-fused64-tpw8-offset10", 2, 256, 65, 67, 0, 10.0, 0.1, 9, 8),
    ("cln_bwd-unfused-C300-B3-slice", 3, 300, 25, 41, 2, 0.0, 1.0, None, None),
    ("cln_bwd-unfused-C300-B1-offset10", 1, 300, 17, 19, 0, 10.0, 0.1, None, None),
]


@pytest.mark.parametrize("row,B,C,H,W,extra,off,spr,G,tpw", [pytest.param(*r, id=r[0]) for r in CLN_ROWS])
def test_chan_layernorm(row, B, C, H, W, extra, off, spr, G, tpw):
    """The fused rows witness G (and so tpw = ceil(ntiles / G)) through idiff_chan_layernorm_bwd_ws_floats = 2 B C G; the unfused rows
    satisfy the launcher's `C > 256` (no fused kernel, thread-per-pixel dx kernel + per-plane parameter kernel)."""
    lib = _lib.load()
    g = _g(100 + C + H)
    HW = H * W
    x = _slice((B, C, H, W), extra, g, off, spr)
    ga, be = _rand((C,), g, 1.0, 0.5), _rand((C,), g)
    dy = _rand((B, C, H, W), g)
    ntiles = (HW + 63) // 64
    if G is not None:
        assert C <= 256
        assert lib.idiff_chan_layernorm_bwd_ws_floats(B, C, HW) // (2 * B * C) == G
        assert -(-ntiles // G) == tpw and (tpw > 1) == (ntiles >= 64)
    else:
        assert C > 256
    rx = x.detach().double().requires_grad_(True)
    rg, rb = ga.double().to(DEV).requires_grad_(True), be.double().to(DEV).requires_grad_(True)
    ref = F.layer_norm(rx.permute(0, 2, 3, 1), (C,), rg, rb, EPS).permute(0, 3, 1, 2)
    ref.backward(dy.double().to(DEV))
    px, pg, pb = x.detach().requires_grad_(True), ga.to(DEV).requires_grad_(True), be.to(DEV).requires_grad_(True)
    out = T.ChanLayerNormFn.apply(px, pg, pb, EPS)
    out.backward(dy.to(DEV))
    # the last workgroup of the fused form (tpw tiles of 64 pixels, the last one partial) / the last 256-pixel block of the unfused
    # thread-per-pixel dx kernel (grid (HW + 255) / 256)
    p0 = (G - 1) * tpw * 64 if G is not None else (HW - 1) // 256 * 256
    tail = (slice(None), slice(None), slice(p0, None))
    big = HW * B >= 65536
    _check(row, "out", out, ref, _cond(1e-5, off, spr))
    _check(row, "dx", px.grad.reshape(B, C, HW), rx.grad.reshape(B, C, HW), _cond(1e-5, off, spr), tail)
    _check(row, "dgamma", pg.grad, rg.grad, _cond(RED if big else 1e-5, off, spr))
    _check(row, "dbeta", pb.grad, rb.grad, RED if big else 1e-5)


def _cln_bwd_raw(dy, x, gamma, mr, dg, db, accumulate):
    """ChanLayerNormFn.backward with the `accumulate` flag it hides (the parameter-sum kernels add into dg / db)"""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    dx = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    ws = torch.empty((lib.idiff_chan_layernorm_bwd_ws_floats(B, Cc, H * W),), device=x.device, dtype=torch.float32)
    check(lib.idiff_chan_layernorm_bwd(_p(dy), _bs(dy), _p(x), _bs(x, "x"), _p(gamma), _p(mr), _p(dx), _bs(dx), _p(dg), _p(db), _p(ws), B, Cc,
                                       H * W, accumulate, _stream()), "chan_layernorm_bwd")
    return dx


@pytest.mark.parametrize("row,B,C,H,W", [
    pytest.param("cln_bwd-fused64-tpw8-accumulate", 3, 160, 65, 67, id="cln_bwd-fused64-tpw8-accumulate"),
    pytest.param("cln_bwd-unfused-C300-accumulate", 2, 300, 9, 11, id="cln_bwd-unfused-C300-accumulate")])
def test_chan_layernorm_accumulate(row, B, C, H, W):
    """accumulate = 1: pair_rows_sum_kernel (fused, C <= 256) / pair_batch_sum_kernel (C > 256) add into dgamma / dbeta"""
    g = _g(110 + C)
    x, dy = _rand((B, C, H, W), g).to(DEV), _rand((B, C, H, W), g).to(DEV)
    ga, be = _rand((C,), g, 1.0, 0.5).to(DEV), _rand((C,), g).to(DEV)
    dg0, db0 = _rand((C,), g).to(DEV), _rand((C,), g).to(DEV)
    rx = x.double().requires_grad_(True)
    rg, rb = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    F.layer_norm(rx.permute(0, 2, 3, 1), (C,), rg, rb, EPS).permute(0, 3, 1, 2).backward(dy.double())
    _, mr = ops.chan_layernorm(x, ga, be, EPS, want_mean_rstd=True)
    dg, db = dg0.clone(), db0.clone()
    dx = _cln_bwd_raw(dy, x, ga, mr, dg, db, 1)
    _check(row, "dx", dx, rx.grad, 1e-5)
    _check(row, "dgamma(+)", dg, dg0.double() + rg.grad, 1e-5)
    _check(row, "dbeta(+)", db, db0.double() + rb.grad, 1e-5)


# =====================================================================================================
# channel L2 normalisation (idiff_chan_normalize_fwd / _bwd via ChanNormalizeFn): C <= 128 -> *_reg_kernel<32>, C <= 256 ->
# *_reg_kernel<64>, C > 256 -> thread-per-pixel kernels; [R, C, 1] token rows (HW = 1, x batch stride C) as in unet_autograd.
# No witness exists: each row's id names the C range of the launcher it satisfies.
# =====================================================================================================
CNORM_ROWS = [
    # id, shape, extra channels, offset, spread
    ("cnorm-reg32-C100-single-partial-tile-B1", (1, 100, 7, 9), 0, 0.0, 1.0),
    ("cnorm-reg32-C32-B3-slice", (3, 32, 33, 35), 4, 0.0, 1.0),
    ("cnorm-reg64-C200-partial-B3-slice", (3, 200, 37, 41), 3, 0.0, 1.0),
    ("cnorm-reg64-C256-HW65536", (2, 256, 256, 256), 0, 0.0, 1.0),
    ("cnorm-reg64-C256-offset10", (2, 256, 31, 33), 0, 10.0, 0.1),
    ("cnorm-thread-C300-B3-slice", (3, 300, 19, 53), 2, 0.0, 1.0),
    ("cnorm-rows-R37-C256", (37, 256, 1), 0, 0.0, 1.0),
    ("cnorm-rows-R5-C100", (5, 100, 1), 0, 0.0, 1.0),
    ("cnorm-rows-R3-C300", (3, 300, 1), 0, 0.0, 1.0),
]


@pytest.mark.parametrize("row,shape,extra,off,spr", [pytest.param(*r, id=r[0]) for r in CNORM_ROWS])
def test_chan_normalize(row, shape, extra, off, spr):
    """C <= 128 / 128 < C <= 256 / C > 256 select the three kernel pairs of idiff_chan_normalize_fwd/_bwd (`if (C <= 128) .. else if
    (C <= 256) .. else`); a 3-D [R, C, 1] input is passed with batch stride C * HW = C (ChanNormalizeFn)."""
    g = _g(200 + shape[1])
    x = _slice(shape, extra, g, off, spr) if len(shape) == 4 else _rand(shape, g, off, spr).to(DEV)
    dy = _rand(shape, g).to(DEV)
    rx = x.detach().double().requires_grad_(True)
    ref = F.normalize(rx, dim=1)
    ref.backward(dy.double())
    px = x.detach().requires_grad_(True)
    out = T.ChanNormalizeFn.apply(px)
    out.backward(dy)
    B, Cc = shape[:2]
    HW = math.prod(shape[2:])
    tail = (slice(None), slice(None), slice(((HW - 1) // 64) * 64, None))
    _check(row, "out", out.reshape(B, Cc, HW), ref.reshape(B, Cc, HW), 1e-5, tail)
    _check(row, "dx", px.grad.reshape(B, Cc, HW), rx.grad.reshape(B, Cc, HW), 1e-5, tail)


# =====================================================================================================
# LayerNorm over rows (idiff_layernorm_rows_bwd via LayerNormRowsFn): ln_rows_bwd_dx_kernel (a wave per row, 4 rows per workgroup,
# lane-strided over C) + ln_rows_bwd_param_kernel (16 columns x 16 row lanes per workgroup).  No witness: one kernel pair, the rows
# cover its tails.
# =====================================================================================================
LNR_ROWS = [
    # id, R, C, extra columns (x is a column slice of a wider matrix), offset, spread
    ("lnr-C256-R1001", 1001, 256, 0, 0.0, 1.0),
    ("lnr-C512-R7", 7, 512, 0, 0.0, 1.0),
    ("lnr-C200-R13-colslice", 13, 200, 24, 0.0, 1.0),
    ("lnr-C100-R1", 1, 100, 0, 0.0, 1.0),
    ("lnr-C96-R70001-param-long", 70001, 96, 0, 0.0, 1.0),
    ("lnr-C256-R515-offset10", 515, 256, 0, 10.0, 0.1),
]


@pytest.mark.parametrize("row,R,C,extra,off,spr", [pytest.param(*r, id=r[0]) for r in LNR_ROWS])
def test_layernorm_rows(row, R, C, extra, off, spr):
    """R % 4 != 0: the last dx workgroup holds fewer than 4 row waves (`r >= R` returns); C % 64 != 0: the last lane pass is partial;
    C % 16 != 0: the last parameter workgroup holds fewer than CS_COLS = 16 columns; R = 70 001 rows walked by 16 row lanes."""
    g = _g(300 + C + R)
    if extra:
        x = _rand((R, C + extra), g, off, spr).to(DEV)[:, 3:3 + C]
    else:
        x = _rand((R, C), g, off, spr).to(DEV)
    ga, be = _rand((C,), g, 1.0, 0.5).to(DEV), _rand((C,), g).to(DEV)
    dy = _rand((R, C), g).to(DEV)
    rx = x.detach().double().requires_grad_(True)
    rg, rb = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    ref = F.layer_norm(rx, (C,), rg, rb, EPS)
    ref.backward(dy.double())
    px, pg, pb = x.detach().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    out = T.LayerNormRowsFn.apply(px, pg, pb, EPS)
    out.backward(dy)
    tail = (slice((R - 1) // 4 * 4, None), slice((C - 1) // 64 * 64, None))
    _check(row, "out", out, ref, _cond(1e-5, off, spr))
    _check(row, "dx", px.grad, rx.grad, _cond(1e-5, off, spr), tail)
    red = RED if R >= 65536 else 1e-5
    _check(row, "dgamma", pg.grad, rg.grad, _cond(red, off, spr), slice((C - 1) // 16 * 16, None))
    _check(row, "dbeta", pb.grad, rb.grad, red, slice((C - 1) // 16 * 16, None))


# =====================================================================================================
# row softmax (idiff_softmax_rows_fwd / _bwd via SoftmaxRowsFn): a workgroup of 256 threads per row, strided over N
# =====================================================================================================
SMX_ROWS = [
    # id, R, N, scale, logit range (uniform in +-range; None: standard normal)
    ("softmax-N50-R1", 1, 50, 0.3, None),
    ("softmax-N300-R37", 37, 300, 0.125, None),
    ("softmax-N4099-R33", 33, 4099, 0.125, None),
    ("softmax-N16384-R8", 8, 16384, 0.125, None),
    ("softmax-N1000-R16-logits60", 16, 1000, 1.0, 60.0),
    ("softmax-N4099-R5-logits60", 5, 4099, 1.0, 60.0),
]


@pytest.mark.parametrize("row,R,N,scale,rng", [pytest.param(*r, id=r[0]) for r in SMX_ROWS])
def test_softmax_rows(row, R, N, scale, rng):
    """N > 256 and N % 256 != 0: the last pass of every thread's stride is partial (256 threads per row)"""
    g = _g(400 + N)
    if rng is None:
        x = _rand((R, N), g, 0.0, 3.0).to(DEV)
    else:
        x = ((torch.rand((R, N), generator=g) * 2 - 1) * rng).to(DEV)
    dy = _rand((R, N), g).to(DEV)
    rx = x.double().requires_grad_(True)
    ref = (rx * scale).softmax(-1)
    ref.backward(dy.double())
    px = x.clone().requires_grad_(True)
    out = T.SoftmaxRowsFn.apply(px, scale)
    out.backward(dy)
    tail = (slice(None), slice((N - 1) // 256 * 256, None))
    _check(row, "p", out, ref, 1e-5, tail)
    _check(row, "dx", px.grad, rx.grad, 1e-5, tail)


# =====================================================================================================
# batched GEMM (idiff_bgemm via BgemmFn / train_ops.bgemm): tile 32x128 for M <= 32, 64x64 otherwise; split over K (pick_nsplit > 1:
# K >= 2048 and < 512 output tiles) into per-split partials that bgemm_reduce_kernel sums (and applies beta to).
# Witness: idiff_bgemm_ws_floats(M, N, K, batch) > 0 exactly when the product is split.
# =====================================================================================================
def _nsplit(M, N, K, batch):
    ws = _lib.load().idiff_bgemm_ws_floats(M, N, K, batch)
    return ws // (batch * M * N) if ws else 1


def _mat(A, t):
    return A.transpose(-1, -2) if t else A


BGEMM_ROWS = [
    # id, batch, M, N, K, transA, transB, alpha, beta, ldc pad, expected split count (1 = none)
    ("bgemm-split-product-M5-N256-K65536-B1", 1, 5, 256, 65536, False, True, 1.0, 0.0, 0, 128),
    ("bgemm-split-M20-N256-K65536-B3-tA", 3, 20, 256, 65536, True, False, 1.0, 0.0, 0, 128),
    ("bgemm-split-kper-short-last-K5000", 1, 20, 256, 5000, False, False, 0.5, 0.0, 0, 9),
    ("bgemm-split-kper-empty-last-K65600", 1, 20, 200, 65600, False, True, 1.0, 0.0, 0, 128),
    ("bgemm-split-64x64-M100-N77-K8191-B2-beta1-ldc", 2, 100, 77, 8191, True, True, 0.7, 1.0, 13, 15),
    ("bgemm-split-M32-N130-K2048-B3-beta1-ldc", 3, 32, 130, 2048, False, False, 1.0, 1.0, 6, 4),
    ("bgemm-nosplit-32x128-M20-N300-K100-B3", 3, 20, 300, 100, False, True, 1.0, 0.0, 0, 1),
    ("bgemm-nosplit-32x128-M1-N1-K1", 1, 1, 1, 1, False, False, 1.0, 0.0, 0, 1),
    ("bgemm-nosplit-64x64-M100-N77-K2047-beta1-ldc", 1, 100, 77, 2047, True, False, 1.0, 1.0, 5, 1),
    ("bgemm-nosplit-K2048-561-tiles", 1, 1030, 2050, 2048, False, False, 1.0, 0.0, 0, 1),
]


@pytest.mark.parametrize("row,batch,M,N,K,tA,tB,alpha,beta,pad,ns", [pytest.param(*r, id=r[0]) for r in BGEMM_ROWS])
def test_bgemm(row, batch, M, N, K, tA, tB, alpha, beta, pad, ns):
    """C[b] = alpha op(A[b]) op(B[b]) + beta C[b] through train_ops.bgemm, C a strided view (row stride N + pad, batch stride
    (M + 1) * ldc) where pad > 0; beta = 1 is applied in bgemm_reduce_kernel when split."""
    assert _nsplit(M, N, K, batch) == ns, "the row no longer reaches the branch it names"
    g = _g(500 + M + N + K)
    A = _rand((batch, K, M) if tA else (batch, M, K), g).to(DEV)
    Bm = _rand((batch, N, K) if tB else (batch, K, N), g).to(DEV)
    ldc = N + pad
    sC = (M + 1) * ldc if pad else M * N
    buf = _rand((batch * sC + 7,), g).to(DEV)
    c0 = buf.clone()
    out = buf[:batch * sC].view(batch, -1)[:, :M * ldc].view(batch, M, ldc)[:, :, :N] if pad else buf[:batch * M * N].view(batch, M, N)
    T.bgemm(A, Bm, M, N, K, A.stride(1), Bm.stride(1), tA, tB, A.stride(0), Bm.stride(0), batch, out=out, alpha=alpha, beta=beta,
            ldc=ldc if pad else None, sC=sC if pad else None)
    ref = alpha * (_mat(A.double(), tA) @ _mat(Bm.double(), tB))
    view = (lambda t: t[:batch * sC].view(batch, -1)[:, :M * ldc].view(batch, M, ldc)[:, :, :N]) if pad else \
        (lambda t: t[:batch * M * N].view(batch, M, N))
    if beta:
        ref = ref + beta * view(c0).double()
    tm, tn = (32, 128) if M <= 32 else (64, 64)
    tail = (slice(None), slice((M - 1) // tm * tm, None), slice((N - 1) // tn * tn, None))
    tol = RED if K >= 65536 else 1e-5
    _check(row, "C", out, ref, tol, tail)
    # nothing outside the C view was written
    mask = torch.ones_like(buf, dtype=torch.bool)
    view(mask).fill_(False)
    assert torch.equal(buf[mask], c0[mask]), f"{row}: bgemm wrote outside C"


@pytest.mark.parametrize("row,batch,M,Cc,N,tB", [
    pytest.param("bgemm_fn-score-bwd-split-M20-K65536-B2", 2, 20, 256, 65536, False, id="bgemm_fn-score-bwd-split-M20-K65536-B2"),
    pytest.param("bgemm_fn-score-bwd-split-M7-K12288-B1-tB", 1, 7, 256, 12288, True, id="bgemm_fn-score-bwd-split-M7-K12288-B1-tB")])
def test_bgemm_fn_split_backward(row, batch, M, Cc, N, tB):
    """score = tvn [b, M, C] . fnm [b, C, N] (unet_autograd: C = 256 channels, N = H*W pixels): the forward is not split (K = C), the
    backward d tvn = dS . fnm^T is (K = N), d fnm = tvn^T . dS is not (K = M)."""
    # the (M, N, K) of the three products BgemmFn launches: forward (M, N, Cc); dA (M, Cc, N); dB (Cc, N, M), or (N, Cc, M) stored
    # transposed when tB
    assert _nsplit(M, N, Cc, batch) == 1, "forward"
    assert _nsplit(M, Cc, N, batch) > 1, "dA must be split"
    assert (_nsplit(N, Cc, M, batch) if tB else _nsplit(Cc, N, M, batch)) == 1, "dB"
    g = _g(550 + N)
    A = _rand((batch, M, Cc), g).to(DEV)
    Bm = _rand((batch, N, Cc) if tB else (batch, Cc, N), g).to(DEV)
    dC = _rand((batch, M, N), g).to(DEV)
    ra, rb = A.double().requires_grad_(True), Bm.double().requires_grad_(True)
    ref = (ra @ _mat(rb, tB)) * 0.5
    ref.backward(dC.double())
    pa, pb = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)
    out = T.BgemmFn.apply(pa, pb, False, tB, 0.5)
    out.backward(dC)
    _check(row, "C", out, ref, 1e-5)
    _check(row, "dA (split)", pa.grad, ra.grad, RED if N >= 65536 else 1e-5)
    _check(row, "dB", pb.grad, rb.grad, 1e-5)


# =====================================================================================================
# GroupNorm(+FiLM)+SiLU backward (idiff_gn_silu_bwd via train_ops.gn_silu_bwd): per-plane reduce, finalize (parameter / FiLM gradients,
# with want_sums the conv-bias gradient sum dh = rstd (g S1 - HW A - rstd Bq S3) and sum dy), apply with gx = clamp(ceil(HW / 1024),
# 1, 64) workgroups per plane looping over the rest.
# =====================================================================================================
GN_ROWS = [
    # id, B, C, groups, H, W, film, want_sums, dy channel slice, offset, spread
    ("gn_bwd-HW1000-film-B3", 3, 64, 8, 25, 40, True, False, 0, 0.0, 1.0),
    ("gn_bwd-HW63-nofilm-B1-sums", 1, 32, 8, 7, 9, False, True, 0, 0.0, 1.0),
    ("gn_bwd-HW65536-film-sums-B2", 2, 64, 8, 256, 256, True, True, 0, 0.0, 1.0),
    ("gn_bwd-HW70747-gridclamp-B1-sums-slice", 1, 16, 4, 263, 269, False, True, 5, 0.0, 1.0),
    ("gn_bwd-HW65536-offset10-sums-B2", 2, 32, 8, 256, 256, True, True, 0, 10.0, 0.1),
    ("gn_bwd-HW4100-offset10-sums-B3-slice", 3, 48, 8, 41, 100, False, True, 3, 10.0, 0.1),
]


def _gn_inputs(B, C, G, H, W, film, extra, off, spr, seed):
    g = _g(seed)
    h = _rand((B, C, H, W), g, off, spr)
    # per-channel offsets inside a group make the plane sums S3 = sum (h - mean) non-trivial
    h = h + (spr * 0.5) * _rand((1, C, 1, 1), g)
    dy = _slice((B, C, H, W), extra, g)
    gam, bet = _rand((C,), g, 1.0, 0.3), _rand((C,), g, 0.0, 0.3)
    fl = _rand((B, 2 * C), g, 0.0, 0.3) if film else None
    hd = h.double().to(DEV)
    hv = hd.reshape(B, G, -1)
    mean, var = hv.mean(-1), hv.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    mr = torch.stack([mean, rstd], -1).float().contiguous()
    cpg = C // G
    mc, rc = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    gd, bd = gam.double().to(DEV), bet.double().to(DEV)
    sc = 1 + fl[:, :C].double().to(DEV) if film else torch.ones((B, C), dtype=torch.float64, device=DEV)
    sh = fl[:, C:].double().to(DEV) if film else torch.zeros((B, C), dtype=torch.float64, device=DEV)
    a = (sc * gd * rc).float().contiguous()
    b = (sc * (bd - gd * mc * rc) + sh).float().contiguous()
    hdev = _in_slice(h, extra + 1 if extra else 0)  # the '-slice' rows: h a channel slice as well (h_bstride above C H W)
    if extra:
        assert _bs(hdev) == (C + extra + 1) * H * W and _bs(dy) == (C + extra) * H * W
    return hdev, dy, gam.to(DEV), bet.to(DEV), (fl.to(DEV) if film else None), a, b, mr


def _gn_ref(h, dy, gam, bet, fl, G):
    C = h.shape[1]
    rh = h.double().requires_grad_(True)
    rg, rb = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    rf = fl.double().requires_grad_(True) if fl is not None else None
    z = F.group_norm(rh, G, rg, rb, EPS)
    if rf is not None:
        z = z * (1 + rf[:, :C, None, None]) + rf[:, C:, None, None]
    F.silu(z).backward(dy.double())
    return rh.grad, rg.grad, rb.grad, (rf.grad if rf is not None else None)


@pytest.mark.parametrize("row,B,C,G,H,W,film,sums,extra,off,spr", [pytest.param(*r, id=r[0]) for r in GN_ROWS])
def test_gn_silu_bwd(row, B, C, G, H, W, film, sums, extra, off, spr):
    """HW % 256 != 0: the reduce's and apply's last strided pass is partial; HW > 65 536: gx is clamped at 64 and the apply loops;
    want_sums: dh_sum / dy_sum out of the finalize pass; film: d scale / d shift into dfilm [B, 2C]."""
    HW = H * W
    gx = min(max((HW + 1023) // 1024, 1), 64)
    if "gridclamp" in row:
        assert gx * 1024 < HW, "the apply grid must be clamped for this row"
    h, dy, gam, bet, fl, a, b, mr = _gn_inputs(B, C, G, H, W, film, extra, off, spr, 600 + HW + C)
    rdh, rdg, rdb, rdf = _gn_ref(h, dy, gam, bet, fl, G)
    res = T.gn_silu_bwd(dy, h, a, b, mr, gam, bet, fl, G, want_sums=sums)
    dh, dg, db, df = res[:4]
    tail = (slice(None), slice(None), slice(((HW - 1) // 256) * 256, None))
    red = RED if HW >= 65536 else 1e-5
    _check(row, "dh", dh.reshape(B, C, HW), rdh.reshape(B, C, HW), _cond(1e-5, off, spr), tail)
    _check(row, "dgamma", dg, rdg, _cond(red, off, spr))
    _check(row, "dbeta", db, rdb, _cond(red, off, spr))
    if film:
        _check(row, "dfilm", df, rdf, _cond(red, off, spr))
    else:
        assert df is None
    if sums:
        _check(row, "dh_sum", res[4], rdh.sum((0, 2, 3)), _cond(red, off, spr))
        _check(row, "dy_sum", res[5], dy.double().sum((2, 3)), red)


def test_gn_silu_bwd_film_without_dfilm():
    """film given, dfilm = NULL (the raw entry point: the wrapper always asks for dfilm): the apply still scales by 1 + film"""
    row = "gn_bwd-film-no-dfilm-HW1000"
    B, C, G, H, W = 3, 32, 4, 20, 50
    lib = _lib.load()
    h, dy, gam, bet, fl, a, b, mr = _gn_inputs(B, C, G, H, W, True, 0, 0.0, 1.0, 650)
    rdh, rdg, rdb, _ = _gn_ref(h, dy, gam, bet, fl, G)
    dh = torch.empty_like(h)
    dg, db = torch.empty_like(gam), torch.empty_like(gam)
    ws = torch.empty((lib.idiff_gn_silu_bwd_ws_floats(B, C, G),), device=DEV, dtype=torch.float32)
    check(lib.idiff_gn_silu_bwd(_p(dy), _bs(dy), _p(h), _bs(h), _p(a), _p(b), _p(mr), _p(gam), _p(bet), _p(fl), fl.stride(0), _p(dh), _bs(dh),
                                _p(dg), _p(db), None, 0, _p(ws), B, C, G, H * W, 0, None, None, _stream()), "gn_silu_bwd")
    _check(row, "dh", dh, rdh, 1e-5)
    _check(row, "dgamma", dg, rdg, 1e-5)
    _check(row, "dbeta", db, rdb, 1e-5)


# =====================================================================================================
# conv weight gradient, the non-Winograd branches of idiff_conv2d_wgrad: direct implicit GEMM (tile 2^twl x 128/2^twl pixels, twl =
# 3 / 4 / 5 for Wout < 16 / < 32 / >= 32; THIN for Cout <= 16; CK = 8 for Cin <= 8) and the streaming 1x1 kernel (Cout % 64 == 0,
# HW % 128 == 0, 16-byte aligned operands).  The Winograd kernels are reached only by shapes none of these rows has (Cout % 64 == 0,
# Cin % 16 == 0, Wout % 16 == 0), so the direct rows need no environment switch.  Witness: idiff_conv2d_wgrad_last_algo().
# The Winograd kernels have their own table, wgrad_wino_rows.py (test_wgrad_wino_gpu.py, mirrored on the CPU by test_wgrad_wino_cpu.py):
# splits that own several chunks, empty splits, prologue-table reloads inside a share, sliced operands, the dY-alignment rungs.
# =====================================================================================================
WG_ROWS = [
    # id, B, C0, C1, Cout, Hin, Win, ks, mode, prologue, dy misaligned, accumulate, expected algo, extra channels (src0, src1 and dy are
    # channel slices [1, 1 + C) of wider buffers: batch strides above C H W, as _samples_contiguous hands a concat source's gradient on)
    ("wg3-direct-tw8-partial-B1", 1, 24, 0, 40, 19, 13, 3, 0, False, False, False, 0, 0),
    ("wg3-direct-tw16-partial-B3", 3, 32, 0, 64, 13, 23, 3, 0, False, False, False, 0, 0),
    ("wg3-direct-tw32-partial-B3-two-sources", 3, 16, 8, 48, 7, 45, 3, 0, False, False, False, 0, 0),
    ("wg3-direct-thin-cout5", 2, 64, 0, 5, 33, 33, 3, 0, False, False, False, 0, 0),
    ("wg3-direct-thin-cin5-cout16", 2, 5, 0, 16, 37, 37, 3, 0, False, False, False, 0, 0),
    ("wg3-direct-ups-cin6", 1, 6, 0, 24, 9, 11, 3, 1, False, False, False, 0, 0),
    ("wg3-direct-ups-cin40-two-sources-B3", 3, 24, 16, 64, 7, 13, 3, 1, False, False, False, 0, 0),
    ("wg3-direct-gnsilu-prologue-B3", 3, 48, 0, 40, 21, 21, 3, 0, True, False, False, 0, 0),
    ("wg3-direct-ups-gnsilu-prologue", 2, 16, 0, 24, 6, 10, 3, 1, True, False, False, 0, 0),
    ("wg3-direct-tw16-partial-accumulate", 3, 32, 0, 64, 13, 23, 3, 0, False, False, True, 0, 0),
    ("wg1-direct-cout40", 2, 70, 0, 40, 17, 19, 1, 0, False, False, False, 0, 0),
    ("wg1-direct-cout64-hw225", 3, 48, 0, 64, 15, 15, 1, 0, False, False, False, 0, 0),
    ("wg1-direct-cout64-dy-unaligned", 2, 48, 0, 64, 16, 16, 1, 0, False, True, False, 0, 0),
    ("wg1-direct-odd-image-cin7-cout5", 1, 7, 0, 5, 11, 13, 1, 0, False, False, False, 0, 0),
    ("wg1-direct-gnsilu-prologue", 2, 40, 0, 64, 16, 16, 1, 0, True, False, False, 0, 0),
    ("wg1-stream-cin48-B3", 3, 48, 0, 64, 32, 32, 1, 0, False, False, False, 2, 0),
    ("wg1-stream-accumulate", 2, 64, 0, 128, 16, 8, 1, 0, False, False, True, 2, 0),
    ("wg1-unshuffle-direct-cout40", 2, 6, 0, 40, 26, 22, 1, 2, False, False, False, 0, 0),
    ("wg1-unshuffle-stream", 1, 4, 0, 64, 32, 64, 1, 2, False, False, False, 2, 0),
    ("wg7-direct-odd-B3-split", 3, 3, 0, 64, 32, 32, 7, 0, False, False, False, 0, 0),
    ("wg3-direct-tw16-partial-B3-two-sources-sliced", 3, 16, 8, 48, 13, 23, 3, 0, False, False, False, 0, 3),
    ("wg3-direct-gnsilu-prologue-sliced", 2, 48, 0, 40, 21, 21, 3, 0, True, False, False, 0, 2),
    ("wg3-direct-ups-two-sources-B1-sliced", 1, 24, 16, 64, 7, 13, 3, 1, False, False, False, 0, 5),
    ("wg1-direct-cout40-B3-sliced", 3, 70, 0, 40, 17, 19, 1, 0, False, False, False, 0, 3),
    ("wg1-stream-cin48-B3-sliced", 3, 48, 0, 64, 32, 32, 1, 0, False, False, False, 2, 3),
    ("wg1-stream-two-sources-sliced", 2, 64, 32, 64, 16, 16, 1, 0, False, False, False, 2, 4),
    ("wg1-unshuffle-stream-sliced", 2, 4, 0, 64, 32, 64, 1, 2, False, False, False, 2, 3),
    ("wg7-direct-odd-B3-sliced", 3, 3, 0, 64, 32, 32, 7, 0, False, False, False, 0, 2),
]


@pytest.mark.parametrize("row,B,C0,C1,Cout,Hin,Win,ks,mode,pro,unal,acc,algo,slc", [pytest.param(*r, id=r[0]) for r in WG_ROWS])
def test_conv_wgrad(row, B, C0, C1, Cout, Hin, Win, ks, mode, pro, unal, acc, algo, slc):
    """dW through train_ops.conv2d_wgrad (fp32 operands) against autograd of F.conv2d over the gathered input (virtual concat, nearest
    x2 upsample, pixel-unshuffle, GN-SiLU prologue silu(a x + b) per (sample, channel)); accumulate adds into a prefilled dW"""
    lib = _lib.load()
    g = _g(700 + C0 + Cout + Hin)
    x0 = _rand((B, C0, Hin, Win), g)
    x1 = _rand((B, C1, Hin, Win), g) if C1 else None
    pa = _rand((B, C0), g, 0.5, 0.5) if pro else None
    pb = _rand((B, C0), g, 0.0, 0.5) if pro else None
    xin = x0.double()
    if pro:
        xin = F.silu(pa.double()[:, :, None, None] * xin + pb.double()[:, :, None, None])
    if C1:
        xin = torch.cat([xin, x1.double()], 1)
    if mode == ops.CONV_UPSAMPLE2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    elif mode == ops.CONV_UNSHUFFLE2:
        xin = F.pixel_unshuffle(xin, 2)
    Cin = xin.shape[1]
    Hout, Wout = xin.shape[2:]
    dy = _rand((B, Cout, Hout, Wout), g)
    rw = torch.zeros((Cout, Cin, ks, ks), dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, rw, padding=ks // 2).backward(dy.double())
    dw0 = _rand((Cout, Cin, ks, ks), g)
    ref = rw.grad + (dw0.double() if acc else 0)
    if unal:  # dy one float past a 16-byte boundary: the streaming kernel's float4 loads do not apply
        buf = torch.empty((dy.numel() + 1,), device=DEV)
        dyd = buf[1:].view(dy.shape)
        dyd.copy_(dy)
        assert dyd.data_ptr() % 16 != 0
    else:
        dyd = _in_slice(dy, slc)
    x0d, x1d = _in_slice(x0, slc), (_in_slice(x1, slc) if C1 else None)
    if slc:
        for t in (x0d, x1d, dyd):
            if t is not None:
                assert _bs(t) == (t.shape[1] + slc) * t.shape[2] * t.shape[3]
    dw = dw0.to(DEV) if acc else None
    out = T.conv2d_wgrad(x0d, x1d, mode, ks, dyd, Cin, pro=(pa.to(DEV), pb.to(DEV)) if pro else None, dw=dw, accumulate=acc, operands="f32")
    assert lib.idiff_conv2d_wgrad_last_algo() == algo, "the row no longer reaches the branch it names"
    if ks == 7:  # the 7x7 form has only the direct geometry: its workspace is nsplit images of dW
        d = T._conv_desc(x0d, None, mode, ks, Cout)
        assert lib.idiff_conv2d_wgrad_ws_floats(ctypes.byref(d)) // (49 * Cin * Cout) > 1, "the 7x7 row must be split"
    if acc:
        assert out.data_ptr() == dw.data_ptr()
    # the last 64-channel output block and the last input-channel chunk (the partial ones where Cout, Cin are not multiples)
    ck = 64 if ks == 1 else (2 if ks == 7 else (8 if Cin <= 8 else 16))
    tail = (slice((Cout - 1) // 64 * 64, None), slice((Cin - 1) // ck * ck, None))
    red = RED if B * Hout * Wout >= 65536 else 1e-5
    _check(row, "dW", out.cpu(), ref, red, tail)


# =====================================================================================================
# MSE loss (idiff_mse_loss: a fixed grid of 256 partial sums) and Adam (idiff_adam_step: grid capped at 8192 workgroups x 256 threads,
# larger buffers loop)
# =====================================================================================================
@pytest.mark.parametrize("n", [pytest.param(1, id="mse-n1"), pytest.param(37, id="mse-n37"), pytest.param(255, id="mse-n255"),
                               pytest.param(65537, id="mse-n65537"), pytest.param(3 * 2 ** 20 + 3, id="mse-n3M-odd")])
def test_mse_loss(n):
    row = f"mse-n{n}"
    g = _g(800 + n % 1000)
    a, b = _rand((n,), g).to(DEV), _rand((n,), g).to(DEV)
    slot = torch.zeros(2, device=DEV)
    grad = T.mse_loss_and_grad(a, b, slot[0:1], weight=0.5)
    ra = a.double().requires_grad_(True)
    loss = F.mse_loss(ra, b.double())
    (0.5 * loss).backward()
    _check(row, "loss", slot[0:1], loss.detach().reshape(1), RED if n >= 65536 else 1e-5)
    assert float(slot[1]) == 0.0, "mse_loss wrote past its slot"
    _check(row, "grad", grad, ra.grad, 1e-5, slice((n - 1) // 4 * 4, None))


@pytest.mark.parametrize("n,wd", [pytest.param(3, 1e-2, id="adam-n3"), pytest.param(255, 1e-2, id="adam-n255"),
                                  pytest.param(256 * 8192 + 37, 0.0, id="adam-n-above-grid-cap"),
                                  pytest.param(3 * 256 * 8192 + 5, 0.0, id="adam-n-3x-grid-cap")])
def test_adam_step(n, wd):
    """n > 256 * 8192: adam_kernel's grid is capped (bgrid(n, 256, 8192)) and every thread loops; the tail past the last full pass is
    compared on its own.  Those rows run without weight decay: among millions of elements some g + wd p cancel to ~eps = 1e-8, where
    the fp32 update is ill-conditioned whatever the kernel does; the small rows (and test_train_gpu's Adam test) carry the decay."""
    row = f"adam-n{n}"
    g = _g(900 + n % 1000)
    p0 = _rand((n,), g)
    ref_p = p0.double().to(DEV).requires_grad_(True)
    ropt = torch.optim.Adam([ref_p], lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    pp = nn.Parameter(p0.clone().to(DEV))
    opt = T.FusedAdam([pp], lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    for it in range(3):
        gr = _rand((n,), g).to(DEV)
        ref_p.grad = gr.double()
        ropt.step()
        opt.zero_grad()
        pp.grad = gr
        opt.step()
    st = ropt.state[ref_p]
    f = opt._flat[0]
    cap = 256 * 8192
    tail = slice((n - 1) // cap * cap, None)
    _check(row, "exp_avg", f["m"], st["exp_avg"], 1e-5, tail)
    _check(row, "exp_avg_sq", f["v"], st["exp_avg_sq"], 1e-5, tail)
    _check(row, "p", pp.data, ref_p, 1e-6, tail)
    # every element's update (p - p0 ~ 6e-3) against the update's own scale, less the fp32 storage of p: three steps round p to
    # float at most half an ulp each, <= 1.5 * 2^-23 * |p| in all (an element the kernel skipped would be off by its whole update)
    p0d = p0.double().to(DEV)
    got, ref = pp.data.double(), ref_p.detach()
    du = float((ref - p0d).abs().max())
    excess = ((got - ref).abs() - 1.5 * 2.0 ** -23 * ref.abs()).clamp_min(0)
    e, et = float(excess.max()) / du, float(excess[tail].max()) / du
    print(f"{row} p - p0 beyond fp32 rounding of p: rel {e:.2e} (tol 1e-05), tail {et:.2e}")
    assert e <= 1e-5 and et <= 1e-5, (row, e, et)
