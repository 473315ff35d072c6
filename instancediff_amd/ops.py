"""Thin torch-tensor wrappers over the C ABI (include/idiff.h).  torch supplies device memory and the
stream; every arithmetic operation below runs in the hand-written HIP kernels.  No fallbacks."""
import contextlib
import ctypes as C
import functools
import math
import os
import threading

import torch

from . import _lib
from ._lib import ConvDesc, check

CONV_NORMAL, CONV_UPSAMPLE2, CONV_UNSHUFFLE2 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
SDE_STEP, SDE_MEAN, SDE_ODE = 0, 1, 2

# bench.py sets this to a list to time every conv launch with events on the launch stream (roofline leg)
PROFILE = None
# tests set this to a collections.Counter: (algo, ks, Cin, Cout, Hout, Wout) -> calls, to assert which kernel served a layer
ALGO_TRACE = None
# the same for the weight gradients of the training path (train_ops.conv2d_wgrad; idiff_conv2d_wgrad_last_algo())
WGRAD_TRACE = None


def launch_count():
    """kernel launches this library has enqueued so far in the process (replays of a captured graph enqueue none)"""
    return int(_lib.load().idiff_launch_count())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, name="tensor", dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.IdiffError(f"{name} must live on the GPU (the hot path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.IdiffError(f"{name} must be {dtype}, got {t.dtype}")


def _bs(t, name="tensor"):
    """batch stride of an NCHW tensor whose samples are contiguous (channel slices of a bigger buffer allowed)."""
    _chk(t, name)
    exp = 1
    for d in range(t.dim() - 1, 0, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            raise _lib.IdiffError(f"{name}: samples must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        exp *= t.shape[d]
    return t.stride(0) if t.shape[0] > 1 else max(exp, t.stride(0))


def _c(t, name="tensor", dtype=torch.float32):
    _chk(t, name, dtype)
    if t is not None and not t.is_contiguous():
        raise _lib.IdiffError(f"{name} must be contiguous")
    return t


# IDIFF_WINOGRAD=0 keeps every 3x3 conv on the direct implicit-GEMM kernel (A/B runs, parity bisection)
WINOGRAD = bool(int(os.environ.get("IDIFF_WINOGRAD", "1")))
# IDIFF_X3=0: no three-plane bf16 images of 1x1 weights are built, so every 1x1 conv stays on the f32 matrix cores
X3 = bool(int(os.environ.get("IDIFF_X3", "1")))
# IDIFF_WINOGRAD4=0 keeps the forward 3x3 convs off the F(4x4,3x3) kernel (they run F(2x2,3x3) or direct instead)
WINOGRAD4 = WINOGRAD and bool(int(os.environ.get("IDIFF_WINOGRAD4", "1")))
# IDIFF_WINOGRAD4_DGRAD=0 keeps the data-gradient convs of the backward pass on F(2x2,3x3)
WINOGRAD4_DGRAD = bool(int(os.environ.get("IDIFF_WINOGRAD4_DGRAD", "1")))


CONV_ALGO_DIRECT, CONV_ALGO_WINOGRAD, CONV_ALGO_STREAM1X1, CONV_ALGO_WINOGRAD4, CONV_ALGO_WINOGRAD4H, CONV_ALGO_X3 = 0, 1, 2, 3, 4, 5
CONV_ALGO_BF16 = 6  # opt-in: 3x3 operands rounded to bf16, fp32 sums (conv_operands("bf16"))
_ALGO_REQUEST = threading.local()
CONV_OPERANDS = ("f32", "bf16")
_OPERANDS = threading.local()


@contextlib.contextmanager
def conv_operands(kind):
    """Scope (this thread only) of the operand precision of the 3x3 convs issued inside: "f32" (the default, the parity path) or
    "bf16" -- the labelled reduced-precision variant (idiff_conv_desc.operands = 1): every gathered operand and weight is rounded once
    to bf16 after the fp32 gather, the products are summed in fp32, the epilogue stays fp32.  Layers that do not tile for the bf16
    kernel keep the fp32 kernels.  conv2d() and train_ops.conv2d_wgrad() read it; the training autograd Functions record it at forward
    time and hand it to their backward explicitly (autograd may run the backward on another thread)."""
    if kind not in CONV_OPERANDS:
        raise ValueError(f"conv operands must be one of {CONV_OPERANDS}, got {kind!r}")
    old = getattr(_OPERANDS, "kind", "f32")
    _OPERANDS.kind = kind
    try:
        yield
    finally:
        _OPERANDS.kind = old


def current_conv_operands():
    """the conv_operands() scope of the calling thread: 'f32' or 'bf16'"""
    return getattr(_OPERANDS, "kind", "f32")


@contextlib.contextmanager
def request_conv3x3_algo(algo):
    """Diagnostic / test scope (this thread only): every 3x3 conv2d() issued inside asks the library for `algo` through the per-call
    idiff_conv_desc.algo_request where the layer's shape tiles for it, e.g. the F(4x4,3x3) kernel on the small levels of a 64x64
    input (which the library's own choice leaves on F(2x2,3x3)).  The product path never enters this scope."""
    old = getattr(_ALGO_REQUEST, "algo", None)
    _ALGO_REQUEST.algo = algo
    try:
        yield
    finally:
        _ALGO_REQUEST.algo = old


# ---------------------------------------------------------------------------------------------------
def _alloc_conv_images(w, transpose, bf16=False):
    """The direct image and, as attributes, whichever other images the weight's shape admits -- allocated, not filled.
    bf16: also the bf16 image of a 3x3 weight (.bf16, idiff_pack_conv_weight_bf16) for the conv_operands("bf16") mode."""
    lib = _lib.load()
    _c(w, "weight")
    co, ci, k, _ = w.shape
    out = torch.empty((k * k, co, ci) if transpose else (k * k, ci, co), device=w.device, dtype=torch.float32)
    if bf16 and k == 3:
        out.bf16 = torch.empty((lib.idiff_conv_weight_bf16_bytes(co, ci, 1 if transpose else 0) // 2,), device=w.device, dtype=torch.int16)
    if k == 3 and WINOGRAD and co % 8 == 0 and ci % 8 == 0 and (ci if transpose else co) % 16 == 0:
        # Winograd-domain copy rides along as an attribute; conv2d hands it to the C ABI (idiff_conv_desc.wwino)
        cconv, kconv = (ci, co) if transpose else (co, ci)  # the conv's (Cout, Cin); Cout is padded to whole 64-blocks
        out.wino = torch.empty((16 * kconv * ((cconv + 63) // 64) * 64,), device=w.device, dtype=torch.float32)
        if WINOGRAD4 and (WINOGRAD4_DGRAD or not transpose):
            out.wino4 = torch.empty((36 * kconv * ((cconv + 63) // 64) * 64,), device=w.device, dtype=torch.float32)
    cconv1, kconv1 = (ci, co) if transpose else (co, ci)  # the conv's (Cout, Cin)
    if k == 1 and X3 and cconv1 % 64 == 0 and kconv1 >= 32 and kconv1 % 8 == 0:
        # three-plane bf16 image of a 1x1 weight (idiff_conv_desc.wx3): flattened 1x1 layers then run on the bf16 matrix cores; the
        # data-gradient pack is the image of the transposed matrix
        out.x3 = torch.empty((lib.idiff_conv1x1_x3_image_bytes(cconv1, kconv1) // 2,), device=w.device, dtype=torch.int16)
    return out


def _fill_conv_images(out, w, transpose, algo=None):
    """algo None: every image `out` carries; CONV_ALGO_x: the one image that kernel reads."""
    lib = _lib.load()
    co, ci, k, _ = w.shape
    tr = 1 if transpose else 0
    if algo is None or algo == CONV_ALGO_DIRECT:
        fn = lib.idiff_pack_conv_weight_T if transpose else lib.idiff_pack_conv_weight
        check(fn(_p(w), _p(out), co, ci, k, _stream()), "pack_conv_weight")
    if hasattr(out, "wino") and (algo is None or algo == CONV_ALGO_WINOGRAD):
        check(lib.idiff_pack_conv_weight_wino(_p(w), _p(out.wino), co, ci, tr, _stream()), "pack_conv_weight_wino")
    if hasattr(out, "wino4") and (algo is None or algo in (CONV_ALGO_WINOGRAD4, CONV_ALGO_WINOGRAD4H)):
        check(lib.idiff_pack_conv_weight_wino4(_p(w), _p(out.wino4), co, ci, tr, _stream()), "pack_conv_weight_wino4")
    if hasattr(out, "x3") and (algo is None or algo == CONV_ALGO_X3):
        cconv1, kconv1 = (ci, co) if transpose else (co, ci)
        wm = w.reshape(co, ci).t().contiguous() if transpose else w
        check(lib.idiff_pack_conv1x1_x3(_p(wm), out.x3.data_ptr(), cconv1, kconv1, _stream()), "pack_conv1x1_x3")
    if hasattr(out, "bf16") and (algo is None or algo == CONV_ALGO_BF16):
        check(lib.idiff_pack_conv_weight_bf16(_p(w), out.bf16.data_ptr(), co, ci, tr, _stream()), "pack_conv_weight_bf16")


def pack_conv_weight(w, transpose=False, bf16=False):
    """[Cout,Cin,k,k] -> packed [k*k][Cin][Cout] (or the flipped/transposed pack for the data gradient), with the Winograd-domain /
    split-bf16 images the shape admits as attributes (.wino, .wino4, .x3); bf16=True adds the bf16-operand image of a 3x3 weight (.bf16)."""
    out = _alloc_conv_images(w, transpose, bf16)
    _fill_conv_images(out, w, transpose)
    return out


class LazyConvWeight:
    """A conv weight for ONE conv2d call whose images are packed at that call: conv2d asks the library which kernel it will launch
    (idiff_conv2d_plan) and fills only the image that kernel reads.  For weights that change every step (training: one pack launch
    per use instead of three); the sampling path packs once per weight version and keeps every image (pack_conv_weight)."""

    def __init__(self, w, transpose=False):
        self.w, self.transpose = _c(w, "weight"), transpose


def conv2d(src0, wpk, bias, ks, Cout, src1=None, mode=CONV_NORMAL, pro=None, out=None, res=None, vec=None, aux=None,
           want_stats=False, algo=None, gn=None, operands=None):
    """Implicit-GEMM conv.  pro=(a,b): per-(b,c) affine+SiLU applied to src0 while it is gathered;
    aux=(tensor,a,b): adds silu(a*tensor+b) in the epilogue.  Returns out or (out, stats).
    algo: None = the library picks; CONV_ALGO_x = that kernel or an error (idiff_conv_desc.algo_request).
    gn = dict(groups, gamma, beta, film=None, eps=1e-5, want_mean_rstd=False): the GroupNorm(+FiLM) finalize of this conv's
    statistics rides on the call (a finalize launch enqueued by the library behind the conv): returns (out, (a, b)) or
    (out, (a, b, mean_rstd)).
    operands: "f32" | "bf16" | None (= the calling thread's conv_operands() scope).  "bf16" on a 3x3 conv sets
    idiff_conv_desc.operands = 1 and hands the weight's .bf16 image over (a LazyConvWeight gets one packed)."""
    lib = _lib.load()
    B, C0, Hin, Win = src0.shape
    operands = current_conv_operands() if operands is None else operands
    if operands not in CONV_OPERANDS:
        raise ValueError(f"conv operands must be one of {CONV_OPERANDS}, got {operands!r}")
    bf16 = operands == "bf16" and ks == 3
    lazy = wpk if isinstance(wpk, LazyConvWeight) else None
    if lazy is not None:
        wpk = _alloc_conv_images(lazy.w, lazy.transpose, bf16 or algo == CONV_ALGO_BF16)
    d = ConvDesc()
    if bf16:
        d.operands = 1
    wb = getattr(wpk, "bf16", None)
    if wb is not None and ks == 3:  # read only with operands = 1 or a request by name
        d.wbf16 = wb.data_ptr()
    if algo is not None:
        d.algo_request = 1 + algo
    elif ks == 3 and getattr(_ALGO_REQUEST, "algo", None) is not None:
        d.algo_request = -(1 + _ALGO_REQUEST.algo)  # scope request: taken where the shape tiles, the library's choice elsewhere
    d.src0, d.src0_bstride, d.C0 = src0.data_ptr(), _bs(src0, "src0"), C0
    if src1 is not None:
        assert src1.shape[0] == B and src1.shape[2:] == src0.shape[2:]
        d.src1, d.src1_bstride, d.C1 = src1.data_ptr(), _bs(src1, "src1"), src1.shape[1]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = B, Hin, Win, mode, ks, Cout
    _c(wpk, "wpk")
    d.wpk = wpk.data_ptr()
    wino = getattr(wpk, "wino", None)
    if wino is not None and ks == 3:
        d.wwino = wino.data_ptr()
        wino4 = getattr(wpk, "wino4", None)
        if wino4 is not None:
            d.wwino4 = wino4.data_ptr()
    x3 = getattr(wpk, "x3", None)
    if x3 is not None and ks == 1 and mode in (CONV_NORMAL, CONV_UNSHUFFLE2):
        d.wx3 = x3.data_ptr()
    if bias is not None:
        d.bias = _c(bias, "bias").data_ptr()
    if pro is not None:
        d.pro_a, d.pro_b = _c(pro[0], "pro_a").data_ptr(), _c(pro[1], "pro_b").data_ptr()
    if mode == CONV_UPSAMPLE2:
        Hout, Wout = Hin * 2, Win * 2
    elif mode == CONV_UNSHUFFLE2:
        Hout, Wout = Hin // 2, Win // 2
    else:
        Hout, Wout = Hin, Win
    if out is None:
        out = torch.empty((B, Cout, Hout, Wout), device=src0.device, dtype=torch.float32)
    else:
        assert tuple(out.shape) == (B, Cout, Hout, Wout), (out.shape, (B, Cout, Hout, Wout))
    d.out, d.out_bstride = out.data_ptr(), _bs(out, "out")
    if res is not None:
        assert res.shape == out.shape
        d.res, d.res_bstride = res.data_ptr(), _bs(res, "res")
    if vec is not None:
        assert tuple(vec.shape) == (B, Cout)
        d.vec = _c(vec, "vec").data_ptr()
    if aux is not None:
        t, a, b = aux
        assert t.shape == out.shape
        d.aux, d.aux_bstride = t.data_ptr(), _bs(t, "aux")
        d.aux_a, d.aux_b = _c(a, "aux_a").data_ptr(), _c(b, "aux_b").data_ptr()
    stats = None
    bufs = gn.get("bufs") if gn is not None else None  # caller-placed (stats, out_a, out_b[, mean_rstd]): the guard-band tests
    if want_stats or gn is not None:
        nt = lib.idiff_conv2d_num_tiles(Hout, Wout)
        stats = bufs[0] if bufs is not None else torch.empty((B, nt, Cout, 2), device=src0.device, dtype=torch.float32)
        assert tuple(stats.shape) == (B, nt, Cout, 2) and stats.is_contiguous() and stats.dtype == torch.float32
        d.stats = stats.data_ptr()
    gn_out = None
    if gn is not None:
        if bufs is not None:
            ga, gb = bufs[1], bufs[2]
            assert tuple(ga.shape) == (B, Cout) == tuple(gb.shape) and ga.is_contiguous() and gb.is_contiguous()
        else:
            ga, gb = torch.empty((B, Cout), device=src0.device, dtype=torch.float32), torch.empty((B, Cout), device=src0.device, dtype=torch.float32)
        d.gn_groups, d.gn_eps = int(gn["groups"]), float(gn.get("eps", 1e-5))
        d.gn_gamma, d.gn_beta = _c(gn["gamma"], "gn gamma").data_ptr(), _c(gn["beta"], "gn beta").data_ptr()
        film = gn.get("film")
        if film is not None:
            _chk(film, "film")
            assert film.shape[0] == B and film.shape[1] == 2 * Cout and film.stride(1) == 1
            d.gn_film, d.gn_film_ld = film.data_ptr(), film.stride(0)
        d.gn_out_a, d.gn_out_b = ga.data_ptr(), gb.data_ptr()
        gn_out = (ga, gb)
        if gn.get("want_mean_rstd"):
            mr = bufs[3] if bufs is not None else torch.empty((B, d.gn_groups, 2), device=src0.device, dtype=torch.float32)
            assert tuple(mr.shape) == (B, d.gn_groups, 2) and mr.is_contiguous()
            d.gn_mean_rstd = mr.data_ptr()
            gn_out = (ga, gb, mr)
    planned = None
    if lazy is not None:
        planned = lib.idiff_conv2d_plan(C.byref(d))
        check(min(planned, 0), "conv2d_plan")
        _fill_conv_images(wpk, lazy.w, lazy.transpose, planned)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.idiff_conv2d_fwd(C.byref(d), _stream()), "conv2d_fwd")
        e1.record()
        Cin = (C0 * 4 if mode == CONV_UNSHUFFLE2 else C0) + (src1.shape[1] if src1 is not None else 0)
        PROFILE.append(dict(ks=ks, mode=mode, Cin=Cin, Cout=Cout, B=B, Hout=Hout, Wout=Wout, e0=e0, e1=e1, algo=lib.idiff_conv2d_last_algo(),
                            flops=2.0 * Cin * Cout * ks * ks * Hout * Wout * B))
    else:
        check(lib.idiff_conv2d_fwd(C.byref(d), _stream()), "conv2d_fwd")
    if planned is not None and lib.idiff_conv2d_last_algo() != planned:  # the one image that was filled is not the one that was read
        raise RuntimeError("conv2d: planned kernel %d, launched %d" % (planned, lib.idiff_conv2d_last_algo()))
    if ALGO_TRACE is not None:
        Cin = (C0 * 4 if mode == CONV_UNSHUFFLE2 else C0) + (src1.shape[1] if src1 is not None else 0)
        ALGO_TRACE[(lib.idiff_conv2d_last_algo(), ks, Cin, Cout, Hout, Wout)] += 1
    if gn is not None:
        return (out, gn_out, stats) if want_stats else (out, gn_out)
    return (out, stats) if want_stats else out


def gn_finalize(stats, groups, HW, gamma, beta, film=None, eps=1e-5, want_mean_rstd=False):
    lib = _lib.load()
    B, nt, Cc, _ = stats.shape
    a = torch.empty((B, Cc), device=stats.device, dtype=torch.float32)
    b = torch.empty_like(a)
    mr = torch.empty((B, groups, 2), device=stats.device, dtype=torch.float32) if want_mean_rstd else None
    film_ld = 0
    if film is not None:
        _chk(film, "film")
        assert film.shape[0] == B and film.shape[1] == 2 * Cc and film.stride(1) == 1
        film_ld = film.stride(0)
    check(lib.idiff_gn_finalize(_p(_c(stats)), nt, B, Cc, groups, HW, _p(_c(gamma)), _p(_c(beta)), _p(film), film_ld, eps,
                                _p(a), _p(b), _p(mr), _stream()), "gn_finalize")
    return (a, b, mr) if want_mean_rstd else (a, b)


def affine_silu_add(h, ab=None, res=None, vec=None, out=None):
    lib = _lib.load()
    B, Cc = h.shape[:2]
    HW = h.shape[2] * h.shape[3]
    if out is None:
        out = torch.empty(h.shape, device=h.device, dtype=torch.float32)
    a, b = ab if ab is not None else (None, None)
    check(lib.idiff_affine_silu_add(_p(h), _bs(h, "h"), _p(_c(a)), _p(_c(b)), _p(res), _bs(res, "res") if res is not None else 0,
                                    _p(_c(vec)), _p(out), _bs(out, "out"), B, Cc, HW, _stream()), "affine_silu_add")
    return out


def linear(x, w, bias=None, res=None, gscale=None, act_in=ACT_NONE, act_out=ACT_NONE, out=None):
    """x [R,K] (row-strided ok), w [N,K] (row-strided ok) -> [R,N]."""
    lib = _lib.load()
    _chk(x, "x"), _chk(w, "w")
    assert x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.stride(1) == 1 and x.shape[1] == w.shape[1]
    R, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((R, N), device=x.device, dtype=torch.float32)
    assert out.stride(1) == 1 and tuple(out.shape) == (R, N)
    if res is not None:
        assert res.stride(1) == 1 and tuple(res.shape) == (R, N)
    check(lib.idiff_linear_fwd(_p(x), x.stride(0), _p(w), w.stride(0), _p(_c(bias)), _p(res), res.stride(0) if res is not None else 0,
                               _p(_c(gscale)), _p(out), out.stride(0), R, K, N, act_in, act_out, _stream()), "linear_fwd")
    return out


def linear_t(x, wT, bias=None, res=None, gscale=None, act_in=ACT_NONE, act_out=ACT_NONE, out=None, ln=None):
    """x [R,K] (row-strided ok), wT [K,N] PRE-TRANSPOSED weight (row-strided ok) -> [R,N].
    ln = (gamma, beta, eps): LayerNorm(x) over K fused in front of the product (no act_in then)."""
    lib = _lib.load()
    _chk(x, "x"), _chk(wT, "wT")
    assert x.dim() == 2 and wT.dim() == 2 and x.stride(1) == 1 and wT.stride(1) == 1 and x.shape[1] == wT.shape[0]
    R, K = x.shape
    N = wT.shape[1]
    if out is None:
        out = torch.empty((R, N), device=x.device, dtype=torch.float32)
    assert out.stride(1) == 1 and tuple(out.shape) == (R, N)
    if res is not None:
        assert res.stride(1) == 1 and tuple(res.shape) == (R, N)
    if ln is not None:
        assert act_in == ACT_NONE
        check(lib.idiff_linear_t_ln_fwd(_p(x), x.stride(0), _p(_c(ln[0])), _p(_c(ln[1])), float(ln[2]), _p(wT), wT.stride(0), _p(_c(bias)), _p(res),
                                        res.stride(0) if res is not None else 0, _p(_c(gscale)), _p(out), out.stride(0), R, K, N, act_out,
                                        _stream()), "linear_t_ln_fwd")
        return out
    check(lib.idiff_linear_t_fwd(_p(x), x.stride(0), _p(wT), wT.stride(0), _p(_c(bias)), _p(res), res.stride(0) if res is not None else 0,
                                 _p(_c(gscale)), _p(out), out.stride(0), R, K, N, act_in, act_out, _stream()), "linear_t_fwd")
    return out


def linear_t_grouped(groups):
    """ONE launch for up to 16 independent linear_t problems (idiff_linear_t_grouped_fwd).  Each group is a dict with the keyword
    arguments of linear_t: x, wT, bias=None, res=None, gscale=None, act_in, act_out, out=None, ln=None.  Returns the outputs."""
    lib = _lib.load()
    n = len(groups)
    assert 1 <= n <= _lib.LINEAR_MAX_GROUPS, n
    arr = (_lib.LinearGroup * n)()
    outs = []
    for d, g in zip(arr, groups):
        x, wT = g["x"], g["wT"]
        _chk(x, "x"), _chk(wT, "wT")
        assert x.dim() == 2 and wT.dim() == 2 and x.stride(1) == 1 and wT.stride(1) == 1 and x.shape[1] == wT.shape[0]
        R, K = x.shape
        N = wT.shape[1]
        out = g.get("out")
        if out is None:
            out = torch.empty((R, N), device=x.device, dtype=torch.float32)
        assert out.stride(1) == 1 and tuple(out.shape) == (R, N)
        res, bias, gs, ln = g.get("res"), g.get("bias"), g.get("gscale"), g.get("ln")
        d.x, d.ldx, d.wT, d.ldw = x.data_ptr(), x.stride(0), wT.data_ptr(), wT.stride(0)
        d.bias = _c(bias, "bias").data_ptr() if bias is not None else None
        if res is not None:
            assert res.stride(1) == 1 and tuple(res.shape) == (R, N)
            d.res, d.ldr = res.data_ptr(), res.stride(0)
        d.gscale = _c(gs, "gscale").data_ptr() if gs is not None else None
        d.out, d.ldo = out.data_ptr(), out.stride(0)
        if ln is not None:
            assert g.get("act_in", ACT_NONE) == ACT_NONE
            d.ln_g, d.ln_b, d.ln_eps = _c(ln[0], "ln_g").data_ptr(), _c(ln[1], "ln_b").data_ptr(), float(ln[2])
        d.R, d.K, d.N, d.act_in, d.act_out = R, K, N, g.get("act_in", ACT_NONE), g.get("act_out", ACT_NONE)
        outs.append(out)
    check(lib.idiff_linear_t_grouped_fwd(arr, n, _stream()), "linear_t_grouped_fwd")
    return outs


def attn_tokens_packed_grouped(qkvs, heads, scale):
    """attn_tokens_packed for several packed projections of one shape [B,N,3C] in ONE launch -> list of [B,N,C]"""
    lib = _lib.load()
    n = len(qkvs)
    assert 1 <= n <= _lib.LINEAR_MAX_GROUPS
    B, Nq, C3 = qkvs[0].shape
    Cc = C3 // 3
    PA = C.c_void_p * n
    q, k, v, o = PA(), PA(), PA(), PA()
    outs = []
    for i, t in enumerate(qkvs):
        _c(t, "qkv")
        assert tuple(t.shape) == (B, Nq, C3)
        out = torch.empty((B, Nq, Cc), device=t.device, dtype=torch.float32)
        base = t.data_ptr()
        q[i], k[i], v[i], o[i] = base, base + 4 * Cc, base + 8 * Cc, out.data_ptr()
        outs.append(out)
    check(lib.idiff_attn_tokens_grouped_fwd(q, k, v, o, n, B, Nq, Nq, Cc, heads, scale, C3, C3, _stream()), "attn_tokens_grouped_fwd")
    return outs


def linear_t_heads(x, wT, bias, out, heads, K, N, x_hs, w_hs, b_hs, o_hs):
    """heads independent [R,K] x [K,N] products in one launch: head h reads x[:, h*x_hs : h*x_hs+K], the [K,N] block of wT
    starting w_hs elements further per head, bias[h*b_hs : h*b_hs+N], and writes out[:, h*o_hs : h*o_hs+N]."""
    lib = _lib.load()
    _chk(x, "x"), _chk(wT, "wT"), _chk(out, "out")
    assert x.dim() == 2 and wT.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and wT.stride(1) == 1 and out.stride(1) == 1
    R = x.shape[0]
    assert out.shape[0] == R and (heads - 1) * x_hs + K <= x.shape[1] and (heads - 1) * o_hs + N <= out.shape[1]
    assert (heads - 1) * w_hs + (K - 1) * wT.stride(0) + N <= wT.numel()
    check(lib.idiff_linear_t_heads_fwd(_p(x), x.stride(0), x_hs, _p(wT), wT.stride(0), w_hs, _p(_c(bias)), b_hs, _p(out), out.stride(0), o_hs,
                                       R, K, N, heads, _stream()), "linear_t_heads_fwd")
    return out


def smm_memproj(feat, ln1_g, ln1_b, wpk, bias, ln2_g, ln2_b, eps=1e-5):
    """feat [B,C,H,W] -> mem [B,256,H*W] = LN(Linear(LN(tokens)))"""
    lib = _lib.load()
    B, Cc, H, W = feat.shape
    out = torch.empty((B, 256, H * W), device=feat.device, dtype=torch.float32)
    check(lib.idiff_smm_memproj_fwd(_p(feat), _bs(feat, "feat"), _p(_c(ln1_g)), _p(_c(ln1_b)), _p(_c(wpk)), _p(_c(bias)), _p(_c(ln2_g)),
                                    _p(_c(ln2_b)), _p(out), B, Cc, H * W, eps, _stream()), "smm_memproj_fwd")
    return out


def smm_memproj_compact(feat, ln1_g, ln1_b, gram, hvec, evar, Cm, eps1=1e-5, eps2=1e-5):
    """feat [B,C,H,W] -> [B,Cm,H*W] rows [xhat*rstd2 ; rstd2 ; 0]: the (C+1)-dim affine pre-image of the 256-wide memory.
    gram [C,C], hvec [C], evar: the quadratic form of the 256-wide variance (memory_variance_form)."""
    lib = _lib.load()
    B, Cc, H, W = feat.shape
    out = torch.empty((B, Cm, H * W), device=feat.device, dtype=torch.float32)
    check(lib.idiff_smm_memproj_compact_fwd(_p(feat), _bs(feat, "feat"), _p(_c(ln1_g)), _p(_c(ln1_b)), _p(_c(gram)), _p(_c(hvec)), float(evar),
                                            _p(out), B, Cc, H * W, Cm, eps1, eps2, _stream()), "smm_memproj_compact_fwd")
    return out


def memory_variance_form(lin_weight, lin_bias):
    """(gram [C,C], hvec [C], evar) with var_256(W x + b) = x^T gram x + 2 hvec.x + evar  (host-side weight preparation, fp64)."""
    W = lin_weight.detach().double()
    b = lin_bias.detach().double()
    Wc = W - W.mean(dim=0, keepdim=True)
    bc = b - b.mean()
    n = W.shape[0]
    return (Wc.t() @ Wc / n).float().contiguous(), (Wc.t() @ bc / n).float().contiguous(), float(bc.dot(bc) / n)


def layernorm_rows(x, gamma, beta, eps=1e-5, want_mean_rstd=False):
    lib = _lib.load()
    _chk(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    R, Cc = x.shape
    out = torch.empty((R, Cc), device=x.device, dtype=torch.float32)
    mr = torch.empty((R, 2), device=x.device, dtype=torch.float32) if want_mean_rstd else None
    check(lib.idiff_layernorm_rows_fwd(_p(x), x.stride(0), _p(_c(gamma)), _p(_c(beta)), _p(out), Cc, R, Cc, eps, _p(mr), _stream()),
          "layernorm_rows")
    return (out, mr) if want_mean_rstd else out


def time_embed(t, dim, freqs=None):
    lib = _lib.load()
    _c(t, "t"), _c(freqs, "freqs")
    B = t.numel()
    out = torch.empty((B, dim), device=t.device, dtype=torch.float32)
    check(lib.idiff_time_embed_fwd(_p(t), _p(freqs), B, dim, _p(out), _stream()), "time_embed")
    return out


def chan_layernorm(x, gamma, beta, eps=1e-5, want_mean_rstd=False):
    lib = _lib.load()
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    mr = torch.empty((B, H * W, 2), device=x.device, dtype=torch.float32) if want_mean_rstd else None
    check(lib.idiff_chan_layernorm_fwd(_p(x), _bs(x, "x"), _p(_c(gamma)), _p(_c(beta)), _p(out), Cc * H * W, B, Cc, H * W, eps, _p(mr),
                                       _stream()), "chan_layernorm")
    return (out, mr) if want_mean_rstd else out


# IDIFF_ATTN_DTYPE=bf16 | f16: the self-attention contractions on the bf16 / fp16 matrix cores (reduced-precision VARIANTS, never the
# default; f16 = the reference's own form, operands clamped to +-255; bench.py --attn bf16|f16 reports them as their own lines with
# the PSNR delta against the fp32 path)
ATTN_DTYPE = os.environ.get("IDIFF_ATTN_DTYPE", "f32").lower()


def attn_self(qkv, heads, scale, want_lse=False):
    """qkv [B,3C,H,W] -> [B,C,H,W]"""
    lib = _lib.load()
    _c(qkv, "qkv")
    B, C3, H, W = qkv.shape
    Cc, N = C3 // 3, H * W
    out = torch.empty((B, Cc, H, W), device=qkv.device, dtype=torch.float32)
    if ATTN_DTYPE in ("bf16", "f16") and not want_lse and Cc // heads == 64 and N % 4 == 0:
        fn = lib.idiff_attn_self_bf16_fwd if ATTN_DTYPE == "bf16" else lib.idiff_attn_self_f16_fwd
        check(fn(_p(qkv), _p(out), B, Cc, N, heads, scale, _stream()), "attn_self_%s_fwd" % ATTN_DTYPE)
        return out
    lse = torch.empty((B, heads, N), device=qkv.device, dtype=torch.float32) if want_lse else None
    check(lib.idiff_attn_self_fwd(_p(qkv), _p(out), _p(lse), B, Cc, N, heads, scale, _stream()), "attn_self_fwd")
    return (out, lse) if want_lse else out


def attn_ctx(q, k, v, heads, scale):
    """q [B,C,H,W]; k,v [B,M,C] -> [B,C,H,W]"""
    lib = _lib.load()
    _c(q, "q"), _c(k, "k"), _c(v, "v")
    B, Cc, H, W = q.shape
    M = k.shape[1]
    out = torch.empty_like(q)
    check(lib.idiff_attn_ctx_fwd(_p(q), _p(k), _p(v), _p(out), B, Cc, H * W, M, heads, scale, _stream()), "attn_ctx_fwd")
    return out


def attn_tokens(q, k, v, heads, scale):
    """q [B,Nq,C]; k,v [B,M,C] -> [B,Nq,C]"""
    lib = _lib.load()
    _c(q, "q"), _c(k, "k"), _c(v, "v")
    B, Nq, Cc = q.shape
    M = k.shape[1]
    out = torch.empty_like(q)
    check(lib.idiff_attn_tokens_fwd(_p(q), _p(k), _p(v), _p(out), B, Nq, M, Cc, heads, scale, Cc, Cc, _stream()), "attn_tokens_fwd")
    return out


def attn_tokens_packed(qkv, heads, scale):
    """self-attention on a packed projection qkv [B,N,3C] (q | k | v along the last dim) -> [B,N,C]; no copies."""
    lib = _lib.load()
    _c(qkv, "qkv")
    B, Nq, C3 = qkv.shape
    Cc = C3 // 3
    out = torch.empty((B, Nq, Cc), device=qkv.device, dtype=torch.float32)
    base = qkv.data_ptr()
    check(lib.idiff_attn_tokens_fwd(C.c_void_p(base), C.c_void_p(base + 4 * Cc), C.c_void_p(base + 8 * Cc), _p(out), B, Nq, Nq, Cc, heads, scale,
                                    C3, C3, _stream()), "attn_tokens_fwd")
    return out


def attn_tokens_packed_f16(qkv, heads, scale):
    """attn_tokens_packed in the reference's half-precision form (Attention_flash: +-255 clamp, fp16 operands and result, fp32
    statistics; idiff_attn_tokens_f16_fwd) -- the `if_flash` variant of the ScoreMapModule decoder"""
    lib = _lib.load()
    _c(qkv, "qkv")
    B, Nq, C3 = qkv.shape
    Cc = C3 // 3
    out = torch.empty((B, Nq, Cc), device=qkv.device, dtype=torch.float32)
    base = qkv.data_ptr()
    check(lib.idiff_attn_tokens_f16_fwd(C.c_void_p(base), C.c_void_p(base + 4 * Cc), C.c_void_p(base + 8 * Cc), _p(out), B, Nq, Nq, Cc, heads, scale,
                                        C3, C3, _stream()), "attn_tokens_f16_fwd")
    return out


def smm_xattn_kv_f16(q, k, v, heads, scale):
    """cross-attention of q [B,Nq,C] over UNFOLDED keys / values k, v [B,C,N] (channel-major) in the reference's half-precision form
    (Attention_flash) -> [B,Nq,C]; C = heads * 64, heads = 4, Nq <= 8"""
    lib = _lib.load()
    _c(q, "q"), _c(k, "k"), _c(v, "v")
    B, Nq, Cc = q.shape
    N = k.shape[2]
    assert tuple(k.shape) == (B, Cc, N) and tuple(v.shape) == (B, Cc, N)
    ws = torch.empty((lib.idiff_smm_xattn_kv_f16_ws_floats(B, N),), device=q.device, dtype=torch.float32)
    out = torch.empty_like(q)
    check(lib.idiff_smm_xattn_kv_f16_fwd(_p(q), _p(k), _p(v), _p(out), _p(ws), B, Nq, heads, Cc, N, scale, _stream()), "smm_xattn_kv_f16_fwd")
    return out


def smm_xattn(qf, mem, scale):
    """qf [B,Nq,heads,Cm]; mem [B,Cm,N] -> o [B,Nq,heads,Cm] (attention-weighted mem rows)."""
    lib = _lib.load()
    _c(qf, "qf"), _c(mem, "mem")
    B, Nq, heads, Cm = qf.shape
    N = mem.shape[2]
    nws = lib.idiff_smm_xattn_ws_floats(B, Nq, heads, Cm, N)
    ws = torch.empty((nws,), device=qf.device, dtype=torch.float32)
    o = torch.empty_like(qf)
    check(lib.idiff_smm_xattn_fwd(_p(qf), _p(mem), _p(o), _p(ws), B, Nq, heads, Cm, N, scale, _stream()), "smm_xattn_fwd")
    return o


def smm_xattn_grouped(qfs, mems, scale):
    """smm_xattn for several (qf [B,Nq,heads,Cm_i], mem [B,Cm_i,N_i]) pairs of one (B, Nq, heads) in ONE attention launch + ONE merge
    launch (idiff_smm_xattn_grouped_fwd) -> list of o; the same bits as the single calls."""
    lib = _lib.load()
    n = len(qfs)
    assert 1 <= n <= _lib.XATTN_MAX_GROUPS and len(mems) == n
    B, Nq, heads, _ = qfs[0].shape
    arr = (_lib.XattnGroup * n)()
    outs, keep = [], []
    for d, qf, mem in zip(arr, qfs, mems):
        _c(qf, "qf"), _c(mem, "mem")
        Cm, N = qf.shape[3], mem.shape[2]
        assert tuple(qf.shape[:3]) == (B, Nq, heads) and tuple(mem.shape[:2]) == (B, Cm)
        ws = torch.empty((lib.idiff_smm_xattn_ws_floats(B, Nq, heads, Cm, N),), device=qf.device, dtype=torch.float32)
        o = torch.empty_like(qf)
        d.qf, d.mem, d.o, d.ws, d.Cm, d.N = qf.data_ptr(), mem.data_ptr(), o.data_ptr(), ws.data_ptr(), Cm, N
        outs.append(o)
        keep.append(ws)
    check(lib.idiff_smm_xattn_grouped_fwd(arr, n, B, Nq, heads, scale, _stream()), "smm_xattn_grouped_fwd")
    return outs


def smm_memproj_compact_grouped(items, eps1=1e-5, eps2=1e-5):
    """smm_memproj_compact for several levels in ONE launch; items: dicts feat, ln1_g, ln1_b, gram, hvec, evar, Cm -> list of [B,Cm,H*W]"""
    lib = _lib.load()
    n = len(items)
    assert 1 <= n <= _lib.MEMPROJ_MAX_GROUPS
    B = items[0]["feat"].shape[0]
    arr = (_lib.MemprojGroup * n)()
    outs = []
    for d, it in zip(arr, items):
        feat = it["feat"]
        Bf, Cc, H, W = feat.shape
        assert Bf == B
        out = torch.empty((B, it["Cm"], H * W), device=feat.device, dtype=torch.float32)
        d.feat, d.feat_bstride = feat.data_ptr(), _bs(feat, "feat")
        d.ln1_g, d.ln1_b = _c(it["ln1_g"]).data_ptr(), _c(it["ln1_b"]).data_ptr()
        d.gram, d.hvec, d.evar = _c(it["gram"]).data_ptr(), _c(it["hvec"]).data_ptr(), float(it["evar"])
        d.out, d.C, d.N, d.Cm = out.data_ptr(), Cc, H * W, it["Cm"]
        outs.append(out)
    check(lib.idiff_smm_memproj_compact_grouped_fwd(arr, n, B, eps1, eps2, _stream()), "smm_memproj_compact_grouped_fwd")
    return outs


def scoremap_grouped(feats, tvs, idx):
    """scoremap for several levels in ONE launch -> list of (score [B,K,H,W], sel [B,1,H,W] or None)"""
    lib = _lib.load()
    n = len(feats)
    assert 1 <= n <= _lib.SCOREMAP_MAX_GROUPS and len(tvs) == n
    B = feats[0].shape[0]
    K = tvs[0].shape[1]
    if idx is not None:
        _c(idx, "idx", torch.int32)
    arr = (_lib.ScoremapGroup * n)()
    outs = []
    for d, feat, tv in zip(arr, feats, tvs):
        Bf, Cc, H, W = feat.shape
        _c(tv, "tv")
        assert Bf == B and tuple(tv.shape) == (B, K, Cc)
        out = torch.empty((B, K, H, W), device=feat.device, dtype=torch.float32)
        sel = torch.empty((B, 1, H, W), device=feat.device, dtype=torch.float32) if idx is not None else None
        d.feat, d.feat_bstride, d.tv, d.out, d.sel, d.C, d.HW = feat.data_ptr(), _bs(feat, "feat"), tv.data_ptr(), out.data_ptr(), \
            (sel.data_ptr() if sel is not None else None), Cc, H * W
        outs.append((out, sel))
    check(lib.idiff_scoremap_grouped_fwd(arr, n, _p(idx), B, K, _stream()), "scoremap_grouped_fwd")
    return outs


def time_mlp(t, freqs, w0, b0, w2, b2):
    """temb [B, nout] = w2 . GELU(w0 . sinusoidal(t) + b0) + b2 in one launch (idiff_time_mlp_fwd)"""
    lib = _lib.load()
    _c(t, "t"), _c(freqs, "freqs"), _c(w0, "w0"), _c(b0, "b0"), _c(w2, "w2"), _c(b2, "b2")
    B = t.numel()
    hid, dim = w0.shape
    nout = w2.shape[0]
    assert w2.shape[1] == hid
    out = torch.empty((B, nout), device=t.device, dtype=torch.float32)
    check(lib.idiff_time_mlp_fwd(_p(t), _p(freqs), _p(w0), _p(b0), _p(w2), _p(b2), _p(out), B, dim, hid, nout, _stream()), "time_mlp")
    return out


def conv3x3_select(x, weight, bias, idx):
    """final 3x3 conv + class gather in one pass: x [B,C,H,W], weight [K,C,3,3] (torch layout), idx int32 [B] -> [B,1,H,W]."""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    K = weight.shape[0]
    assert tuple(weight.shape) == (K, Cc, 3, 3) and idx.dtype == torch.int32 and idx.numel() == B
    out = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    check(lib.idiff_conv3x3_select_fwd(_p(x), _bs(x, "x"), _p(_c(weight)), _p(_c(bias)), C.c_void_p(idx.contiguous().data_ptr()), _p(out), B, Cc, K, H, W,
                                       _stream()), "conv3x3_select_fwd")
    return out


def scoremap(feat, tv, idx=None):
    """feat [B,C,H,W], tv [B,K,C] -> score [B,K,H,W] (+ sel [B,1,H,W] = score[b, idx[b]])."""
    lib = _lib.load()
    B, Cc, H, W = feat.shape
    K = tv.shape[1]
    _c(tv, "tv")
    out = torch.empty((B, K, H, W), device=feat.device, dtype=torch.float32)
    sel = None
    if idx is not None:
        _c(idx, "idx", torch.int32)
        sel = torch.empty((B, 1, H, W), device=feat.device, dtype=torch.float32)
    check(lib.idiff_scoremap_fwd(_p(feat), _bs(feat, "feat"), _p(tv), _p(out), _p(idx), _p(sel), B, Cc, H * W, K, _stream()), "scoremap")
    return out, sel


def image_metrics(pred, target):
    """pred/target [B,H,W] in [-1,1] -> [B,3] = (RMSE, PSNR dB, SSIM) on x/2+0.5, data_range 1 (device tensor).

    SSIM is NaN for H < 11 or W < 11 (no pixel has a whole 11x11 window; skimage refuses such an image), not 0.  The window moments are
    accumulated in fp32 on values shifted by the window-centre pixels (variances and the covariance are shift-invariant; the means get
    the shifts back), which keeps locally flat bright or saturated regions from cancelling against C2 = 9e-4; pixel values are summed by
    64 x 256 threads striding the image, a wave butterfly, four waves in order and 64 partials in fp64 (include/idiff.h)."""
    lib = _lib.load()
    pred, target = pred.contiguous(), target.contiguous()
    _c(pred, "pred"), _c(target, "target")
    B, H, W = pred.shape
    out = torch.empty((B, 3), device=pred.device, dtype=torch.float32)
    ws = torch.empty((B * 128,), device=pred.device, dtype=torch.float32)
    check(lib.idiff_image_metrics(_p(pred), _p(target), _p(out), _p(ws), B, H, W, _stream()), "image_metrics")
    return out


def gather_channel(x, idx):
    lib = _lib.load()
    _c(x, "x"), _c(idx, "idx", torch.int32)
    B, Cc, H, W = x.shape
    out = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    check(lib.idiff_gather_channel(_p(x), _p(idx), _p(out), B, Cc, H * W, _stream()), "gather_channel")
    return out


# ---------------------------------------------------------------------------------------------------
def irsde_reverse_step(x, mu, noise_pred, z, theta, sigma, sigma_bar, dt, sqrt_dt, mode=SDE_STEP, seed=0, offset=0, out=None):
    lib = _lib.load()
    _c(x, "x"), _c(mu, "mu"), _c(noise_pred, "noise_pred"), _c(z, "z")
    if out is None:
        out = torch.empty_like(x)
    check(lib.idiff_irsde_reverse_step(_p(x), _p(mu), _p(noise_pred), _p(z), _p(out), x.numel(), theta, sigma, sigma_bar, dt, sqrt_dt, mode,
                                       seed, offset, _stream()), "irsde_reverse_step")
    return out


# op codes of idiff_irsde_map (include/idiff.h)
(IRSDE_SCORE_FROM_NOISE, IRSDE_MU_BAR, IRSDE_DRIFT, IRSDE_REV_DRIFT, IRSDE_DISPERSION, IRSDE_STEP_MEAN, IRSDE_STEP_SDE, IRSDE_FORWARD_STEP,
 IRSDE_OPT_STEP, IRSDE_REAL_NOISE, IRSDE_REAL_SCORE, IRSDE_INIT_FROM_NOISE, IRSDE_RANDOM_STATES) = range(13)


def irsde_map(op, like, a=None, b=None, z=None, mu=None, k=None, coef_dev=None, seed=0, offset=0, out=None):
    """One piece of the reference's IRSDE arithmetic (include/idiff.h: IDIFF_IRSDE_*) over tensors shaped like `like` [B,...].
    mu: tensor of that shape or a python number; k: up to 6 python floats, or coef_dev: device [B,6] per-sample rows."""
    lib = _lib.load()
    _c(like, "like")
    for name, t in (("a", a), ("b", b), ("z", z)):
        _c(t, name)
        if t is not None and t.shape != like.shape:
            raise _lib.IdiffError(f"irsde_map: operand {name} has shape {tuple(t.shape)}, expected {tuple(like.shape)}")
    mu_t, mu_s = (mu, 0.0) if torch.is_tensor(mu) else (None, float(mu if mu is not None else 0.0))
    if mu_t is not None:
        if mu_t.shape != like.shape:
            mu_t = mu_t.expand(like.shape).contiguous()
        _c(mu_t, "mu")
    B = like.shape[0] if (coef_dev is not None and like.dim() > 0) else 1
    karr = None
    if coef_dev is not None:
        _c(coef_dev, "coef_dev")
        assert tuple(coef_dev.shape) == (B, 6), (coef_dev.shape, B)
    else:
        kk = [float(v) for v in (k or [])]
        karr = (C.c_float * 6)(*(kk + [0.0] * (6 - len(kk))))
    if out is None:
        out = torch.empty_like(like)
    check(lib.idiff_irsde_map(op, _p(a), _p(b), _p(z), _p(mu_t), mu_s, _p(out), B, like.numel() // B, _p(coef_dev), karr, seed, offset,
                              _stream()), "irsde_map")
    return out


def drift_reverse_step(x, r_hat, e_hat, z, a, b, c, cond=None, seed=0, offset=0, out=None, xa_out=None):
    lib = _lib.load()
    _c(x, "x"), _c(r_hat, "r_hat"), _c(e_hat, "e_hat"), _c(z, "z"), _c(cond, "cond")
    if out is None:
        out = torch.empty_like(x)
    if cond is not None and xa_out is None:
        xa_out = torch.empty_like(x)
    check(lib.idiff_drift_reverse_step(_p(x), _p(r_hat), _p(e_hat), _p(z), _p(cond), _p(out), _p(xa_out), x.numel(), a, b, c, seed, offset,
                                       _stream()), "drift_reverse_step")
    return (out, xa_out) if cond is not None else out


def _step_tables(coef, rows, state):
    """the device-state drift steps' shared assertion: `coef` [one of `rows`, T+1] and `state` int32 [3] on the GPU"""
    assert state.dtype == torch.int32 and state.is_cuda and state.numel() == 3 and coef.dim() == 2 and coef.shape[0] in rows


def drift_reverse_step_dev(x, r_hat, e_hat, z_base, cond, xa, coef, state, seed, nper, offset_base=0):
    """in-place, graph-replayable drift step: per-step scalars from `coef` [3, T+1] and `state` int32 [3] on the device"""
    lib = _lib.load()
    _c(x, "x"), _c(r_hat, "r_hat"), _c(e_hat, "e_hat"), _c(z_base, "z"), _c(cond, "cond"), _c(xa, "xa"), _c(coef, "coef")
    _step_tables(coef, (3,), state)
    check(lib.idiff_drift_reverse_step_dev(_p(x), _p(r_hat), _p(e_hat), _p(z_base), _p(cond), _p(xa), x.numel(), _p(coef), coef.shape[1],
                                           C.c_void_p(state.data_ptr()), seed, nper, offset_base, _stream()), "drift_reverse_step_dev")


def drift_reverse_step2_dev(x, r_hat, e_hat, r_prev, e_prev, z_base, cond, xa, coef5, state, seed, nper, offset_base=0):
    """second-order multistep form of drift_reverse_step_dev: `coef5` [5, T+1] adds the rows (rho_d, rho_s); r_prev / e_prev hold the
    previous jump's predictions and are overwritten with this jump's (not read where rho == 0)"""
    lib = _lib.load()
    _c(x, "x"), _c(r_hat, "r_hat"), _c(e_hat, "e_hat"), _c(r_prev, "r_prev"), _c(e_prev, "e_prev"), _c(z_base, "z"), _c(cond, "cond")
    _c(xa, "xa"), _c(coef5, "coef5")
    _step_tables(coef5, (5,), state)
    assert r_prev.numel() == x.numel() and e_prev.numel() == x.numel()
    check(lib.idiff_drift_reverse_step2_dev(_p(x), _p(r_hat), _p(e_hat), _p(r_prev), _p(e_prev), _p(z_base), _p(cond), _p(xa), x.numel(),
                                            _p(coef5), coef5.shape[1], C.c_void_p(state.data_ptr()), seed, nper, offset_base, _stream()),
          "drift_reverse_step2_dev")


# ---- posterior ensembles: member noise streams (include/idiff.h) ----
def member_ids(members, device):
    """ids (ints >= 1, any nesting flattened by the caller) -> int64 [R] on the device: the uint64 words the kernels read.  Id 0 is
    the stream of randn() and the plain steps and is refused, as are ids that do not fit 63 bits."""
    ids = [int(m) for m in members]
    if not ids or any(m < 1 or m >= 1 << 63 for m in ids):
        raise ValueError(f"member ids must be ints in [1, 2**63), got {ids}")
    return torch.tensor(ids, dtype=torch.int64, device=device)


def _members(members, rows):
    _c(members, "members", torch.int64)
    if members.dim() != 1 or members.numel() != rows:
        raise _lib.IdiffError(f"members must be int64 [{rows}], got {tuple(members.shape)}")
    return C.c_void_p(members.data_ptr())


def randn_members(members, sample_shape, seed, j=0):
    """[R, *sample_shape] normals: row r is draw j of member members[r] (int64 [R] on the device, from member_ids())"""
    lib = _lib.load()
    R = members.numel()
    out = torch.empty((R,) + tuple(sample_shape), device=members.device, dtype=torch.float32)
    check(lib.idiff_randn_members(_p(out), R, out.numel() // R, _members(members, R), seed, j, _stream()), "randn_members")
    return out


def ensemble_init(cond, S, members, sigma, seed):
    """cond [B, ...] -> (cond_rep, x, xa), each [B*S, ...]: row b*S + s holds cond[b], cond[b] + sigma*z(member, j = 0), x - cond[b]"""
    lib = _lib.load()
    _c(cond, "cond")
    B = cond.shape[0]
    cond_rep = torch.empty((B * S,) + tuple(cond.shape[1:]), device=cond.device, dtype=torch.float32)
    x, xa = torch.empty_like(cond_rep), torch.empty_like(cond_rep)
    check(lib.idiff_ensemble_init(_p(cond), _p(cond_rep), _p(x), _p(xa), B, S, cond.numel() // B, _members(members, B * S), sigma, seed,
                                  _stream()), "ensemble_init")
    return cond_rep, x, xa


def chain_begin(cond_in, cond, x, xa, state, tdev, sigma, seed, offset=0, t0=0, calls0=0, members=None, S=1, row0=0):
    """The start of an image in a held chain (idiff_chain_begin), one launch: cond <- cond_in's rows, x <- cond + sigma*z, xa <- x - cond,
    state <- {t0, calls0, 0}, tdev[:] <- t0.  Plain chain (members None): cond_in and the outputs are [B, ...], z is randn(seed, offset)
    over the flattened batch.  Member chain: cond_in is [B, ...], the outputs [R, ...] are rows row0 .. row0 + R of the B*S ensemble
    rows, row r from member members[r] (int64 [R] on the device) at draw 0."""
    lib = _lib.load()
    _c(cond_in, "cond_in"), _c(cond, "cond"), _c(x, "x"), _c(xa, "xa"), _c(state, "state", torch.int32), _c(tdev, "tdev")
    B, R = cond_in.shape[0], cond.shape[0]
    n_s = cond_in.numel() // B
    if state.numel() != 3 or tdev.numel() != R or x.shape != cond.shape or xa.shape != cond.shape or cond.numel() != R * n_s:
        raise _lib.IdiffError(f"chain_begin: cond / x / xa must be [R, sample] alike, state int32 [3], tdev [R]; got {tuple(cond.shape)}, "
                              f"{tuple(x.shape)}, {tuple(xa.shape)}, {tuple(state.shape)}, {tuple(tdev.shape)} for samples of {n_s}")
    check(lib.idiff_chain_begin(_p(cond_in), _p(cond), _p(x), _p(xa), B, S, n_s, row0, R, None if members is None else _members(members, R),
                                sigma, seed, offset, C.c_void_p(state.data_ptr()), _p(tdev), t0, calls0, _stream()), "chain_begin")


def drift_reverse_step_members_dev(x, r_hat, e_hat, r_prev, e_prev, z_base, cond, xa, coef, state, members, seed):
    """drift_reverse_step_dev (coef [3, T+1], r_prev = e_prev = None) or drift_reverse_step2_dev (coef [5, T+1]) on the rows of x
    [R, ...], with row r's z from member members[r]'s stream at draw 1 + state[1] (or from z_base [steps, R, ...])"""
    lib = _lib.load()
    _c(x, "x"), _c(r_hat, "r_hat"), _c(e_hat, "e_hat"), _c(r_prev, "r_prev"), _c(e_prev, "e_prev"), _c(z_base, "z"), _c(cond, "cond")
    _c(xa, "xa"), _c(coef, "coef"), _c(state, "state", torch.int32)
    R = x.shape[0]
    _step_tables(coef, (3, 5), state)
    for t in (r_hat, e_hat, r_prev, e_prev, cond, xa):
        assert t is None or t.numel() == x.numel()
    assert z_base is None or z_base.numel() % x.numel() == 0
    check(lib.idiff_drift_reverse_step_members_dev(_p(x), _p(r_hat), _p(e_hat), _p(r_prev), _p(e_prev), _p(z_base), _p(cond), _p(xa), R,
                                                   x.numel() // R, _p(coef), coef.shape[0], coef.shape[1], C.c_void_p(state.data_ptr()),
                                                   _members(members, R), seed, _stream()), "drift_reverse_step_members_dev")


def ensemble_stats(x):
    """x [B, S, ...] -> (mean, std), each [B, ...]: per-pixel mean and sample standard deviation over the S members, one pass"""
    lib = _lib.load()
    _c(x, "x")
    assert x.dim() >= 3, "ensemble_stats: x is [B, S, ...]"
    B, S = x.shape[:2]
    mean = torch.empty((B,) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    check(lib.idiff_ensemble_stats(_p(x), _p(mean), _p(std), B, S, x.numel() // (B * S), _stream()), "ensemble_stats")
    return mean, std


ORDER_AUTO, ORDER_NETWORK, ORDER_RANK = 0, 1, 2


def ensemble_order_stats(x, ks, algo=ORDER_AUTO, out=None):
    """x [B, S, ...] -> [B, nk, ...]: plane i holds, per pixel, the ks[i]-th smallest (0-based) of the pixel's S values; 1 <= nk <= 8 host
    ints in [0, S), any order, duplicates allowed.  algo: ORDER_AUTO | ORDER_NETWORK (S <= 16) | ORDER_RANK; the forms select the same
    values.  A NaN among a pixel's S values makes every plane NaN there."""
    lib = _lib.load()
    _c(x, "x")
    assert x.dim() >= 3, "ensemble_order_stats: x is [B, S, ...]"
    B, S = x.shape[:2]
    ks = list(ks)
    if any(not isinstance(k, int) or isinstance(k, bool) for k in ks):
        raise _lib.IdiffError(f"ensemble_order_stats: ks must be ints, got {ks}")
    if algo not in (ORDER_AUTO, ORDER_NETWORK, ORDER_RANK) or isinstance(algo, bool):
        raise _lib.IdiffError(f"ensemble_order_stats: algo must be 0 (auto), 1 (network) or 2 (rank), got {algo!r}")
    nk = len(ks)
    shape = (B, nk) + tuple(x.shape[2:])
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    _c(out, "out")
    assert tuple(out.shape) == shape, (tuple(out.shape), shape)
    ks_host = (C.c_int32 * max(nk, 1))(*ks)
    check(lib.idiff_ensemble_order_stats(_p(x), _p(out), B, S, x.numel() // (B * S), ks_host, nk, algo, _stream()), "ensemble_order_stats")
    return out


def interval_coverage(lo, hi, target):
    """lo, hi, target [B, ...] -> int32 [B, 3] = per image the pixels of target (below lo, inside [lo, hi], above hi), exact counts; a
    pixel where any of the three is NaN counts nowhere"""
    lib = _lib.load()
    _c(lo, "lo"), _c(hi, "hi"), _c(target, "target")
    assert lo.dim() >= 2 and lo.shape == hi.shape == target.shape, "interval_coverage: lo, hi, target are [B, ...] of one shape"
    B = lo.shape[0]
    n_s = lo.numel() // B
    counts = torch.empty((B, 3), device=lo.device, dtype=torch.int32)
    ws = torch.empty((max(int(lib.idiff_interval_coverage_ws_ints(B, n_s)), 1),), device=lo.device, dtype=torch.int32)
    check(lib.idiff_interval_coverage(_p(lo), _p(hi), _p(target), C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()), B, n_s,
                                      _stream()), "interval_coverage")
    return counts


def ensemble_scores(x, target, want_map=False):
    """x [B, S, ...] (the samples of an ensemble), target [B, ...] -> (sums float64 [B, 3], counts int32 [B, S + 2], crps_map [B, ...] or
    None), all on the device: per image the sums of the per-pixel CRPS, squared error of the ensemble mean and sample variance over the
    valid pixels; the rank histogram of the truth among the members (hist[0..S]) followed by the number of invalid (NaN) pixels; and,
    with want_map, the per-pixel CRPS (NaN where invalid).  Two launches, no host copy; include/idiff.h states the arithmetic.
    models/SDEs/driftSDE.py's ensemble_score_summary turns (pooled) sums and counts into CRPS / SSR / RANK_DEV / OUTLIERS."""
    lib = _lib.load()
    _c(x, "x"), _c(target, "target")
    assert x.dim() >= 3, "ensemble_scores: x is [B, S, ...]"
    B, S = x.shape[:2]
    assert tuple(target.shape) == (B,) + tuple(x.shape[2:]), "ensemble_scores: target is x without the member axis"
    n_s = x.numel() // (B * S) if B * S else 0
    sums = torch.empty((B, 3), device=x.device, dtype=torch.float64)
    counts = torch.empty((B, S + 2), device=x.device, dtype=torch.int32)
    crps_map = torch.empty_like(target) if want_map else None
    ws = torch.empty((max(int(lib.idiff_ensemble_scores_ws_bytes(B, S)), 8) // 8,), device=x.device, dtype=torch.float64)
    check(lib.idiff_ensemble_scores(_p(x), _p(target), _p(crps_map), C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()),
                                    C.c_void_p(ws.data_ptr()), B, S, n_s, _stream()), "ensemble_scores")
    return sums, counts, crps_map


def ensemble_distances(x, target=None):
    """x [B, S, ...] (the samples of an ensemble), target [B, ...] or None -> (d2 float64 [B, M, M], counts int32 [B, 2], pick int32
    [B, 2]), all on the device, M = S + (target is not None): per image the squared L2 distances between its M rows (the members in
    index order, then the target) over the pixels at which all M rows are finite; counts = (valid, invalid) pixels; pick = (medoid,
    best member), the best member -1 without a target.  Two launches, no host copy; include/idiff.h states the arithmetic and the
    scan order.  models/SDEs/driftSDE.py's ensemble_distance_summary turns d2 and counts into ES / ES_FAIR / DIVERSITY."""
    lib = _lib.load()
    _c(x, "x"), _c(target, "target")
    assert x.dim() >= 3, "ensemble_distances: x is [B, S, ...]"
    B, S = x.shape[:2]
    assert target is None or tuple(target.shape) == (B,) + tuple(x.shape[2:]), "ensemble_distances: target is x without the member axis"
    n_s = x.numel() // (B * S) if B * S else 0
    M = S + (target is not None)
    d2 = torch.empty((B, M, M), device=x.device, dtype=torch.float64)
    counts = torch.empty((B, 2), device=x.device, dtype=torch.int32)
    pick = torch.empty((B, 2), device=x.device, dtype=torch.int32)
    ws = torch.empty((max(int(lib.idiff_ensemble_distances_ws_bytes(B, S, int(target is not None))), 8) // 8,), device=x.device,
                     dtype=torch.float64)
    check(lib.idiff_ensemble_distances(_p(x), _p(target), C.c_void_p(d2.data_ptr()), C.c_void_p(counts.data_ptr()),
                                       C.c_void_p(pick.data_ptr()), C.c_void_p(ws.data_ptr()), B, S, n_s, _stream()), "ensemble_distances")
    return d2, counts, pick


def ensemble_pick_rows(x, pick, col):
    """x [B, S, ...], pick int32 [B, ncol] on the device (ops.ensemble_distances' pick), col a host int -> [B, ...]: row b is member
    pick[b, col] of image b, read on the device (one launch, no host copy), bit for bit.  An index outside [0, S) -- the best member of
    a call without a target -- gives a row of NaN."""
    lib = _lib.load()
    _c(x, "x"), _c(pick, "pick", torch.int32)
    assert x.dim() >= 3, "ensemble_pick_rows: x is [B, S, ...]"
    B, S = x.shape[:2]
    assert pick.dim() == 2 and pick.shape[0] == B, "ensemble_pick_rows: pick is [B, ncol]"
    if isinstance(col, bool) or not isinstance(col, int) or not 0 <= col < pick.shape[1]:
        raise _lib.IdiffError(f"ensemble_pick_rows: col must be an int in [0, {pick.shape[1]}), got {col!r}")
    n_s = x.numel() // (B * S) if B * S else 0
    out = torch.empty((B,) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    check(lib.idiff_ensemble_pick_rows(_p(x), C.c_void_p(pick.data_ptr() + 4 * col), pick.shape[1], _p(out), B, S, n_s, _stream()),
          "ensemble_pick_rows")
    return out


ENSEMBLE_MODES_REL_FLOOR = 2.0 ** -30
ENSEMBLE_PROJECT_MAX_K = 8


def ensemble_modes(d2, S, has_target, rel_floor=ENSEMBLE_MODES_REL_FLOOR):
    """d2 float64 [B, M, M] on the device (ops.ensemble_distances' matrix, M = S + has_target) -> (lam [B, S], vec [B, S, S], coef
    [B, S, S], tcoord [B, S], tnorm2 [B], all float64, info int32 [B, 2] = rank, sweeps), all on the device: the principal modes of the
    S members about their centroid.  lam are the eigenvalues of the centred Gram matrix in descending order, row k of vec the unit
    eigenvector of lam[k], row k of coef = vec[k] / sqrt(lam[k]) (zeros for a mode at or below rel_floor * lam[0]), so that
    ops.ensemble_project(x, coef[:, :K]) gives the K leading unit-norm mode images; with a target tcoord[k] is the coordinate of
    (target - ensemble mean) along mode k and tnorm2 its squared norm.  One launch, no host copy; include/idiff.h states the centring,
    the Jacobi schedule, the stop rule and the degenerate cases.  models/SDEs/driftSDE.py's ensemble_mode_summary reads EXPLAINED /
    EFF_MODES / SPAN_SHARE / MODE_Z off them."""
    lib = _lib.load()
    _c(d2, "d2", torch.float64)
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise _lib.IdiffError(f"ensemble_modes: S must be an int >= 1, got {S!r}")
    M = S + (1 if has_target else 0)
    assert d2.dim() == 3 and tuple(d2.shape[1:]) == (M, M), f"ensemble_modes: d2 is [B, {M}, {M}], got {tuple(d2.shape)}"
    B = d2.shape[0]
    dev = d2.device
    lam = torch.empty((B, S), device=dev, dtype=torch.float64)
    vec = torch.empty((B, S, S), device=dev, dtype=torch.float64)
    coef = torch.empty((B, S, S), device=dev, dtype=torch.float64)
    tcoord = torch.empty((B, S), device=dev, dtype=torch.float64)
    tnorm2 = torch.empty((B,), device=dev, dtype=torch.float64)
    info = torch.empty((B, 2), device=dev, dtype=torch.int32)
    check(lib.idiff_ensemble_modes(_p(d2), B, S, int(bool(has_target)), float(rel_floor), _p(lam), _p(vec), _p(coef), _p(tcoord), _p(tnorm2),
                                   _p(info), _stream()), "ensemble_modes")
    return lam, vec, coef, tcoord, tnorm2, info


def ensemble_project(x, coef):
    """x [B, S, ...] float32, coef [B, K, S] float64 on the device, any K >= 1 -> [B, K, ...] float32: plane k of image b is
    sum_s coef[b, k, s] (x[b, s] - the per-pixel member mean), in fp64 per pixel with the members in index order; any coefficients are
    taken (rows of ops.ensemble_modes' coef give unit-norm mode images).  A pixel where a member is NaN or infinite is NaN in every
    plane.  One launch per ENSEMBLE_PROJECT_MAX_K rows of coef, no host copy."""
    lib = _lib.load()
    _c(x, "x"), _chk(coef, "coef", torch.float64)
    assert x.dim() >= 3, "ensemble_project: x is [B, S, ...]"
    B, S = x.shape[:2]
    assert coef.dim() == 3 and coef.shape[0] == B and coef.shape[2] == S and coef.shape[1] >= 1, \
        f"ensemble_project: coef is [B, K, S] = [{B}, K >= 1, {S}], got {tuple(coef.shape)}"
    K = coef.shape[1]
    if not coef.is_contiguous():  # the leading rows of a larger table (coef[:, :K] of ops.ensemble_modes) are read in place
        if coef[0].is_contiguous() and coef.stride(0) >= K * S:
            image_stride = coef.stride(0)
        else:
            raise _lib.IdiffError("coef must be contiguous, or contiguous [K, S] tables at a fixed distance")
    else:
        image_stride = K * S
    n_s = x.numel() // (B * S) if B * S else 0
    step = ENSEMBLE_PROJECT_MAX_K
    direct = K <= step or B == 1  # the kernel writes [B][rows][n_s] densely: more than one chunk of a batch goes through pieces
    out = torch.empty((B, K) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32) if direct else None
    pieces = []
    for k0 in range(0, K, step):
        rows = min(step, K - k0)
        if direct:
            dst = out.data_ptr() + 4 * k0 * n_s
        else:
            pieces.append(torch.empty((B, rows) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32))
            dst = pieces[-1].data_ptr()
        check(lib.idiff_ensemble_project(_p(x), C.c_void_p(coef.data_ptr() + 8 * k0 * S), image_stride, C.c_void_p(dst), B, S, rows, n_s, _stream()),
              "ensemble_project")
    return out if direct else torch.cat(pieces, dim=1)


SPARSIFICATION_MAX_K = 64


def sparsification(key, pred, target, K=20):
    """key (a per-pixel uncertainty, or None for the oracle: the squared error itself), pred, target [B, ...] -> (sums float64
    [B, K + 1, 2], counts int32 [B, K + 1, 2], tau [B, K]), all on the device: per image and point k of the sparsification curve the
    sum of (pred - target)^2 and the number of pixels whose key is above / equal to the key of rank floor(k N / K) (row k), then the
    total and (N, invalid) (row K); tau is that key (NaN where the rank is 0).  Three launches, no sort, no host copy; include/idiff.h
    states the order, the arithmetic and the tie rule.  models/SDEs/driftSDE.py's sparsification_summary turns the (pooled) records of a
    map and of the oracle into the curves and AUSE / AURG."""
    lib = _lib.load()
    _c(key, "key"), _c(pred, "pred"), _c(target, "target")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= SPARSIFICATION_MAX_K:
        raise _lib.IdiffError(f"sparsification: K must be an int in [1, {SPARSIFICATION_MAX_K}], got {K!r}")
    assert pred.dim() >= 2 and pred.shape == target.shape, "sparsification: pred and target are [B, ...] of one shape"
    assert key is None or key.shape == pred.shape, "sparsification: key has the shape of pred"
    B = pred.shape[0]
    n_s = pred.numel() // B if B else 0
    sums = torch.empty((B, K + 1, 2), device=pred.device, dtype=torch.float64)
    counts = torch.empty((B, K + 1, 2), device=pred.device, dtype=torch.int32)
    tau = torch.empty((B, K), device=pred.device, dtype=torch.float32)
    ws = torch.empty((max(int(lib.idiff_sparsification_ws_bytes(B, K, n_s)), 8) // 8,), device=pred.device, dtype=torch.float64)
    check(lib.idiff_sparsification(_p(key), _p(pred), _p(target), K, C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()),
                                   C.c_void_p(tau.data_ptr()), C.c_void_p(ws.data_ptr()), B, n_s, _stream()), "sparsification")
    return sums, counts, tau


REGION_MAX_L = 64
REGION_MAX_S = 64
BAND_MAX_EDGES = 63


def region_scores(x, target, labels, L):
    """x [B, S, ...] (the samples of an ensemble) or [B, ...] (one restoration, S = 1), target [B, ...], labels uint8 [B, ...] (one map
    per image) or [...] (one map shared by every image), L regions -> (sums float64 [B, L, 4], counts int32 [B, L, S + 2], outside int32
    [B]), all on the device: ops.ensemble_scores' record per region -- the sums of the per-pixel CRPS, squared error of the ensemble mean,
    sample variance and signed mean error over the region's valid pixels; the region's rank histogram followed by its invalid pixels --
    and the pixels whose label is >= L (255 is the conventional "ignore"), which add nowhere else.  Two launches, no host copy;
    include/idiff.h states the arithmetic and the order.  models/SDEs/driftSDE.py's region_score_summary turns (pooled) records into
    per-region CRPS / RMSE / PSNR / BIAS / SSR / RANK_DEV / OUTLIERS and the error shares."""
    lib = _lib.load()
    _c(x, "x"), _c(target, "target"), _c(labels, "labels", torch.uint8)
    if isinstance(L, bool) or not isinstance(L, int) or not 1 <= L <= REGION_MAX_L:
        raise _lib.IdiffError(f"region_scores: L must be an int in [1, {REGION_MAX_L}], got {L!r}")
    assert target.dim() >= 2, "region_scores: target is [B, ...]"
    if x.dim() == target.dim():
        x = x.unsqueeze(1)
    B, S = x.shape[:2]
    assert tuple(target.shape) == (B,) + tuple(x.shape[2:]), "region_scores: target is x without the member axis"
    shared = tuple(labels.shape) == tuple(target.shape[1:])
    assert shared or tuple(labels.shape) == tuple(target.shape), "region_scores: labels has the shape of target, or of one image of it"
    n_s = x.numel() // (B * S) if B * S else 0
    sums = torch.empty((B, L, 4), device=x.device, dtype=torch.float64)
    counts = torch.empty((B, L, S + 2), device=x.device, dtype=torch.int32)
    outside = torch.empty((B,), device=x.device, dtype=torch.int32)
    ws = torch.empty((max(int(lib.idiff_region_scores_ws_bytes(B, S, L)), 8) // 8,), device=x.device, dtype=torch.float64)
    check(lib.idiff_region_scores(_p(x), _p(target), _p(labels), 0 if shared else n_s, L, C.c_void_p(sums.data_ptr()),
                                  C.c_void_p(counts.data_ptr()), C.c_void_p(outside.data_ptr()), C.c_void_p(ws.data_ptr()), B, S, n_s,
                                  _stream()), "region_scores")
    return sums, counts, outside


def band_labels(target, edges):
    """target (any shape, float32) -> uint8 labels of the same shape: labels = #{ j : edges[j] <= target }, i.e.
    np.searchsorted(edges, target, side="right"), and 255 where target is NaN.  edges: 1 .. 63 finite, strictly ascending host floats
    (rounded to float32), passed by value: "error by intensity band of the truth" for ops.region_scores with L = len(edges) + 1."""
    lib = _lib.load()
    _c(target, "target")
    edges = [float(e) for e in edges]
    ne = len(edges)
    labels = torch.empty(target.shape, device=target.device, dtype=torch.uint8)
    edges_host = (C.c_float * max(ne, 1))(*edges)
    check(lib.idiff_band_labels(_p(target), _p(labels), target.numel(), edges_host, ne, _stream()), "band_labels")
    return labels


@functools.lru_cache(maxsize=16)
def _grid_labels_host(H, W, gy, gx):
    return torch.tensor([[(r * gy // H) * gx + (c * gx // W) for c in range(W)] for r in range(H)], dtype=torch.uint8)


@functools.lru_cache(maxsize=16)
def _grid_labels_dev(H, W, gy, gx, device):
    return _grid_labels_host(H, W, gy, gx).to(device)


def grid_labels(H, W, gy, gx, device="cpu"):
    """uint8 [H, W] labels of a gy x gx grid of near-equal cells: label(r, c) = (r gy // H) gx + (c gx // W), gy gx <= 64 regions.
    Built on the host in integer arithmetic and cached per (H, W, gy, gx, device): treat the tensor as read-only."""
    for name, val in (("H", H), ("W", W), ("gy", gy), ("gx", gx)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"grid_labels: {name} must be an int >= 1, got {val!r}")
    if gy * gx > REGION_MAX_L or gy > H or gx > W:
        raise ValueError(f"grid_labels: a {gy} x {gx} grid needs gy gx <= {REGION_MAX_L}, gy <= H = {H} and gx <= W = {W}")
    return _grid_labels_dev(H, W, gy, gx, str(torch.device(device)))


DESPECKLE_NQ = 12  # sum a, a^2, y, y^2, a y | rho, rho^2 | La, Ly, La^2, Ly^2, La Ly
DESPECKLE_NC = 4   # valid, ratio, stencil, invalid


def despeckle_stats(x, ref, labels, L, scale=0.5, shift=0.5, ratio_floor=2.0 ** -8):
    """x [B, S, C, H, W] (the samples of an ensemble) or [B, C, H, W] (one restoration, S = 1), ref [B, C, H, W] (the noisy input, or the
    target), labels uint8 [B, C, H, W] or one shared [C, H, W], L regions -> (sums float64 [B, S, L, 12], counts int32 [B, S, L, 4],
    outside int32 [B]), all on the device: the sums behind the no-reference despeckling statistics per region and member.  With
    a = x scale + shift and y = ref scale + shift (the defaults put [-1, 1] tensors on the [0, 1] intensity scale, on which speckle is
    multiplicative): sum a, a^2, y, y^2, a y over the region's valid pixels (a and y finite); sum rho, rho^2 of the ratio image
    rho = y / a where a >= ratio_floor; sum La, Ly, La^2, Ly^2, La Ly of the 4-neighbour Laplacians where the whole stencil is valid
    and inside the plane.  counts = valid, ratio, stencil and invalid pixels; outside = pixels with a label >= L.  Two launches, no host
    copy; include/idiff.h states the arithmetic and the order.  models/SDEs/driftSDE.py's despeckle_summary turns the record into
    ENL / SSI / SMPI / MEAN_RATIO / VAR_RATIO / EPI / LAP_RATIO / CNR."""
    lib = _lib.load()
    _c(x, "x"), _c(ref, "ref"), _c(labels, "labels", torch.uint8)
    if isinstance(L, bool) or not isinstance(L, int) or not 1 <= L <= REGION_MAX_L:
        raise _lib.IdiffError(f"despeckle_stats: L must be an int in [1, {REGION_MAX_L}], got {L!r}")
    assert ref.dim() == 4, "despeckle_stats: ref is [B, C, H, W]"
    if x.dim() == 4:
        x = x.unsqueeze(1)
    assert x.dim() == 5, "despeckle_stats: x is [B, S, C, H, W] or [B, C, H, W]"
    B, S = x.shape[:2]
    assert tuple(ref.shape) == (B,) + tuple(x.shape[2:]), "despeckle_stats: ref is x without the member axis"
    shared = tuple(labels.shape) == tuple(ref.shape[1:])
    assert shared or tuple(labels.shape) == tuple(ref.shape), "despeckle_stats: labels has the shape of ref, or of one image of it"
    P, H, W = (int(n) for n in ref.shape[1:])
    sums = torch.empty((B, S, L, DESPECKLE_NQ), device=x.device, dtype=torch.float64)
    counts = torch.empty((B, S, L, DESPECKLE_NC), device=x.device, dtype=torch.int32)
    outside = torch.empty((B,), device=x.device, dtype=torch.int32)
    ws = torch.empty((max(int(lib.idiff_despeckle_stats_ws_bytes(B, S, L)), 8) // 8,), device=x.device, dtype=torch.float64)
    check(lib.idiff_despeckle_stats(_p(x), _p(ref), _p(labels), 0 if shared else P * H * W, L, float(scale), float(shift), float(ratio_floor),
                                    C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(outside.data_ptr()),
                                    C.c_void_p(ws.data_ptr()), B, S, P, H, W, _stream()), "despeckle_stats")
    return sums, counts, outside


@functools.lru_cache(maxsize=16)
def radial_bins(H, W):
    """The radial frequency bins of an H x W image's half plane, on the host in exact integer arithmetic -> (bins int32 [H, Wh], counts
    int64 [nb], freq float64 [nb]), Wh = W // 2 + 1.  With L = max(H, W), u' = min(u, H - u) and v' = v, the bin of (u, v) is the
    largest integer k with (2k - 1)^2 H^2 W^2 <= 4 L^2 (u'^2 W^2 + v'^2 H^2): the nearest integer to L sqrt((u'/H)^2 + (v'/W)^2), ties
    going up.  nb = the largest bin + 1; counts[k] = the bin's points of the full H x W plane (a half-plane point counts once for v = 0
    and for v = W/2 with W even, else twice), so counts.sum() == H W; freq[k] = k / L cycles per pixel.  Cached: treat the tensors as
    read-only."""
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < 1:
        raise ValueError(f"radial_bins: H and W must be ints >= 1, got {H!r}, {W!r}")
    Wh, L, D = W // 2 + 1, max(H, W), H * W
    rows = []
    for up in range(H // 2 + 1):
        rows.append([(math.isqrt(4 * L * L * (up * up * W * W + v * v * H * H)) // D + 1) // 2 for v in range(Wh)])
    table = [rows[min(u, H - u)] for u in range(H)]
    nb = max(max(row) for row in table) + 1
    counts = [0] * nb
    for row in table:
        for v, k in enumerate(row):
            counts[k] += 1 if v == 0 or 2 * v == W else 2
    return (torch.tensor(table, dtype=torch.int32), torch.tensor(counts, dtype=torch.int64),
            torch.tensor([k / L for k in range(nb)], dtype=torch.float64))


_radial_bins_dev = {}
SPECTRUM_MAX_WS_BYTES = 256 << 20


def radial_power_spectrum(x, sub=None, sub_rep=1, bins=None, nb=None, max_ws_bytes=SPECTRUM_MAX_WS_BYTES):
    """x [..., H, W] -> float64 [..., nb]: per plane the power |DFT|^2 / (H W) summed over the radial bins of radial_bins(H, W), the
    full frequency plane counted (so the bins of a plane add up to the sum of its squares).  With sub [..., H, W] of R / sub_rep planes
    the plane r is (double)x[r] - (double)sub[r // sub_rep]: residual spectra without a temporary.  fp64 on the matrix cores, no
    atomics, no host copy; a plane with a NaN or inf gives NaN in all its bins (idiff_radial_power_spectrum, include/idiff.h).  The
    bin table is uploaded once per (H, W, device); bins (int32 [H, Wh] on the device) and nb replace it: an entry outside [0, nb) drops
    its point.  The planes go in chunks whose workspace stays within max_ws_bytes; a plane's bits do not depend on the chunking."""
    lib = _lib.load()
    _c(x, "x"), _c(sub, "sub")
    assert x.dim() >= 2, "radial_power_spectrum: x is [..., H, W]"
    H, W = int(x.shape[-2]), int(x.shape[-1])
    R = 1
    for d in x.shape[:-2]:
        R *= int(d)
    if bins is None:
        key = (H, W, x.device)
        if key not in _radial_bins_dev:
            if not (1 <= H <= 1024 and 1 <= W <= 1024):
                raise _lib.IdiffError(f"radial_power_spectrum: H = {H}, W = {W} are outside [1, 1024]")
            table, counts, _ = radial_bins(H, W)
            _radial_bins_dev[key] = (table.to(x.device), int(counts.numel()))
        bins, nb = _radial_bins_dev[key]
    else:
        _c(bins, "bins", torch.int32)
        assert tuple(bins.shape) == (H, W // 2 + 1), "radial_power_spectrum: bins is [H, W // 2 + 1]"
        if isinstance(nb, bool) or not isinstance(nb, int):
            raise _lib.IdiffError(f"radial_power_spectrum: nb must be an int beside bins, got {nb!r}")
    if sub is not None:
        if isinstance(sub_rep, bool) or not isinstance(sub_rep, int) or sub_rep < 1 or R % sub_rep:
            raise _lib.IdiffError(f"radial_power_spectrum: sub_rep = {sub_rep!r} does not divide the {R} planes of x")
        if tuple(sub.shape[-2:]) != (H, W) or sub.numel() != (R // sub_rep) * H * W:
            raise _lib.IdiffError(f"radial_power_spectrum: sub holds {tuple(sub.shape)}, not {R // sub_rep} planes of {H} x {W}")
    out = torch.empty(tuple(x.shape[:-2]) + (max(nb, 0),), device=x.device, dtype=torch.float64)
    # rows per call: the workspace rule is the library's; groups of sub_rep rows stay together while one group fits
    rows = min(max(R, 1), 65535)
    while rows > 1 and int(lib.idiff_radial_power_spectrum_ws_bytes(rows, H, W)) > max_ws_bytes:
        rows = max(1, min(rows - 1, rows * max_ws_bytes // int(lib.idiff_radial_power_spectrum_ws_bytes(rows, H, W))))
    group = sub_rep if sub is not None else 1
    if rows >= group:
        rows -= rows % group
    ws = torch.empty((max(int(lib.idiff_radial_power_spectrum_ws_bytes(rows, H, W)), 8) // 8,), device=x.device, dtype=torch.float64)
    r0 = 0
    while True:
        n = min(rows, R - r0)
        rep = group
        if sub is not None and rows < group:  # a chunk inside one group of rows: they all take the same plane of sub
            n = min(n, group - r0 % group)
            rep = n
        check(lib.idiff_radial_power_spectrum(C.c_void_p(x.data_ptr() + 4 * r0 * H * W),
                                              None if sub is None else C.c_void_p(sub.data_ptr() + 4 * (r0 // group) * H * W), rep,
                                              C.c_void_p(bins.data_ptr()), nb, C.c_void_p(out.data_ptr() + 8 * r0 * max(nb, 0)),
                                              C.c_void_p(ws.data_ptr()), n, H, W, _stream()), "radial_power_spectrum")
        r0 += n
        if r0 >= R:
            return out


def dihedral_rows(x, codes, S=None, in_rep=1, out=None):
    """x [B, C, H, W] -> [B * in_rep, C, H, W]: output row r is input row r // in_rep under the code codes[(r % S) % len(codes)], a flip
    and / or transposition of its planes (idiff_dihedral_rows).  codes: a host list of 1 to 8 ints in [0, 8): bit 0 = transpose, bit 1 =
    flip H, bit 2 = flip W, the flips after the transposition -- x.transpose(-1, -2) if bit 0, then .flip(-2) if bit 1, then .flip(-1) if
    bit 2.  S (None: the number of output rows, so row r simply takes code r % len(codes)) is the period of the member index, as in the
    B*S rows of an ensemble.  W must be a multiple of 4 and a transposing code needs H == W; out, if given, must not overlap x.  One
    launch; a pure permutation, bit for bit."""
    lib = _lib.load()
    codes = list(codes)
    if not 1 <= len(codes) <= 8 or any(not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < 8 for k in codes):
        raise ValueError(f"dihedral_rows: codes must be 1 to 8 ints in [0, 8), got {codes}")
    if isinstance(in_rep, bool) or not isinstance(in_rep, int) or in_rep < 1:
        raise ValueError(f"dihedral_rows: in_rep must be an int >= 1, got {in_rep!r}")
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"dihedral_rows: x must be a [B, C, H, W] tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    B, Cc, H, W = x.shape
    R = B * in_rep
    S = R if S is None else S
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"dihedral_rows: S must be an int >= 1 (or None: the number of output rows), got {S!r}")
    if W % 4:
        raise ValueError(f"dihedral_rows: the image width {W} is not a multiple of 4")
    if H != W and any(k & 1 for k in codes):
        raise ValueError(f"dihedral_rows: a transposing code needs a square image, got {H} x {W} with codes {codes}")
    _c(x, "x")
    if out is None:
        out = torch.empty((R, Cc, H, W), device=x.device, dtype=torch.float32)
    _c(out, "out")
    if tuple(out.shape) != (R, Cc, H, W):
        raise _lib.IdiffError(f"dihedral_rows: out must be {(R, Cc, H, W)}, got {tuple(out.shape)}")
    packed = 0
    for i, k in enumerate(codes):
        packed |= k << (3 * i)
    check(lib.idiff_dihedral_rows(_p(x), _p(out), R, Cc, H, W, in_rep, S, len(codes), packed, _stream()), "dihedral_rows")
    return out


def plane_sum(x):
    """x [B, C, H, W] -> [B, C]: the sum over the pixels of every plane"""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc), device=x.device, dtype=torch.float32)
    check(lib.idiff_plane_sum(_p(x), _bs(x, "x"), _p(out), B, Cc, H * W, _stream()), "plane_sum")
    return out


# ---- tiled sampling (include/idiff.h; the plan is models/SDEs/driftSDE.py's TilePlan, moved to the device by plan.to(device)) ----
def _tile_args(plan, full, name):
    """(B, C, H, W, ny, nx, Ph, Pw) of a full image under a device plan, after the shape checks"""
    if full.dim() != 4 or tuple(full.shape[2:]) != (plan.H, plan.W):
        raise _lib.IdiffError(f"{name}: the image must be [B, C, {plan.H}, {plan.W}] for this plan, got {tuple(full.shape)}")
    for t, dt in ((plan.ytab, torch.int32), (plan.xtab, torch.int32), (plan.ywt, torch.float32), (plan.xwt, torch.float32)):
        _c(t, "plan table", dt)
    return (full.shape[0], full.shape[1], plan.H, plan.W, plan.ny, plan.nx, plan.Ph, plan.Pw)


def tile_gather(full, plan, out=None):
    """full [B, C, H, W] -> windows [B*ny*nx, C, Ph, Pw], row (b*ny + iy)*nx + ix = full[b, :, oy[iy]:+Ph, ox[ix]:+Pw]"""
    lib = _lib.load()
    _c(full, "full")
    dims = _tile_args(plan, full, "tile_gather")
    B, Cc = dims[:2]
    shape = (B * plan.ny * plan.nx, Cc, plan.Ph, plan.Pw)
    if out is None:
        out = torch.empty(shape, device=full.device, dtype=torch.float32)
    _c(out, "out")
    assert tuple(out.shape) == shape, (tuple(out.shape), shape)
    check(lib.idiff_tile_gather(_p(full), _p(out), *dims, C.c_void_p(plan.ytab.data_ptr()), C.c_void_p(plan.xtab.data_ptr()), _stream()),
          "tile_gather")
    return out


def drift_reverse_step_tiled_dev(x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, plan, coef, state, seed, nper,
                                 offset_base=0):
    """the step of a tiled chain, in place on the full image x [B, C, H, W]: blends the window predictions r_tiles / e_tiles
    [B*ny*nx, C, Ph, Pw], updates x as drift_reverse_step_dev (coef [3, T+1], r_prev = e_prev = None) or drift_reverse_step2_dev (coef
    [5, T+1], full-image history) does, and scatters x and x - cond into x_tiles / xa_tiles"""
    lib = _lib.load()
    _c(x, "x"), _c(r_tiles, "r_tiles"), _c(e_tiles, "e_tiles"), _c(r_prev, "r_prev"), _c(e_prev, "e_prev"), _c(z_base, "z"), _c(cond, "cond")
    _c(x_tiles, "x_tiles"), _c(xa_tiles, "xa_tiles"), _c(coef, "coef"), _c(state, "state", torch.int32)
    dims = _tile_args(plan, x, "drift_reverse_step_tiled_dev")
    nt = dims[0] * plan.ny * plan.nx * dims[1] * plan.Ph * plan.Pw
    _step_tables(coef, (3, 5), state)
    for t in (r_tiles, e_tiles, x_tiles, xa_tiles):
        assert t.numel() == nt, (t.numel(), nt)
    for t in (r_prev, e_prev, cond):
        assert t is None or t.numel() == x.numel()
    assert z_base is None or (z_base.numel() % x.numel() == 0 and z_base.numel() >= x.numel())
    check(lib.idiff_drift_reverse_step_tiled_dev(_p(x), _p(r_tiles), _p(e_tiles), _p(r_prev), _p(e_prev), _p(z_base), _p(cond), _p(x_tiles),
                                                 _p(xa_tiles), *dims, C.c_void_p(plan.ytab.data_ptr()), _p(plan.ywt),
                                                 C.c_void_p(plan.xtab.data_ptr()), _p(plan.xwt), _p(coef), coef.shape[0], coef.shape[1],
                                                 C.c_void_p(state.data_ptr()), seed, nper, offset_base, _stream()),
          "drift_reverse_step_tiled_dev")


def drift_reverse_step_tiled_members_dev(x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, plan, coef, state, members,
                                         seed):
    """drift_reverse_step_tiled_dev on the rows of an ensemble: x [R, C, H, W] holds one member of one image per row, the window
    buffers [R*ny*nx, C, Ph, Pw], and row r's z comes from member members[r]'s stream (int64 [R] on the device) at draw 1 + state[1],
    as in drift_reverse_step_members_dev, or from z_base [steps, R, C, H, W]"""
    lib = _lib.load()
    _c(x, "x"), _c(r_tiles, "r_tiles"), _c(e_tiles, "e_tiles"), _c(r_prev, "r_prev"), _c(e_prev, "e_prev"), _c(z_base, "z"), _c(cond, "cond")
    _c(x_tiles, "x_tiles"), _c(xa_tiles, "xa_tiles"), _c(coef, "coef"), _c(state, "state", torch.int32)
    dims = _tile_args(plan, x, "drift_reverse_step_tiled_members_dev")
    R = dims[0]
    nt = R * plan.ny * plan.nx * dims[1] * plan.Ph * plan.Pw
    _step_tables(coef, (3, 5), state)
    for t in (r_tiles, e_tiles, x_tiles, xa_tiles):
        if t.numel() != nt:
            raise _lib.IdiffError(f"drift_reverse_step_tiled_members_dev: a window buffer holds {t.numel()} elements, the plan needs {nt}")
    for t in (r_prev, e_prev, cond):
        assert t is None or t.numel() == x.numel()
    assert z_base is None or (z_base.numel() % x.numel() == 0 and z_base.numel() >= x.numel())
    if members is None:
        raise _lib.IdiffError("drift_reverse_step_tiled_members_dev: members is required (int64 [R] on the device, from member_ids())")
    check(lib.idiff_drift_reverse_step_tiled_members_dev(_p(x), _p(r_tiles), _p(e_tiles), _p(r_prev), _p(e_prev), _p(z_base), _p(cond),
                                                         _p(x_tiles), _p(xa_tiles), *dims, C.c_void_p(plan.ytab.data_ptr()), _p(plan.ywt),
                                                         C.c_void_p(plan.xtab.data_ptr()), _p(plan.xwt), _p(coef), coef.shape[0],
                                                         coef.shape[1], C.c_void_p(state.data_ptr()), _members(members, R), seed, _stream()),
          "drift_reverse_step_tiled_members_dev")


def step_state_advance(state, tdev, T, t_stop=0):
    lib = _lib.load()
    _c(tdev, "tdev")
    check(lib.idiff_step_state_advance(C.c_void_p(state.data_ptr()), _p(tdev), tdev.numel(), T, t_stop, _stream()), "step_state_advance")


def step_state_advance_table(state, tdev, next_t, t_first, t_stop=0):
    """few-step form: t <- next_t[t] (int32 [T+1] on the device), back to t_first once t <= t_stop"""
    lib = _lib.load()
    _c(tdev, "tdev"), _c(state, "state", torch.int32), _c(next_t, "next_t", torch.int32)
    assert state.numel() == 3 and next_t.dim() == 1
    check(lib.idiff_step_state_advance_table(C.c_void_p(state.data_ptr()), _p(tdev), tdev.numel(), C.c_void_p(next_t.data_ptr()),
                                             next_t.numel(), t_first, t_stop, _stream()), "step_state_advance_table")


def randn(shape, device, seed, offset=0):
    lib = _lib.load()
    out = torch.empty(shape, device=device, dtype=torch.float32)
    check(lib.idiff_randn(_p(out), out.numel(), seed, offset, _stream()), "randn")
    return out


def dropout(x, p, seed, offset, out=None):
    """inverted dropout with the Philox-keyed mask of (seed, offset): x / (1-p) where kept, else 0 (the backward is the same call)"""
    lib = _lib.load()
    _c(x, "x")
    if out is None:
        out = torch.empty_like(x)
    check(lib.idiff_dropout(_p(x), _p(out), x.numel(), float(p), int(seed), int(offset), _stream()), "dropout")
    return out


def philox_raw(ncounters, device, seed, offset=0):
    lib = _lib.load()
    out = torch.empty((ncounters, 4), device=device, dtype=torch.int32)
    check(lib.idiff_philox_raw(_p(out), ncounters, seed, offset, _stream()), "philox_raw")
    return out


def axpby(x, y, alpha, beta, out=None):
    lib = _lib.load()
    _c(x, "x"), _c(y, "y")
    if out is None:
        out = torch.empty_like(x)
    check(lib.idiff_axpby(_p(x), _p(y), _p(out), x.numel(), alpha, beta, _stream()), "axpby")
    return out


def mix3_per_sample(x0, cond, eps, c0, c1, c2):
    lib = _lib.load()
    for t in (x0, cond, eps, c0, c1, c2):
        _c(t)
    B = x0.shape[0]
    out = torch.empty_like(x0)
    check(lib.idiff_mix3_per_sample(_p(x0), _p(cond), _p(eps), _p(c0), _p(c1), _p(c2), _p(out), B, x0.numel() // B, _stream()),
          "mix3_per_sample")
    return out


def f32_to_bf16(x, out=None):
    """flat fp32 -> bf16 (round to nearest even), the wire format of the gradient all-reduce"""
    lib = _lib.load()
    _c(x, "x")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _c(out, "out", torch.bfloat16)
    check(lib.idiff_f32_to_bf16(_p(x), C.c_void_p(out.data_ptr()), x.numel(), _stream()), "f32_to_bf16")
    return out


def bf16_to_f32(x, out=None):
    lib = _lib.load()
    _c(x, "x", torch.bfloat16)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _c(out, "out")
    check(lib.idiff_bf16_to_f32(C.c_void_p(x.data_ptr()), _p(out), x.numel(), _stream()), "bf16_to_f32")
    return out

