"""The forward convolution's direct kernel (conv_igemm_kernel<KS, CK, TWL, MODE, VECW, MB, SPEC> in csrc/conv_igemm.hip), one table row
per reachable instantiation (conv_branch_rows.ROWS: 65 of 65, mirrored without a GPU by test_conv_branches_cpu.py), in the style of
test_train_kernels_gpu.py and test_step_kernels_gpu.py; then the kernel-selection ladder of idiff_conv2d_fwd at its edges, one row per
argument check of the call, and the fused output layer (csrc/conv_select.hip) forward and backward.

Every row runs the HIP kernel and compares it with a plain torch float64 evaluation on the CPU of the formula written in
conv_branch_ref.py.  No row's reference is another kernel of this library.  Every direct-kernel row asks for the direct kernel by name
and asserts idiff_conv2d_last_algo() == 0; which INSTANTIATION that is follows from the launcher's rule (conv_branch_rows.expected_branch)
and was confirmed once from a kernel trace (profiles/r08/conv_branches.txt).

Metric: max|got - ref| / max|ref| per output tensor; rows with a partial tile (ragged H or W, Cout not a multiple of the channel block)
also check the last tile row, the last tile column and the last channel block element by element against tol * max|ref|.
Tolerances are the project's existing ones: 2e-6 of the output range for the direct kernel (_conv_tol of test_ops_gpu.py: 6e-6 F(2x2),
4e-5 F(4x4), 2e-6 bf16x3), 1e-5 for statistics totals, 2e-5 per tile, 1e-5 for the select kernels' gradients.  Rows whose inputs carry a
DC offset or that run silu_fast (prologue, aux term) take max(that, 4 x the error of the SAME formula evaluated in fp32 torch on the
CPU against the fp64 one); both numbers are in the assertion message.  No bound was chosen from what the kernels return."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops  # noqa: E402
from instancediff_amd._lib import ConvDesc  # noqa: E402
from instancediff_amd.ops import _bs, _p, _stream  # noqa: E402

from conv_branch_ref import gn_affine, make_inputs, reference, tile_stats  # noqa: E402
from conv_branch_rows import ROWS, _float_offset, batch_stride, expected_branch, out_size, tile_shape  # noqa: E402
from conv_guard_util import DEV, SENT, _buf, _check, _floor, _guard_intact, _pad  # noqa: E402

E_BADARG, E_UNSUPPORTED = -1, -2
DIRECT, WINO, WINO4, WINO4H, X3, BF16 = 0, 1, 3, 4, 5, 6
TOL_ALGO = {0: 2e-6, 1: 6e-6, 3: 4e-5, 4: 4e-5, 5: 2e-6}  # _conv_tol of test_ops_gpu.py
TOL_OUT, TOL_SUM, TOL_TILE, TOL_GRAD = 2e-6, 1e-5, 2e-5, 1e-5
IDS = [r["name"] for r in ROWS]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _tails(row, Hout, Wout):
    """the last (partial) tile column, tile row and channel block of a row's output"""
    ks, mode, twl, vecw, mb, spec = row["claim"]
    out = []
    if twl != 8:
        TH, TW = tile_shape(twl)
        if Wout % TW:
            out.append(("last tile column", (slice(None), slice(None), slice(None), slice((Wout // TW) * TW, None))))
        if Hout % TH:
            out.append(("last tile row", (slice(None), slice(None), slice((Hout // TH) * TH, None))))
    bm = 32 * mb
    if row["Cout"] % bm:
        out.append(("last channel block", (slice(None), slice((row["Cout"] // bm) * bm, None))))
    return out


# ---- 1. one row per instantiation of the direct kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_direct_kernel_branch(row):
    lib = _lib.load()
    name = row["name"]
    assert row["claim"] == expected_branch(row)
    inp = make_inputs(row, 1000 + IDS.index(name))
    ref, raw = reference(row, inp)
    B, C0, C1, Cout, ks, mode = (row[k] for k in ("B", "C0", "C1", "Cout", "ks", "mode"))
    Hout, Wout = out_size(row)
    sl, odd = row["slices"], row["odd"]
    for k in list(sl) + list(odd):
        assert k in ("src0", "src1", "res", "aux", "out", "wpk"), k

    _, x0 = _buf(inp["src0"].shape, sl.get("src0", 0), "src0" in odd, inp["src0"])
    assert _bs(x0) == batch_stride(row, "src0", C0, row["Hin"] * row["Win"])
    x1 = None
    if C1:
        _, x1 = _buf(inp["src1"].shape, sl.get("src1", 0), "src1" in odd, inp["src1"])
    wpk = ops.pack_conv_weight(inp["w"].to(DEV))
    if "wpk" in odd:
        wflat = torch.zeros((wpk.numel() + 8,), device=DEV, dtype=torch.float32)
        wv = wflat[1:1 + wpk.numel()].view(wpk.shape)
        wv.copy_(wpk)
        wpk = wv
    assert (wpk.data_ptr() % 16 == 0) == ("wpk" not in odd)
    assert (x0.data_ptr() % 16 == 0) == (_float_offset(row, "src0", row["Hin"] * row["Win"]) % 4 == 0)
    kw = {}
    if row["pro"]:
        kw["pro"] = tuple(t.to(DEV) for t in inp["pro"])
    if row["res"]:
        kw["res"] = _buf(inp["res"].shape, sl.get("res", 0), "res" in odd, inp["res"])[1]
    if row["vec"]:
        kw["vec"] = inp["vec"].to(DEV)
    if row["aux"]:
        t, aa, ab = inp["aux"]
        kw["aux"] = (_buf(t.shape, sl.get("aux", 0), "aux" in odd, t)[1], aa.to(DEV), ab.to(DEV))
    oflat, out = _buf((B, Cout, Hout, Wout), sl.get("out", 0), False)
    guards = [(oflat, out, "out")]
    if row["gn"]:
        nt = lib.idiff_conv2d_num_tiles(Hout, Wout)
        bufs = [_pad((B, nt, Cout, 2)), _pad((B, Cout)), _pad((B, Cout))]
        guards += [(f, v, w) for (f, v), w in zip(bufs, ("stats", "gn a", "gn b"))]
        kw["gn"] = dict(groups=row["gn"], gamma=inp["gamma"].to(DEV), beta=inp["beta"].to(DEV), bufs=[v for _, v in bufs])

    got = ops.conv2d(x0, wpk, None if inp["bias"] is None else inp["bias"].to(DEV), ks, Cout, src1=x1, mode=mode, out=out,
                     want_stats=row["stats"], algo=ops.CONV_ALGO_DIRECT, **kw)
    assert lib.idiff_conv2d_last_algo() == DIRECT
    torch.cuda.synchronize()
    stats = gnab = None
    if row["gn"]:
        got, gnab, stats = got
    elif row["stats"]:
        got, stats = got
    assert got.data_ptr() == out.data_ptr()

    loose = row["dc"] or row["pro"] or row["aux"]
    ref32 = raw32 = None
    if loose:
        ref32, raw32 = reference(row, inp, torch.float32)
    tol = _floor(TOL_OUT, ref32, ref) if loose else TOL_OUT
    _check(name, "out", out, ref, tol, _tails(row, Hout, Wout), base=TOL_OUT)
    for flat, view, what in guards:
        _guard_intact(flat, view, f"{name} {what}")
    if stats is not None:
        st = tile_stats(raw)
        assert tuple(stats.shape) == tuple(st.shape), (stats.shape, st.shape)
        s = stats.double().cpu()
        for w, what in ((0, "sum"), (1, "sumsq")):
            tsum, ttile = TOL_SUM, TOL_TILE
            if row["dc"] or row["pro"]:
                st32 = tile_stats(raw32)
                tsum, ttile = _floor(TOL_SUM, st32.sum(1)[..., w], st.sum(1)[..., w]), _floor(TOL_TILE, st32[..., w], st[..., w])
            _check(name, f"stats {what} total", s.sum(1)[..., w], st.sum(1)[..., w], tsum, base=TOL_SUM)
            _check(name, f"stats {what} per tile", s[..., w], st[..., w], ttile, base=TOL_TILE)
    if gnab is not None:
        a, b = gn_affine(raw, row["gn"], inp["gamma"], inp["beta"])
        a32, b32 = gn_affine(raw32 if raw32 is not None else raw.float(), row["gn"], inp["gamma"], inp["beta"])
        _check(name, "gn a", gnab[0], a, _floor(TOL_SUM, a32, a), base=TOL_SUM)
        _check(name, "gn b", gnab[1], b, _floor(TOL_SUM, b32, b), base=TOL_SUM)


# ---- 2. the selection ladder of idiff_conv2d_fwd at its edges --------------------------------------------------------------------
def _mkdesc(x0, wpk, out, ks, Cout, mode=0, x1=None, req=0):
    d = ConvDesc()
    d.src0, d.src0_bstride, d.C0 = x0.data_ptr(), _bs(x0), x0.shape[1]
    if x1 is not None:
        d.src1, d.src1_bstride, d.C1 = x1.data_ptr(), _bs(x1), x1.shape[1]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = x0.shape[0], x0.shape[2], x0.shape[3], mode, ks, Cout
    d.wpk = wpk.data_ptr()
    if ks == 3 and hasattr(wpk, "wino"):
        d.wwino = wpk.wino.data_ptr()
        if hasattr(wpk, "wino4"):
            d.wwino4 = wpk.wino4.data_ptr()
    if ks == 1 and hasattr(wpk, "x3"):
        d.wx3 = wpk.x3.data_ptr()
    d.out, d.out_bstride = out.data_ptr(), _bs(out)
    d.algo_request = req
    return d


def _soft(a):
    return -(1 + a)


def _hard(a):
    return 1 + a


# name, ks, C0, Cout, H, W, algo_request, expected IDIFF_CONV_ALGO_* (None: IDIFF_E_BADARG and nothing written)
# items16 = ceil(W/32) * ceil(H/16) * ceil(Cout/64) per sample, items8 = ceil(W/32) * ceil(H/8) * ceil(Cout/64)
LADDER = [
    ("items16-15-items8-30-half-patch", 3, 32, 192, 80, 32, 0, WINO4H),
    ("items16-16-16x32", 3, 32, 256, 64, 32, 0, WINO4),
    ("items8-15-F2x2", 3, 32, 192, 40, 32, 0, WINO),
    ("items8-16-half-patch", 3, 32, 256, 32, 32, 0, WINO4H),
    ("Cin8-items16-16-not-16x32-half-patch", 3, 8, 128, 64, 64, 0, WINO4H),
    ("Cin8-small-F2x2", 3, 8, 64, 32, 32, 0, WINO),
    ("Cin8-hard-16x32-refused", 3, 8, 64, 32, 32, _hard(WINO4), None),
    ("Cin16-hard-16x32-threshold-waived", 3, 16, 64, 32, 32, _hard(WINO4), WINO4),
    ("W22-direct", 3, 32, 64, 32, 22, 0, DIRECT),
    ("W24-small-F2x2", 3, 32, 64, 64, 24, 0, WINO),
    ("W24-items16-16-partial-patch", 3, 32, 256, 64, 24, 0, WINO4),
    ("soft-16x32-H30-falls-to-F2x2", 3, 32, 64, 30, 36, _soft(WINO4), WINO),
    ("soft-16x32-W22-falls-to-direct", 3, 32, 64, 32, 22, _soft(WINO4), DIRECT),
    ("soft-F2x2-odd-H-falls-to-direct", 3, 32, 64, 31, 32, _soft(WINO), DIRECT),
    ("soft-x3-on-3x3-library-choice", 3, 32, 64, 32, 32, _soft(X3), WINO),
    ("soft-half-patch-taken-below-threshold", 3, 32, 64, 32, 32, _soft(WINO4H), WINO4H),
    ("soft-direct-taken", 3, 32, 256, 64, 32, _soft(DIRECT), DIRECT),
    ("hard-direct-taken", 3, 32, 256, 64, 32, _hard(DIRECT), DIRECT),
    ("hard-16x32-H30-refused", 3, 32, 64, 30, 36, _hard(WINO4), None),
    ("hard-half-patch-W22-refused", 3, 32, 64, 32, 22, _hard(WINO4H), None),
    ("hard-F2x2-odd-H-refused", 3, 32, 64, 31, 32, _hard(WINO), None),
    ("hard-x3-on-3x3-refused", 3, 32, 64, 32, 32, _hard(X3), None),
    ("hard-bf16-without-image-refused", 3, 32, 64, 32, 32, _hard(BF16), None),
    ("1x1-HW256-W16-not-flattened-direct", 1, 64, 64, 16, 16, 0, DIRECT),
    ("1x1-HW256-W32-x3", 1, 64, 64, 8, 32, 0, X3),
]


@pytest.mark.parametrize("name,ks,C0,Cout,H,W,req,want", LADDER, ids=[r[0] for r in LADDER])
def test_selection_ladder(name, ks, C0, Cout, H, W, req, want):
    lib = _lib.load()
    g = _g(4000 + [r[0] for r in LADDER].index(name))
    B = 2
    x = torch.randn(B, C0, H, W, generator=g)
    w = torch.randn(Cout, C0, ks, ks, generator=g) / math.sqrt(C0 * ks * ks)
    assert ops.WINOGRAD and ops.WINOGRAD4 and ops.X3, "the ladder is tested at the process-wide switches' defaults"
    wpk = ops.pack_conv_weight(w.to(DEV))
    xd = x.to(DEV)
    oflat, out = _pad((B, Cout, H, W))
    d = _mkdesc(xd, wpk, out, ks, Cout, req=req)
    planned = lib.idiff_conv2d_plan(ctypes.byref(d))
    rc = lib.idiff_conv2d_fwd(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    if want is None:
        assert planned == E_BADARG and rc == E_BADARG, (name, planned, rc)
        assert bool((oflat == SENT).all()), f"{name}: a refused call wrote to out"
        return
    assert rc == 0, (name, rc, lib.idiff_last_error())
    assert planned == want and lib.idiff_conv2d_last_algo() == want, (name, planned, lib.idiff_conv2d_last_algo(), want)
    ref = F.conv2d(x.double(), w.double(), None, padding=ks // 2)
    _check(name, "out", out, ref, TOL_ALGO[want])
    _guard_intact(oflat, out, name)


# ---- 3. one row per argument check of idiff_conv2d_fwd ---------------------------------------------------------------------------
def _reject_base():
    """a valid 3x3 call (B 2, 8 -> 8 channels, 8x8) with every optional operand allocated but not attached; out is roomy enough for the
    upsample rows to reach the check they are about"""
    t = dict(x=torch.zeros(2, 8, 8, 8, device=DEV), x1=torch.zeros(2, 4, 8, 8, device=DEV), w=torch.zeros(49 * 12 * 8, device=DEV),
             pa=torch.zeros(2, 8, device=DEV), pb=torch.zeros(2, 8, device=DEV), aux=torch.zeros(2, 8, 16, 16, device=DEV),
             aa=torch.zeros(2, 8, device=DEV), ab=torch.zeros(2, 8, device=DEV), stats=torch.full((2, 8, 8, 2), SENT, device=DEV),
             ga=torch.full((2, 8), SENT, device=DEV), gb=torch.full((2, 8), SENT, device=DEV),
             out=torch.full((2, 8, 16, 16), SENT, device=DEV))
    d = ConvDesc()
    d.src0, d.src0_bstride, d.C0 = t["x"].data_ptr(), 8 * 64, 8
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = 2, 8, 8, 0, 3, 8
    d.wpk, d.out, d.out_bstride = t["w"].data_ptr(), t["out"].data_ptr(), 8 * 256
    return d, t


def _two(d, t):
    d.src1, d.src1_bstride, d.C1 = t["x1"].data_ptr(), 4 * 64, 4


def _pro(d, t):
    d.pro_a, d.pro_b = t["pa"].data_ptr(), t["pb"].data_ptr()


def _gnf(d, t, groups, stats=True):
    d.gn_out_a, d.gn_out_b, d.gn_groups, d.gn_eps = t["ga"].data_ptr(), t["gb"].data_ptr(), groups, 1e-5
    if stats:
        d.stats = t["stats"].data_ptr()


def _set(**kw):
    def f(d, t):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _both(*fs):
    def f(d, t):
        for fn in fs:
            fn(d, t)
    return f


REJECT = [
    ("null-out", _set(out=None), "null pointer"),
    ("B-0", _set(B=0), "bad dims"),
    ("ks-5", _set(ks=5), "ks must be 1, 3 or 7"),
    ("mode-3", _set(mode=3), "bad mode"),
    ("C1-without-src1", _set(C1=4), "src1/C1 mismatch"),
    ("src1-without-C1", lambda d, t: setattr(d, "src1", t["x1"].data_ptr()), "src1/C1 mismatch"),
    ("prologue-with-two-sources", _both(_two, _pro), "prologue needs a single source"),
    ("pro_a-alone", lambda d, t: setattr(d, "pro_a", t["pa"].data_ptr()), "pro_a/pro_b"),
    ("pro_b-alone", lambda d, t: setattr(d, "pro_b", t["pb"].data_ptr()), "pro_a/pro_b"),
    ("aux-without-affine", lambda d, t: (setattr(d, "aux", t["aux"].data_ptr()), setattr(d, "aux_bstride", 8 * 256)), "aux needs aux_a/aux_b"),
    ("aux-with-aux_a-only", lambda d, t: (setattr(d, "aux", t["aux"].data_ptr()), setattr(d, "aux_bstride", 8 * 256),
                                          setattr(d, "aux_a", t["aa"].data_ptr())), "aux needs aux_a/aux_b"),
    ("unshuffle-ks-3", _set(mode=2), "unshuffle mode needs ks=1"),
    ("unshuffle-two-sources", _both(_set(mode=2, ks=1), _two), "unshuffle mode needs ks=1 and a single source"),
    ("unshuffle-odd-H", _set(mode=2, ks=1, Hin=7), "unshuffle needs even H, W"),
    ("unshuffle-odd-W", _set(mode=2, ks=1, Win=7), "unshuffle needs even H, W"),
    ("upsample-ks-1", _set(mode=1, ks=1), "upsample mode needs ks=3"),
    ("ks-7-upsample", _set(mode=1, ks=7), "ks=7 needs normal mode"),
    ("src0-bstride-one-below-dense", _set(src0_bstride=8 * 64 - 1), "src0_bstride too small"),
    ("src1-bstride-one-below-dense", _both(_two, _set(src1_bstride=4 * 64 - 1)), "src1_bstride too small"),
    ("out-bstride-one-below-dense", _set(out_bstride=8 * 64 - 1), "out_bstride too small"),
    ("out-bstride-one-below-dense-upsample", _set(mode=1, out_bstride=8 * 256 - 1), "out_bstride too small"),
    ("algo-request-8", _set(algo_request=8), "bad algo_request"),
    ("algo-request-minus-8", _set(algo_request=-8), "bad algo_request"),
    ("algo-request-wgrad-only-stream1x1", _set(algo_request=3), "bad algo_request"),
    ("operands-2", _set(operands=2), "bad operands"),
    ("finalize-without-stats", lambda d, t: _gnf(d, t, 2, stats=False), "GroupNorm finalize needs stats"),
    ("finalize-groups-3-of-8", lambda d, t: _gnf(d, t, 3), "GroupNorm finalize needs stats"),
    ("finalize-without-gn_out_b", lambda d, t: (_gnf(d, t, 2), setattr(d, "gn_out_b", None)), "GroupNorm finalize needs stats"),
]


@pytest.mark.parametrize("name,mutate,fragment", REJECT, ids=[r[0] for r in REJECT])
def test_conv2d_rejections_return_badarg_and_write_nothing(name, mutate, fragment):
    lib = _lib.load()
    d, t = _reject_base()
    assert lib.idiff_conv2d_plan(ctypes.byref(d)) == DIRECT, "the base call itself is valid"
    mutate(d, t)
    planned = lib.idiff_conv2d_plan(ctypes.byref(d))
    rc = lib.idiff_conv2d_fwd(ctypes.byref(d), _stream())
    msg = lib.idiff_last_error().decode()
    torch.cuda.synchronize()
    assert rc == E_BADARG and planned == E_BADARG, (name, rc, planned, msg)
    assert fragment in msg, (name, msg)
    for k in ("out", "stats", "ga", "gb"):
        assert bool((t[k] == SENT).all()), f"{name}: a refused call wrote to {k}"


def test_conv2d_grid_limit_is_an_argument_error():
    """B * ntiles * ncob >= 2^31 workgroups: refused by the plan (no launch, no memory touched: the pointers only have to be non-null)"""
    lib = _lib.load()
    d, t = _reject_base()
    d.ks, d.Cout = 1, 8
    d.B, d.Hin, d.Win = 65536, 1024, 8192  # 128 x 256 tiles of 8x32 = 32768 per sample, one channel block
    d.src0_bstride = d.out_bstride = 8 * 1024 * 8192
    assert lib.idiff_conv2d_plan(ctypes.byref(d)) == E_BADARG
    assert "grid too large" in lib.idiff_last_error().decode()
    d.B = 65535
    assert lib.idiff_conv2d_plan(ctypes.byref(d)) == DIRECT


def _direct_lds_bytes(ks, twl, mb, pro_channels):
    """launch_conv's LDS request: two staging buffers (input patch with halo + weight tile), the prologue table, 4 * BM constants"""
    ck = {3: 8, 1: 16, 7: 2}[ks]
    th, tw = tile_shape(twl)
    in_tile = (ck * (th + ks - 1) * (tw + ks - 1) + 3) // 4 * 4
    w_tile = ks * ks * ck * 32 * mb
    return (2 * (in_tile + w_tile) + 2 * pro_channels + 4 * 32 * mb) * 4


def test_conv2d_lds_ceiling():
    """conv_igemm_kernel<1, 16, 3, NORMAL, true, 1, 0> with a prologue: the table of 2 * C0 floats takes the request over 160 KiB at
    C0 = 15809 (IDIFF_E_UNSUPPORTED before any launch); C0 = 15808 asks for exactly 160 KiB and runs"""
    lib = _lib.load()
    c_bad = next(c for c in range(1, 1 << 20) if _direct_lds_bytes(1, 3, 1, c) > 160 * 1024)
    assert c_bad == 15809 and _direct_lds_bytes(1, 3, 1, c_bad - 1) == 160 * 1024
    B, Cout, H, W = 1, 4, 8, 8
    for C0 in (c_bad, c_bad - 1):
        row = dict(name=f"lds-C{C0}", ks=1, mode=0, B=B, C0=C0, C1=0, Cout=Cout, Hin=H, Win=W, pro=True, res=False, vec=False, aux=False,
                   bias=True, stats=False, gn=0, slices={}, odd=(), dc=False)
        assert expected_branch(row) == (1, 0, 3, 1, 1, 0)
        inp = make_inputs(row, 77)
        oflat, out = _pad((B, Cout, H, W))
        args = (inp["src0"].to(DEV), ops.pack_conv_weight(inp["w"].to(DEV)), inp["bias"].to(DEV), 1, Cout)
        kw = dict(pro=tuple(t.to(DEV) for t in inp["pro"]), out=out, algo=ops.CONV_ALGO_DIRECT)
        if C0 == c_bad:
            with pytest.raises(_lib.IdiffError, match=r"\(-2\).*LDS budget exceeded"):
                ops.conv2d(*args, **kw)
            torch.cuda.synchronize()
            assert bool((oflat == SENT).all()), "a refused call wrote to out"
        else:
            ops.conv2d(*args, **kw)
            assert lib.idiff_conv2d_last_algo() == DIRECT
            ref, _ = reference(row, inp)
            ref32, _ = reference(row, inp, torch.float32)
            # K = 15808 is 14 times the longest reduction the 2e-6 of the direct kernel was set on (K = 9 * 128 = 1152).  The kernel sums
            # in one k-ordered fp32 fma chain (the CPU's fp32 conv sums blockwise, so _floor does not see this): K roundings of half an
            # ulp of a partial sum of the output's magnitude walk to sqrt(K) * 2^-24 of the output range.  That model gives 2.0e-6 at
            # K = 1152 -- the project's tolerance -- and 7.5e-6 here.
            tol = max(_floor(TOL_OUT, ref32, ref), math.sqrt(C0) * 2.0 ** -24)
            _check(row["name"], "out", out, ref, tol, base=TOL_OUT)
            _guard_intact(oflat, out, row["name"])


# ---- 4. the fused output layer: 3x3 conv + class gather (csrc/conv_select.hip) ----------------------------------------------------
def _select_ref(x, w, bias, idx):
    """fp64 conv2d over all K classes -> gather of each sample's class"""
    y = F.conv2d(x, w, bias, padding=1)
    return y[torch.arange(x.shape[0]), idx.long()][:, None]


# name, B, C, K, H, W, idx, bias?, extra channels of the buffer x is a slice of
SELECT_FWD = [
    ("C13-channel-tail", 2, 13, 5, 8, 32, [1, 3], True, 0),
    ("C1-5x7", 2, 1, 5, 5, 7, [4, 0], True, 0),
    ("H3-W20-inside-one-tile", 2, 8, 5, 3, 20, [2, 2], True, 0),
    ("W33-one-column-second-tile-H9", 2, 8, 5, 9, 33, [0, 4], True, 0),
    ("every-class-used-one-unused", 5, 16, 6, 8, 32, [4, 0, 3, 1, 2], True, 0),
    ("no-bias-C20", 2, 20, 5, 16, 40, [3, 1], False, 0),
    ("x-channel-slice-C64", 2, 64, 5, 17, 36, [1, 4], True, 6),
]


@pytest.mark.parametrize("name,B,C,K,H,W,idx,has_bias,extra", SELECT_FWD, ids=[r[0] for r in SELECT_FWD])
def test_conv3x3_select_fwd_rows(name, B, C, K, H, W, idx, has_bias, extra):
    g = _g(5000 + [r[0] for r in SELECT_FWD].index(name))
    x = torch.randn(B, C, H, W, generator=g) * 0.5 + (3.0 if "tail" in name or "slice" in name else 0.0)
    w = torch.randn(K, C, 3, 3, generator=g) / math.sqrt(9 * C)
    bias = torch.randn(K, generator=g) if has_bias else None
    idx_t = torch.tensor(idx, dtype=torch.int32)
    ref = _select_ref(x.double(), w.double(), None if bias is None else bias.double(), idx_t)
    _, xd = _buf(x.shape, extra, False, x)
    out = ops.conv3x3_select(xd, w.to(DEV), None if bias is None else bias.to(DEV), idx_t.to(DEV))
    ref32 = _select_ref(x, w, bias, idx_t)
    tails = []
    if W % 32:
        tails.append(("last tile column", (slice(None), slice(None), slice(None), slice((W // 32) * 32, None))))
    if H % 8:
        tails.append(("last tile row", (slice(None), slice(None), slice((H // 8) * 8, None))))
    _check(name, "out", out, ref, _floor(TOL_OUT, ref32, ref), tails, base=TOL_OUT)


# name, B, C, K, H, W, idx, which gradients ("x", "w", "b"), extra channels of the buffer dx is a slice of
SELECT_BWD = [
    ("HW4092-one-tile", 2, 8, 5, 31, 132, [1, 3], "xwb", 0),
    ("HW4096-one-tile-exactly", 2, 8, 5, 64, 64, [0, 4], "xwb", 0),
    ("HW4100-second-tile-of-one-strip", 2, 8, 5, 25, 164, [2, 0], "xwb", 0),
    ("HW4224-two-tiles-two-samples-of-one-class", 3, 12, 5, 32, 132, [3, 1, 3], "xwb", 0),
    ("dx-only", 2, 16, 5, 16, 32, [1, 2], "x", 0),
    ("dw-only-no-db", 2, 16, 5, 16, 32, [4, 4], "w", 0),
    ("dx-slice-guard-band-C5", 2, 5, 4, 12, 20, [0, 3], "xwb", 3),
]


@pytest.mark.parametrize("name,B,C,K,H,W,idx,which,extra", SELECT_BWD, ids=[r[0] for r in SELECT_BWD])
def test_conv3x3_select_bwd_rows(name, B, C, K, H, W, idx, which, extra):
    lib = _lib.load()
    g = _g(6000 + [r[0] for r in SELECT_BWD].index(name))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) / math.sqrt(9 * C)
    bias = torch.randn(K, generator=g)
    dpred = torch.randn(B, 1, H, W, generator=g)
    idx_t = torch.tensor(idx, dtype=torch.int32)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    _select_ref(x64, w64, b64, idx_t).backward(dpred.double())
    ntile = -(-H * W // 4096)
    assert lib.idiff_conv3x3_select_bwd_ws_floats(B, C, H, W) == B * ntile * (C * 9 + 1)
    xd, wd, gd, idd = x.to(DEV), w.to(DEV), dpred.to(DEV), idx_t.to(DEV)
    dxflat, dx = _buf((B, C, H, W), extra, False) if "x" in which else (None, None)
    dwflat, dw = _pad((K, C, 3, 3)) if "w" in which else (None, None)
    dbflat, db = _pad((K,)) if "b" in which else (None, None)
    ws = torch.full((B * ntile * (C * 9 + 1),), SENT, device=DEV) if "w" in which else None
    rc = lib.idiff_conv3x3_select_bwd(_p(xd), _bs(xd), _p(wd), ctypes.c_void_p(idd.data_ptr()), _p(gd), _p(dx), _bs(dx) if dx is not None else 0,
                                      _p(dw), _p(db), _p(ws), B, C, K, H, W, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, lib.idiff_last_error())
    if dx is not None:
        _check(name, "dx", dx, x64.grad, TOL_GRAD)
        _guard_intact(dxflat, dx, f"{name} dx")
    if dw is not None:
        _check(name, "dw", dw, w64.grad, TOL_GRAD)
        _guard_intact(dwflat, dw, f"{name} dw")
        unused = [k for k in range(K) if k not in idx]
        assert unused and bool((dw[unused] == 0).all()), f"{name}: a class without a sample must get a weight gradient of exactly 0"
        if db is not None:
            _check(name, "db", db, b64.grad, TOL_GRAD)
            _guard_intact(dbflat, db, f"{name} db")
            assert bool((db[unused] == 0).all())


def test_conv3x3_select_bwd_rejections():
    lib = _lib.load()
    B, C, K, H, W = 2, 8, 5, 8, 16
    x, w, gd = torch.zeros(B, 257, H, W, device=DEV), torch.zeros(K, 257, 3, 3, device=DEV), torch.zeros(B, 1, H, W, device=DEV)
    idx = torch.zeros(B, dtype=torch.int32, device=DEV)
    dx, dw, db = (torch.full(s, SENT, device=DEV) for s in ((B, 257, H, W), (K, 257, 3, 3), (K,)))
    ws = torch.full((lib.idiff_conv3x3_select_bwd_ws_floats(B, 257, H, W),), SENT, device=DEV)

    def call(C=C, H=H, W=W, ws=ws, dx=dx, dw=dw, xoff=0):
        xp = ctypes.c_void_p(x.data_ptr() + 4 * xoff)
        return lib.idiff_conv3x3_select_bwd(xp, 257 * H * W, _p(w), ctypes.c_void_p(idx.data_ptr()), _p(gd), _p(dx), 257 * H * W, _p(dw), _p(db), _p(ws),
                                            B, C, K, H, W, _stream())

    assert call(H=16, W=8 - 1) == E_BADARG and "W % 4 == 0" in lib.idiff_last_error().decode()
    assert call(C=257) == E_BADARG and "C <= 256" in lib.idiff_last_error().decode()
    assert call(dx=None, dw=None) == E_BADARG and "null pointer" in lib.idiff_last_error().decode()
    assert call(xoff=1) == E_BADARG and "16-byte rows" in lib.idiff_last_error().decode()
    torch.cuda.synchronize()
    for t in (dx, dw, db, ws):
        assert bool((t == SENT).all()), "a refused call wrote to an output"
    assert call(ws=None) == E_BADARG and "workspace" in lib.idiff_last_error().decode()
    torch.cuda.synchronize()
    for t in (dx, dw, db, ws):  # the data gradient is not enqueued either: every check comes before the first launch
        assert bool((t == SENT).all()), "a refused call wrote to an output"
    assert call() == 0
