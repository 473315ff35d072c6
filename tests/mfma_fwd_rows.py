"""The launch-branch tables of the two forward convolution kernels on the bf16 matrix cores behind idiff_conv2d_fwd --
conv1x1_x3_kernel<UNSH> (csrc/conv1x1_x3.hip, IDIFF_CONV_ALGO_X3: 1x1, fp32 operands split three ways, epilogue compiled per
(RES, AUX)) and conv_bf16_kernel<MODE> (csrc/conv_bf16.hip, IDIFF_CONV_ALGO_BF16: 3x3, bf16-rounded operands, opt-in) -- and the
selection ladder that leads to them, shared by the GPU rows of test_mfma_fwd_gpu.py and their CPU mirror test_mfma_fwd_cpu.py.
Plain data and pure Python; nothing here imports the library.

A row has the shape of a row of conv_branch_rows.py plus `kernel`, so conv_branch_ref.make_inputs / reference / tile_stats serve it
unchanged, and the fields of the call: `req` (idiff_conv_desc.algo_request: 1 + algo = hard, -(1 + algo) = soft, 0 = the library
picks), `operands` (1 = bf16), `image` (the weight carries the kernel's image: .x3 of a 1x1, .bf16 of a 3x3), `bs0_plus` (floats
added to src0's batch stride), `transposed` (the image is packed from the transposed matrix, as the data gradient does).

claim:  bf16x3  (X3, UNSH, RES, AUX)            UNSH = pixel-unshuffle gather; RES / AUX = the epilogue's residual / silu(a*aux+b) term
        bf16    (BF16, MODE, prologue, two)     MODE = NORMAL or UPSAMPLE2; a prologue excludes a second source (include/idiff.h)

The rules, from csrc/conv_igemm.hip (conv2d_run), conv1x1_x3_eligible and conv_bf16_eligible:
  bf16    first: ks 3, NORMAL / UPSAMPLE2, a 16-byte-aligned bf16 image, Cout % 64, C0 % 32, C1 % 32, Cin >= 32, Hout % 8, Wout % 32;
          taken when asked for by name, or when operands == 1 and nothing is asked for; a hard request elsewhere is IDIFF_E_BADARG
  bf16x3  then: ks 1, a 16-byte-aligned x3 image, output pixels per sample % 256, Cout % 64, Cin % 8, Cin >= 32, no prologue, no
          statistics; NORMAL: the call flattens (MB 2, 16-byte weight loads: Cout % 4 and wpk aligned, sources and their batch strides
          16-byte aligned, Wout >= 32) and C0 % 8 == 0; UNSHUFFLE2: Wout % 4 == 0, src0 and its batch stride 16-byte aligned;
          taken when asked for by name or when nothing is asked for; a hard request elsewhere is IDIFF_E_BADARG
  else    3x3: F(2x2,3x3) where wino_fwd_rows.eligible says so (every 3x3 row here stays below the 16 items per sample from which the
          F(4x4,3x3) kernels take over: test_conv_branches_gpu.LADDER pins those thresholds), else the direct kernel; 1x1: direct
In the kernel a 1x1 layer is walked in chunks of 32 input channels (unshuffle: 4 * C0 virtual ones), four octets each, channel blocks
of 64 and tiles of 256 consecutive output pixels; a 3x3 layer in chunks of 32, blocks of 64 and 8x32 patches."""
from conv_branch_rows import N, S, SLICE_LO, U, _float_offset, batch_stride, out_size  # noqa: F401
from wino_fwd_rows import eligible as _wino_eligible

DIRECT, WINO, WINO4, WINO4H, X3, BF16 = 0, 1, 3, 4, 5, 6  # IDIFF_CONV_ALGO_*
KERNELS = (X3, BF16)
CKB, BM, TILE = 32, 64, 256


def _hard(a):
    return 1 + a


def _soft(a):
    return -(1 + a)


def _row(name, kernel, ks, mode, C0, C1, Cout, Hin, Win, claim, B=2, **kw):
    row = dict(name=name, kernel=kernel, ks=ks, mode=mode, B=B, C0=C0, C1=C1, Cout=Cout, Hin=Hin, Win=Win, claim=claim, pro=False, res=False,
               vec=False, aux=False, bias=True, stats=False, gn=0, slices={}, odd=(), dc=False, transposed=False, req=0, operands=0,
               image=True, bs0_plus=0, want=None)
    assert set(kw) <= set(row), kw
    row.update(kw)
    if row["gn"]:
        row["stats"] = True
    return row


def _x(name, mode, C0, C1, Cout, Hin, Win, claim, **kw):
    """a bf16x3 table row: asked for by name"""
    return _row(name, X3, 1, mode, C0, C1, Cout, Hin, Win, (X3,) + claim, req=_hard(X3), want=X3, **kw)


def _b(name, mode, C0, C1, Cout, Hin, Win, claim, **kw):
    """a bf16 table row: operands = 1, nothing asked for"""
    return _row(name, BF16, 3, mode, C0, C1, Cout, Hin, Win, (BF16,) + claim, operands=1, want=BF16, **kw)


ROWS = [
    # ---- conv1x1_x3_kernel<false>: claim (UNSH, RES, AUX) ---------------------------------------------------------------------------
    _x("x3-n00-8x32-C32-one-chunk-Cout64-plain", N, 32, 0, 64, 8, 32, (0, 0, 0)),
    _x("x3-n00-8x32-C64-Cout64-no-bias", N, 64, 0, 64, 8, 32, (0, 0, 0), bias=False),
    _x("x3-n00-8x32-C8+24-one-chunk-Cout64-src1-slice", N, 8, 24, 64, 8, 32, (0, 0, 0), slices={"src1": 4}),
    _x("x3-n00-16x32-C40-Cout64-dc", N, 40, 0, 64, 16, 32, (0, 0, 0), dc=True),
    _x("x3-n00-8x32-C64-Cout128-transposed-vec", N, 64, 0, 128, 8, 32, (0, 0, 0), transposed=True, vec=True),
    _x("x3-n10-16x32-C40+24-Cout128-res-slice-vec", N, 40, 24, 128, 16, 32, (0, 1, 0), res=True, vec=True, slices={"res": 4}),
    _x("x3-n10-8x32-C56-Cout64-res-src0-slice-B3", N, 56, 0, 64, 8, 32, (0, 1, 0), B=3, res=True, slices={"src0": 4}),
    _x("x3-n01-8x64-C56+48-four-chunks-Cout128-aux-slice", N, 56, 48, 128, 8, 64, (0, 0, 1), aux=True, slices={"aux": 4}),
    _x("x3-n11-24x32-C80-three-chunks-Cout192-res-aux-vec-out-slice", N, 80, 0, 192, 24, 32, (0, 1, 1), res=True, aux=True, vec=True,
       slices={"out": 4}),
    # ---- conv1x1_x3_kernel<true>: pixel-unshuffle, 4 * C0 virtual channels, output Hin/2 x Win/2 ------------------------------------
    _x("x3-s00-16x64-C8-one-chunk-Cout64-plain", S, 8, 0, 64, 16, 64, (1, 0, 0)),
    _x("x3-s00-32x64-C16-Cout192-out-slice-dc-no-bias", S, 16, 0, 192, 32, 64, (1, 0, 0), dc=True, bias=False, slices={"out": 4}),
    _x("x3-s10-16x64-C10-Cin40-Cout64-res-slice-vec", S, 10, 0, 64, 16, 64, (1, 1, 0), res=True, vec=True, slices={"res": 4}),
    _x("x3-s01-128x8-Wout4-C16-Cout128-aux", S, 16, 0, 128, 128, 8, (1, 0, 1), aux=True),
    _x("x3-s11-128x24-Wout12-C24-three-chunks-Cout64-res-aux-src0-slice", S, 24, 0, 64, 128, 24, (1, 1, 1), res=True, aux=True,
       slices={"src0": 4}),
    # ---- conv_bf16_kernel<NORMAL>: claim (MODE, prologue, two sources) ----------------------------------------------------------------
    _b("bf-n00-8x32-C32-one-chunk-Cout64-plain", N, 32, 0, 64, 8, 32, (N, 0, 0)),
    _b("bf-n00-8x32-C32-Cout64-odd-src0-no-bias", N, 32, 0, 64, 8, 32, (N, 0, 0), odd=("src0",), bias=False),
    _b("bf-n00-8x32-C64-Cout128-res-slice-vec", N, 64, 0, 128, 8, 32, (N, 0, 0), res=True, vec=True, slices={"res": 4}),
    _b("bf-n00-16x64-C32-Cout64-gn8-stats-guard", N, 32, 0, 64, 16, 64, (N, 0, 0), gn=8),
    _b("bf-n00-8x32-C96-three-chunks-Cout64-transposed", N, 96, 0, 64, 8, 32, (N, 0, 0), transposed=True),
    _b("bf-n01-8x32-C32+32-Cout64-src1-slice-B3", N, 32, 32, 64, 8, 32, (N, 0, 1), B=3, slices={"src1": 4}),
    _b("bf-n01-16x64-C64+32-Cout128-stats-out-slice", N, 64, 32, 128, 16, 64, (N, 0, 1), stats=True, slices={"out": 4}),
    _b("bf-n10-8x32-C64-Cout64-pro-aux-slice", N, 64, 0, 64, 8, 32, (N, 1, 0), pro=True, aux=True, slices={"aux": 4}),
    _b("bf-n10-16x64-C64-Cout128-pro-stats", N, 64, 0, 128, 16, 64, (N, 1, 0), pro=True, stats=True),
    # ---- conv_bf16_kernel<UPSAMPLE2>: output 2 Hin x 2 Win ------------------------------------------------------------------------------
    _b("bf-u00-4x16-C32-one-chunk-Cout64-stats", U, 32, 0, 64, 4, 16, (U, 0, 0), stats=True),
    _b("bf-u01-8x32-C32+32-Cout64-res-src0-slice", U, 32, 32, 64, 8, 32, (U, 0, 1), res=True, slices={"src0": 4}),
    _b("bf-u10-4x16-C64-Cout64-pro-vec", U, 64, 0, 64, 4, 16, (U, 1, 0), pro=True, vec=True),
]

# tuples of REACHABLE that no row claims, each with its reason: none -- every one is reachable at the kernels' smallest shapes
LEFT_OUT = {}

REACHABLE = ({(X3, u, r, a) for u in (0, 1) for r in (0, 1) for a in (0, 1)} |         # 8
             {(BF16, m, p, t) for m in (N, U) for (p, t) in ((0, 0), (1, 0), (0, 1))})  # 6: a prologue needs a single source


def cin(row):
    """input channels the kernel walks (unshuffle: four virtual channels per real one)"""
    return (4 * row["C0"] if row["mode"] == S else row["C0"]) + row["C1"]


def nchunks(row):
    return -(-cin(row) // CKB)


def exact(row):
    """the row also runs with integer operands: no silu_fast anywhere (bf16x3: no aux term; bf16: no prologue either)"""
    return not row["aux"] and not row["pro"]


def expected_instantiation(row):
    """the claim: (X3, UNSH, RES, AUX) of conv1x1_x3_kernel<UNSH> and the (RES, AUX) form of its epilogue, or
    (BF16, MODE, prologue, two sources) of conv_bf16_kernel<MODE>"""
    if row["kernel"] == X3:
        return (X3, int(row["mode"] == S), int(row["res"]), int(row["aux"]))
    return (BF16, row["mode"], int(row["pro"]), int(row["C1"] > 0))


def kernel_name(t):
    """the instantiation as the demangled kernel name of a trace spells it"""
    if t[0] == X3:
        return "conv1x1_x3_kernel<%s>" % ("true" if t[1] else "false")
    return "conv_bf16_kernel<%d>" % t[1]


def src0_bstride(row):
    return batch_stride(row, "src0", row["C0"], row["Hin"] * row["Win"]) + row["bs0_plus"]


def _aligned(row, name, plane):
    return _float_offset(row, name, plane) % 4 == 0


def bf16_eligible(row):
    Hout, Wout = out_size(row)
    return (row["ks"] == 3 and row["mode"] in (N, U) and row["image"] and row["Cout"] % BM == 0 and row["C0"] % CKB == 0 and
            row["C1"] % CKB == 0 and cin(row) >= CKB and Hout % 8 == 0 and Wout % 32 == 0)


def flattened(row):
    """the 1x1 NORMAL call runs on 256 consecutive pixels per tile (conv_branch_rows.expected_branch's TWL 8, plus src0's stride)"""
    Hout, Wout = out_size(row)
    plane = row["Hin"] * row["Win"]
    in16 = _aligned(row, "src0", plane) and src0_bstride(row) % 4 == 0
    if row["C1"]:
        in16 = in16 and _aligned(row, "src1", plane) and batch_stride(row, "src1", row["C1"], plane) % 4 == 0
    vecw = row["Cout"] % 4 == 0 and "wpk" not in row["odd"]
    return (row["ks"] == 1 and row["mode"] == N and not row["stats"] and row["Cout"] > 32 and vecw and in16 and (Hout * Wout) % TILE == 0 and
            Wout >= 32)


def x3_eligible(row):
    Hout, Wout = out_size(row)
    hw = Hout * Wout
    if row["ks"] != 1 or not row["image"]:
        return False
    if hw % TILE or hw > (1 << 25) or row["Cout"] % BM or cin(row) % 8 or cin(row) < CKB or row["pro"] or row["stats"]:
        return False
    if row["mode"] == S:
        return not row["C1"] and Wout % 4 == 0 and src0_bstride(row) % 4 == 0 and _aligned(row, "src0", row["Hin"] * row["Win"])
    return row["mode"] == N and flattened(row) and row["C0"] % 8 == 0


def expected_algo(row):
    """what idiff_conv2d_plan answers for the row's call: an IDIFF_CONV_ALGO_*, or None for IDIFF_E_BADARG"""
    hard = row["req"] > 0
    req = abs(row["req"]) - 1  # -1: the library picks
    assert not (row["pro"] and row["C1"]) and (row["mode"] != S or (row["ks"] == 1 and not row["C1"])), "a call the header refuses outright"
    can = bf16_eligible(row)
    if hard and req == BF16 and not can:
        return None
    if can and (req == BF16 or (req == -1 and row["operands"] == 1)):
        return BF16
    can = x3_eligible(row)
    if hard and req == X3 and not can:
        return None
    if can and req in (X3, -1):
        return X3
    if row["ks"] == 3:
        Hout, Wout = out_size(row)
        assert req not in (WINO4, WINO4H) and -(-Wout // 32) * -(-Hout // 8) * -(-row["Cout"] // 64) < 16, "below the F(4x4,3x3) thresholds"
        wino = _wino_eligible(row, WINO)
        if (req in (-1, WINO) or not hard) and req != DIRECT and wino:
            return WINO
        if hard and req == WINO:
            return None
    return DIRECT


# ---- the selection ladder: one case per edge of the rules above; `want` is what a CPU build of the library answered -----------------
def _l1(name, want, C0=32, C1=0, Cout=64, Hin=8, Win=32, mode=N, **kw):
    return _row("1x1-" + name, None, 1, mode, C0, C1, Cout, Hin, Win, None, want=want, **kw)


def _l3(name, want, C0=32, C1=0, Cout=64, Hin=8, Win=32, mode=N, operands=1, **kw):
    return _row("3x3-" + name, None, 3, mode, C0, C1, Cout, Hin, Win, None, want=want, operands=operands, **kw)


LADDER = [
    # 1x1 normal, -> 64 at 8x32 unless noted
    _l1("n-C32", X3),
    _l1("n-C40", X3, C0=40),
    _l1("n-C8+24", X3, C0=8, C1=24),
    _l1("n-C40+24-Cout128", X3, C0=40, C1=24, Cout=128),
    _l1("n-C24-below-a-chunk", DIRECT, C0=24),
    _l1("n-C36-not-whole-octets", DIRECT, C0=36),
    _l1("n-C12+20-octet-spans-the-sources", DIRECT, C0=12, C1=20),
    _l1("n-C12+20-hard-refused", None, C0=12, C1=20, req=_hard(X3)),
    _l1("n-Cout96", DIRECT, Cout=96),
    _l1("n-Cout32-one-half-block", DIRECT, Cout=32),
    _l1("n-16x16-narrow", DIRECT, Hin=16, Win=16),
    _l1("n-9x32-no-whole-tiles", DIRECT, Hin=9),
    _l1("n-prologue", DIRECT, pro=True),
    _l1("n-prologue-hard-refused", None, pro=True, req=_hard(X3)),
    _l1("n-stats", DIRECT, stats=True),
    _l1("n-stats-hard-refused", None, stats=True, req=_hard(X3)),
    _l1("n-src0-4-bytes-off", DIRECT, odd=("src0",)),
    _l1("n-src1-4-bytes-off", DIRECT, C0=8, C1=24, odd=("src1",)),
    _l1("n-wpk-4-bytes-off-no-flattening", DIRECT, odd=("wpk",)),  # the x3 kernel never reads wpk: the flattening rule decides
    _l1("n-src0-bstride-dense+2", DIRECT, bs0_plus=2),
    _l1("n-no-x3-image", DIRECT, image=False),
    _l1("n-no-x3-image-hard-refused", None, image=False, req=_hard(X3)),
    _l1("n-9x32-soft-request", DIRECT, Hin=9, req=_soft(X3)),
    _l1("n-hard-direct", DIRECT, req=_hard(DIRECT)),
    # 1x1 unshuffle, -> 64
    _l1("s-C8-16x64", X3, C0=8, Hin=16, Win=64, mode=S),
    _l1("s-C10-16x64", X3, C0=10, Hin=16, Win=64, mode=S),
    _l1("s-128x24-Wout12", X3, C0=8, Hin=128, Win=24, mode=S),
    _l1("s-128x8-Wout4", X3, C0=8, Hin=128, Win=8, mode=S),
    _l1("s-64x16-Wout8", X3, C0=8, Hin=64, Win=16, mode=S),
    _l1("s-C9-Cin36", DIRECT, C0=9, Hin=16, Win=64, mode=S),
    _l1("s-C4-Cin16", DIRECT, C0=4, Hin=16, Win=64, mode=S),
    _l1("s-Cout96", DIRECT, C0=8, Cout=96, Hin=16, Win=64, mode=S),
    _l1("s-18x64-no-whole-tiles", DIRECT, C0=8, Hin=18, Win=64, mode=S),
    _l1("s-256x12-Wout6", DIRECT, C0=8, Hin=256, Win=12, mode=S),
    _l1("s-256x12-Wout6-hard-refused", None, C0=8, Hin=256, Win=12, mode=S, req=_hard(X3)),
    _l1("s-src0-4-bytes-off", DIRECT, C0=8, Hin=16, Win=64, mode=S, odd=("src0",)),
    _l1("s-prologue", DIRECT, C0=8, Hin=16, Win=64, mode=S, pro=True),
    _l1("s-stats", DIRECT, C0=8, Hin=16, Win=64, mode=S, stats=True),
    # 3x3 with operands = 1, 32 -> 64 at 8x32 unless noted
    _l3("plain", BF16),
    _l3("C32+32", BF16, C1=32),
    _l3("u-C32+32-4x16", BF16, C1=32, Hin=4, Win=16, mode=U),
    _l3("u-prologue-C64-4x16", BF16, C0=64, Hin=4, Win=16, mode=U, pro=True),
    _l3("odd-src0", BF16, odd=("src0",)),
    _l3("stats", BF16, stats=True),
    _l3("by-name-operands-0", BF16, operands=0, req=_hard(BF16)),
    _l3("C16+48-chunk-spans-the-sources", WINO, C0=16, C1=48),
    _l3("C16+48-hard-refused", None, C0=16, C1=48, req=_hard(BF16)),
    _l3("Cout96", WINO, Cout=96),
    _l3("12x32-no-whole-patches", WINO, Hin=12),
    _l3("8x48-no-whole-patches", WINO, Win=48),
    _l3("no-bf16-image", WINO, image=False),
    _l3("12x32-soft-request-by-name", WINO, Hin=12, req=_soft(BF16)),
    _l3("hard-F2x2-request", WINO, req=_hard(WINO)),
]
