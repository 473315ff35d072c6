"""The launch-branch table of the direct implicit-GEMM convolution (conv_igemm_kernel<KS, CK, TWL, MODE, VECW, MB, SPEC> behind
idiff_conv2d_fwd, csrc/conv_igemm.hip), shared by the GPU rows of test_conv_branches_gpu.py and their CPU mirror
test_conv_branches_cpu.py.  Plain data and one pure-Python rule; nothing here imports the library.

The rule (expected_branch), from include/idiff.h and the launcher's comments:
  output size  NORMAL: Hin x Win; UPSAMPLE2: 2Hin x 2Win; UNSHUFFLE2: Hin/2 x Win/2 with 4*C0 virtual input channels
  TWL          pixel tile = 2^TWL columns x 256 / 2^TWL rows: 5 (8x32) from 24 output columns up, 4 (16x16) from 16, else 3 (32x8)
  MB           32 * MB output channels per workgroup: 1 up to Cout = 32, else 2
  VECW         16-byte weight loads: Cout % 4 == 0 and a 16-byte-aligned weight image
  flattened    a 1x1 NORMAL layer without statistics, MB = 2, VECW, 16-byte-aligned sources and batch strides, Hout*Wout % 256 == 0
               and Wout >= 32 runs on 256 consecutive pixels per tile: TWL = 8
  SPEC         only the flattened tile and (3x3, NORMAL, TWL 5, MB 2, VECW) are specialised: 2 = prologue, 3 = two sources,
               1 = neither; every other instantiation is the generic 0
CK (input channels per chunk) follows KS: 8 for 3x3, 16 for 1x1, 2 for 7x7, so it is not part of the tuple.

A row's operands: `slices` maps an operand to the number of extra channels of the wider buffer it is the channel slice [1 : 1 + C]
of (batch stride above the dense one); `odd` lists operands that start one float past a 16-byte boundary; `dc` inputs carry a DC
offset (mean 3, spread 0.5); `gn` = groups: the statistics (and the finalize outputs) are placed inside larger sentinel buffers."""
import itertools

N, U, S = 0, 1, 2  # IDIFF_CONV_NORMAL, IDIFF_CONV_UPSAMPLE2, IDIFF_CONV_UNSHUFFLE2
MODE_NAME = {N: "normal", U: "up2", S: "unshuffle2"}
SLICE_LO = 1  # first channel of a sliced operand inside its wider buffer


def _r(name, ks, mode, B, C0, C1, Cout, Hin, Win, claim, **kw):
    row = dict(name=name, ks=ks, mode=mode, B=B, C0=C0, C1=C1, Cout=Cout, Hin=Hin, Win=Win, claim=claim, pro=False, res=False, vec=False,
               aux=False, bias=True, stats=False, gn=0, slices={}, odd=(), dc=False)
    assert set(kw) <= set(row), kw
    row.update(kw)
    if row["gn"]:
        row["stats"] = True
    return row


# claim = (KS, MODE, TWL, VECW, MB, SPEC)
ROWS = [
    # ---- 3x3 normal ------------------------------------------------------------------------------------------------------------
    _r("c3n-t3-v1-m1-stats-ragged-halfwaves", 3, N, 2, 24, 0, 32, 12, 12, (3, N, 3, 1, 1, 0), stats=True),
    _r("c3n-t3-v0-m1-Cout5-ragged-W9", 3, N, 1, 8, 0, 5, 40, 9, (3, N, 3, 0, 1, 0), res=True),
    _r("c3n-t4-v1-m1-two-src-stats-dc", 3, N, 2, 16, 8, 20, 20, 20, (3, N, 4, 1, 1, 0), stats=True, dc=True),
    _r("c3n-t4-v0-m1-Cout30-pro-W23", 3, N, 2, 12, 0, 30, 16, 23, (3, N, 4, 0, 1, 0), pro=True),
    _r("c3n-t5-v1-m1-Cout8-aux-out-slice", 3, N, 2, 40, 0, 8, 9, 33, (3, N, 5, 1, 1, 0), aux=True, slices={"out": 3}),
    _r("c3n-t5-v0-m1-Cout17-two-src-stats-W24", 3, N, 2, 8, 8, 17, 32, 24, (3, N, 5, 0, 1, 0), stats=True),
    _r("c3n-t3-v1-m2-Cout96-res-slice-stats", 3, N, 2, 16, 0, 96, 8, 8, (3, N, 3, 1, 2, 0), res=True, stats=True, slices={"res": 5}),
    _r("c3n-t3-v0-m2-Cout66-vec-ragged", 3, N, 1, 8, 0, 66, 33, 15, (3, N, 3, 0, 2, 0), vec=True),
    _r("c3n-t4-v1-m2-pro-gn-guard", 3, N, 2, 32, 0, 64, 16, 16, (3, N, 4, 1, 2, 0), pro=True, gn=8),
    _r("c3n-t4-v0-m2-odd-wpk-src1-slice", 3, N, 2, 16, 16, 64, 17, 19, (3, N, 4, 0, 2, 0), slices={"src1": 4}, odd=("wpk",)),
    _r("c3n-t5-v0-m2-Cout70-res-aux-dc", 3, N, 2, 24, 0, 70, 10, 40, (3, N, 5, 0, 2, 0), res=True, aux=True, dc=True),
    _r("c3n-t5-v1-m2-spec1-Cout96-C20-stats-out-slice", 3, N, 2, 20, 0, 96, 12, 36, (3, N, 5, 1, 2, 1), stats=True, slices={"out": 2}),
    _r("c3n-t5-v1-m2-spec2-pro-res-dc", 3, N, 2, 32, 0, 64, 16, 32, (3, N, 5, 1, 2, 2), pro=True, res=True, dc=True),
    _r("c3n-t5-v1-m2-spec3-two-src-C12-aux-slices", 3, N, 2, 12, 20, 128, 8, 48, (3, N, 5, 1, 2, 3), aux=True,
       slices={"aux": 6, "src0": 3}),
    # ---- 3x3 upsample x2 (Winograd refuses two sources and prologues here: these always land on the direct kernel) ---------------
    _r("c3u-t3-v1-m1-pro-odd-5x3", 3, U, 2, 8, 0, 16, 5, 3, (3, U, 3, 1, 1, 0), pro=True),
    _r("c3u-t3-v0-m1-Cout6-two-src", 3, U, 2, 6, 4, 6, 4, 7, (3, U, 3, 0, 1, 0)),
    _r("c3u-t4-v1-m1-stats-dc-9x9", 3, U, 2, 16, 0, 32, 9, 9, (3, U, 4, 1, 1, 0), stats=True, dc=True),
    _r("c3u-t4-v0-m1-Cout31-res", 3, U, 1, 8, 0, 31, 8, 11, (3, U, 4, 0, 1, 0), res=True),
    _r("c3u-t5-v1-m1-Cout24-aux-6x13", 3, U, 2, 16, 0, 24, 6, 13, (3, U, 5, 1, 1, 0), aux=True),
    _r("c3u-t5-v0-m1-Cout7-vec", 3, U, 2, 8, 0, 7, 4, 16, (3, U, 5, 0, 1, 0), vec=True),
    _r("c3u-t3-v1-m2-two-src-out-slice-7x5", 3, U, 2, 12, 12, 64, 7, 5, (3, U, 3, 1, 2, 0), slices={"out": 4}),
    _r("c3u-t3-v0-m2-Cout34-stats", 3, U, 2, 8, 0, 34, 3, 6, (3, U, 3, 0, 2, 0), stats=True),
    _r("c3u-t4-v1-m2-Cout80-pro-src0-slice", 3, U, 2, 16, 0, 80, 8, 8, (3, U, 4, 1, 2, 0), pro=True, slices={"src0": 2}),
    _r("c3u-t4-v0-m2-odd-wpk-5x10", 3, U, 1, 8, 0, 64, 5, 10, (3, U, 4, 0, 2, 0), odd=("wpk",)),
    _r("c3u-t5-v1-m2-two-src-src1-slice-res-stats", 3, U, 2, 32, 16, 64, 12, 16, (3, U, 5, 1, 2, 0), res=True, stats=True,
       slices={"src1": 8}),
    _r("c3u-t5-v0-m2-Cout65-pro-dc-5x15", 3, U, 2, 8, 0, 65, 5, 15, (3, U, 5, 0, 2, 0), pro=True, dc=True),
    # ---- 1x1 normal -------------------------------------------------------------------------------------------------------------
    _r("c1n-t3-v1-m1-C40-stats", 1, N, 2, 40, 0, 32, 10, 10, (1, N, 3, 1, 1, 0), stats=True),
    _r("c1n-t3-v0-m1-Cout3-pro", 1, N, 2, 16, 0, 3, 7, 15, (1, N, 3, 0, 1, 0), pro=True),
    _r("c1n-t4-v1-m1-two-src-res-slice", 1, N, 2, 20, 12, 12, 16, 16, (1, N, 4, 1, 1, 0), res=True, slices={"res": 4}),
    _r("c1n-t4-v0-m1-Cout29-aux-dc", 1, N, 2, 32, 0, 29, 5, 22, (1, N, 4, 0, 1, 0), aux=True, dc=True),
    _r("c1n-t5-v1-m1-Cout4-out-slice-no-flatten-mb1", 1, N, 2, 64, 0, 4, 8, 32, (1, N, 5, 1, 1, 0), slices={"out": 4}),
    _r("c1n-t5-v0-m1-Cout31-C17-stats", 1, N, 2, 17, 0, 31, 9, 25, (1, N, 5, 0, 1, 0), stats=True),
    _r("c1n-t3-v1-m2-vec", 1, N, 2, 48, 0, 64, 16, 8, (1, N, 3, 1, 2, 0), vec=True),
    _r("c1n-t3-v0-m2-Cout33-stats", 1, N, 2, 16, 0, 33, 12, 12, (1, N, 3, 0, 2, 0), stats=True),
    _r("c1n-t4-v1-m2-pro-no-flatten-W16", 1, N, 2, 32, 0, 128, 16, 16, (1, N, 4, 1, 2, 0), pro=True),
    _r("c1n-t4-v0-m2-odd-wpk-two-src", 1, N, 2, 16, 16, 72, 8, 20, (1, N, 4, 0, 2, 0), odd=("wpk",)),
    _r("c1n-t5-v1-m2-no-flatten-stats-gn-guard", 1, N, 2, 64, 0, 64, 8, 32, (1, N, 5, 1, 2, 0), gn=8),
    _r("c1n-t5-v1-m2-no-flatten-HW288-res", 1, N, 2, 32, 0, 96, 9, 32, (1, N, 5, 1, 2, 0), res=True),
    _r("c1n-t5-v1-m2-no-flatten-W24-aux", 1, N, 1, 32, 0, 64, 32, 24, (1, N, 5, 1, 2, 0), aux=True),
    _r("c1n-t5-v1-m2-no-flatten-odd-src0", 1, N, 2, 32, 0, 64, 8, 32, (1, N, 5, 1, 2, 0), odd=("src0",)),
    _r("c1n-t5-v0-m2-Cout66", 1, N, 2, 32, 0, 66, 8, 32, (1, N, 5, 0, 2, 0)),
    _r("c1n-flat-spec1-Cout96-C40-res-only", 1, N, 2, 40, 0, 96, 8, 32, (1, N, 8, 1, 2, 1), res=True),
    _r("c1n-flat-spec1-aux-only-out-slice", 1, N, 2, 16, 0, 64, 16, 32, (1, N, 8, 1, 2, 1), aux=True, slices={"out": 3}),
    _r("c1n-flat-spec1-product-256-256-64x64-res-aux", 1, N, 1, 256, 0, 256, 64, 64, (1, N, 8, 1, 2, 1), res=True, aux=True),
    _r("c1n-flat-spec1-plain-vec", 1, N, 2, 32, 0, 64, 8, 64, (1, N, 8, 1, 2, 1), vec=True),
    _r("c1n-flat-spec2-pro-C24-res-aux-dc", 1, N, 2, 24, 0, 128, 16, 32, (1, N, 8, 1, 2, 2), pro=True, res=True, aux=True, dc=True),
    _r("c1n-flat-spec3-two-src-src1-slice-Cout96-res", 1, N, 2, 24, 40, 96, 8, 96, (1, N, 8, 1, 2, 3), res=True, slices={"src1": 8}),
    # ---- 1x1 pixel-unshuffle ----------------------------------------------------------------------------------------------------
    _r("c1s-t3-v1-m1-C6-pro", 1, S, 2, 6, 0, 32, 16, 16, (1, S, 3, 1, 1, 0), pro=True),
    _r("c1s-t3-v0-m1-Cout9-odd-src0-no-pair-gather", 1, S, 2, 4, 0, 9, 10, 30, (1, S, 3, 0, 1, 0), odd=("src0",)),
    _r("c1s-t4-v1-m1-stats", 1, S, 2, 8, 0, 16, 24, 32, (1, S, 4, 1, 1, 0), stats=True),
    _r("c1s-t4-v0-m1-Cout27-C5-dc", 1, S, 2, 5, 0, 27, 8, 44, (1, S, 4, 0, 1, 0), dc=True),
    _r("c1s-t5-v1-m1-Cout28-res", 1, S, 2, 8, 0, 28, 12, 48, (1, S, 5, 1, 1, 0), res=True),
    _r("c1s-t5-v0-m1-Cout10-C3-pro-odd-src0", 1, S, 2, 3, 0, 10, 18, 66, (1, S, 5, 0, 1, 0), pro=True, odd=("src0",)),
    _r("c1s-t3-v1-m2-aux", 1, S, 2, 16, 0, 64, 16, 16, (1, S, 3, 1, 2, 0), aux=True),
    _r("c1s-t3-v0-m2-Cout35", 1, S, 2, 4, 0, 35, 6, 28, (1, S, 3, 0, 2, 0)),
    _r("c1s-t4-v1-m2-Cout96-src0-slice-out-slice", 1, S, 2, 12, 0, 96, 32, 32, (1, S, 4, 1, 2, 0), slices={"src0": 3, "out": 2}),
    _r("c1s-t4-v0-m2-odd-wpk-stats", 1, S, 2, 8, 0, 64, 14, 36, (1, S, 4, 0, 2, 0), stats=True, odd=("wpk",)),
    _r("c1s-t5-v1-m2-pro-dc-vec", 1, S, 2, 16, 0, 64, 16, 64, (1, S, 5, 1, 2, 0), pro=True, dc=True, vec=True),
    _r("c1s-t5-v0-m2-Cout37-res-W25", 1, S, 2, 8, 0, 37, 20, 50, (1, S, 5, 0, 2, 0), res=True),
    # ---- 7x7 normal -------------------------------------------------------------------------------------------------------------
    _r("c7n-t3-v1-m1-C3-stats", 7, N, 2, 3, 0, 32, 12, 12, (7, N, 3, 1, 1, 0), stats=True),
    _r("c7n-t3-v0-m1-Cout3-pro", 7, N, 2, 2, 0, 3, 9, 15, (7, N, 3, 0, 1, 0), pro=True),
    _r("c7n-t4-v1-m1-C1-res", 7, N, 2, 1, 0, 8, 16, 16, (7, N, 4, 1, 1, 0), res=True),
    _r("c7n-t4-v0-m1-Cout30-C3-dc", 7, N, 2, 3, 0, 30, 7, 23, (7, N, 4, 0, 1, 0), dc=True),
    _r("c7n-t5-v1-m1-two-src-aux", 7, N, 2, 2, 1, 16, 10, 40, (7, N, 5, 1, 1, 0), aux=True),
    _r("c7n-t5-v0-m1-Cout6", 7, N, 2, 4, 0, 6, 8, 24, (7, N, 5, 0, 1, 0)),
    _r("c7n-t3-v1-m2-C3-vec-out-slice", 7, N, 2, 3, 0, 64, 33, 8, (7, N, 3, 1, 2, 0), vec=True, slices={"out": 2}),
    _r("c7n-t3-v0-m2-Cout34", 7, N, 2, 2, 0, 34, 8, 13, (7, N, 3, 0, 2, 0)),
    _r("c7n-t4-v1-m2-Cout96-C3-pro-stats-res", 7, N, 2, 3, 0, 96, 20, 20, (7, N, 4, 1, 2, 0), pro=True, stats=True, res=True),
    _r("c7n-t4-v0-m2-odd-wpk", 7, N, 2, 2, 0, 64, 16, 17, (7, N, 4, 0, 2, 0), odd=("wpk",)),
    _r("c7n-t5-v1-m2-product-224x224-C2-stats", 7, N, 1, 2, 0, 64, 224, 224, (7, N, 5, 1, 2, 0), stats=True),
    _r("c7n-t5-v0-m2-Cout65-C3-aux-src0-slice", 7, N, 2, 3, 0, 65, 9, 30, (7, N, 5, 0, 2, 0), aux=True, slices={"src0": 2}),
]

# tuples of REACHABLE that no row claims, each with its reason (at most 3 allowed; none needed)
LEFT_OUT = {}


def _reachable():
    out = set()
    for ks, mode in ((3, N), (3, U), (1, N), (1, S), (7, N)):
        for mb, twl, vecw in itertools.product((1, 2), (3, 4, 5), (0, 1)):
            if (ks, mode, mb, twl, vecw) == (3, N, 2, 5, 1):
                out |= {(ks, mode, twl, vecw, mb, spec) for spec in (1, 2, 3)}
            else:
                out.add((ks, mode, twl, vecw, mb, 0))
    out |= {(1, N, 8, 1, 2, spec) for spec in (1, 2, 3)}
    return out


REACHABLE = _reachable()  # 14 + 12 + 15 + 12 + 12 = 65


def out_size(row):
    if row["mode"] == U:
        return row["Hin"] * 2, row["Win"] * 2
    if row["mode"] == S:
        return row["Hin"] // 2, row["Win"] // 2
    return row["Hin"], row["Win"]


def pick_twl(Wout):
    return 5 if Wout >= 24 else (4 if Wout >= 16 else 3)


def tile_shape(twl):
    """(TH, TW) of a pixel tile"""
    return 256 >> twl, 1 << twl


def _float_offset(row, name, plane):
    """distance in floats of an operand's first element from the 16-byte-aligned start of its buffer"""
    return (SLICE_LO * plane if name in row["slices"] else 0) + (1 if name in row["odd"] else 0)


def batch_stride(row, name, C, plane):
    return (C + row["slices"].get(name, 0)) * plane


def expected_branch(row):
    """(KS, MODE, TWL, VECW, MB, SPEC) of the instantiation idiff_conv2d_fwd launches for this row when asked for the direct kernel"""
    ks, mode = row["ks"], row["mode"]
    Hout, Wout = out_size(row)
    twl = pick_twl(Wout)
    mb = 1 if row["Cout"] <= 32 else 2
    vecw = row["Cout"] % 4 == 0 and "wpk" not in row["odd"]
    plane = row["Hin"] * row["Win"]
    in16 = _float_offset(row, "src0", plane) % 4 == 0 and batch_stride(row, "src0", row["C0"], plane) % 4 == 0
    if row["C1"]:
        in16 = in16 and _float_offset(row, "src1", plane) % 4 == 0 and batch_stride(row, "src1", row["C1"], plane) % 4 == 0
    if ks == 1 and mode == N and not row["stats"] and mb == 2 and vecw and in16 and (Hout * Wout) % 256 == 0 and Wout >= 32:
        twl = 8
    special = twl == 8 or (twl == 5 and ks == 3 and mode == N and mb == 2 and vecw)
    spec = (2 if row["pro"] else 3 if row["C1"] else 1) if special else 0
    return (ks, mode, twl, int(vecw), mb, spec)


def kernel_name(t):
    """the instantiation as the demangled kernel name of a trace spells its template arguments"""
    ck = {3: 8, 1: 16, 7: 2}[t[0]]
    return "conv_igemm_kernel<%d, %d, %d, %d, %s, %d, %d>" % (t[0], ck, t[2], t[1], "true" if t[3] else "false", t[4], t[5])
