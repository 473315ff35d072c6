"""The multi-chunk rows of the Winograd weight-gradient kernels behind idiff_conv2d_wgrad (wino_wgrad_kernel, F(2x2,3x3), algo 1:
csrc/conv_wino_wgrad.hip; wino4_wgrad_kernel, F(4x4,3x3), algo 3: csrc/conv_wino4_wgrad.hip), shared by the GPU rows of
test_wgrad_wino_gpu.py and their CPU mirror test_wgrad_wino_cpu.py.  Plain data and one pure-Python rule; nothing here imports the
library or torch.

The rule (expected), from the two eligibility functions, the two geometry functions and the kernels' split of the chunk list:
  output size  NORMAL: Hin x Win; UPSAMPLE2: 2Hin x 2Win.  Cin = C0 + C1
  eligibility  both: 3x3, Cout % 64 == 0, Cin % 16 == 0, Wout % 16 == 0, no prologue with a second source, neither of them with upsample
               algo 1: Hout % 2 == 0; two sources need C0 % 64 == 0; dY 8-byte aligned with an even batch stride (float2 loads)
               algo 3: Hout % 4 == 0; two sources need C0 % 32 == 0; dY 16-byte aligned with a batch stride % 4 == 0 (float4 loads)
               algo 3 is tried first, then algo 1, then the direct kernel (algo 0)
  geometry     a workgroup owns 64 co x CIB ci of dW (CIB = 64 for algo 1, 32 for algo 3) and one share of the chunk list; a chunk is one
               row of tiles, TR x 16 output pixels (TR = 2 for algo 1, 4 for algo 3):
               ncob = Cout / 64, ncib = ceil(Cin / CIB), total = B * (Hout / TR) * (Wout / 16)
               nsplit = min(total, max(1, 512 // (ncob * ncib))), per = ceil(total / nsplit); split sp walks chunks [sp * per, sp * per + per)
               cut at total: `used` = ceil(total / per) splits have work, the other `empty` = nsplit - used write a zero partial, the last
               used share has `last_share` = total - (used - 1) * per chunks
  crossings    the positions c - c_begin >= 1 inside a share at which chunk c is the first of a new sample (there the steady state
               reloads the prologue table and the chunk's base pointers move by a batch stride)
  direct       (rows that fall off the ladder) 16-channel chunks, 64-co blocks, tiles of 128 pixels dealt out round-robin:
               nchunks = ceil(Cin / 16), ncob = ceil(Cout / 64), nsplit = min(B * ntiles, max(1, 1536 // (nchunks * ncob)))

  workspace    idiff_conv2d_wgrad_ws_floats = 9 Cin Cout x the LARGEST split count of the forms the shape could get: the direct one, algo 1's
               where Cout % 64 == 0, algo 3's where also Hout % 4 == 0 and Wout % 16 == 0 (ws_splits).  It is an upper bound only: algo 1's
               count is never below algo 3's, so the query says nothing about algo 3's nsplit.  What a launch's nsplit and empty splits
               really were is read by the GPU rows from the NaN-prefilled workspace (which images hold numbers, which are all zero);
               which kernel ran from idiff_conv2d_wgrad_last_algo()

A row's claim is (algo, per, empty, last_share, crossings); a direct row claims (0, 0, 0, 0, ()): its splits are strided, not shares.

Operands: `slc` > 0 makes src0, src1 and dY the channel slices [1, 1 + C) of buffers with `slc` more channels (batch strides above
C H W); `dyoff` moves dY that many floats past a 16-byte boundary; `dc` inputs have mean 3 and spread 0.5; `pro` is the prologue
silu(a x + b) per (sample, channel) with clearly different tables per sample; `acc` accumulates into a prefilled dW; `core` rows are
also called twice for bit-equal results."""

N, U = 0, 1  # IDIFF_CONV_NORMAL, IDIFF_CONV_UPSAMPLE2
DIRECT, WINO, WINO4 = 0, 1, 3  # IDIFF_CONV_ALGO_*
SLICE_LO = 1  # first channel of a sliced operand inside its wider buffer
MAX_B, MAX_CH, MAX_HW = 4, 256, 64 * 96  # the size limits of a row


def _r(name, B, C0, C1, Cout, Hin, Win, claim, **kw):
    row = dict(name=name, B=B, C0=C0, C1=C1, Cout=Cout, Hin=Hin, Win=Win, claim=claim, mode=N, pro=False, acc=False, slc=0, dyoff=0,
               dc=False, core=False)
    assert set(kw) <= set(row), kw
    row.update(kw)
    return row


# claim = (algo, per, empty, last_share, crossings)
ROWS = [
    # ---- the core rows: F(2x2,3x3) ------------------------------------------------------------------------------------------------
    _r("w2-B3-256-256-22x32-per3", 3, 256, 0, 256, 22, 32, (WINO, 3, 10, 3, (1, 2)), core=True),
    _r("w2-B3-256-256-22x16-per2-last1", 3, 256, 0, 256, 22, 16, (WINO, 2, 15, 1, (1,)), core=True),
    _r("w2-B4-64+80-256-22x16-two-src-last-block-16-of-64", 4, 64, 80, 256, 22, 16, (WINO, 2, 20, 2, (1,)), core=True),
    _r("w2-B2-256-256-12x48-dy-8-byte-aligned", 2, 256, 0, 256, 12, 48, (WINO, 2, 14, 2, ()), dyoff=2, core=True),
    # ---- the core rows: F(4x4,3x3) ------------------------------------------------------------------------------------------------
    _r("w4-B3-256-256-44x16-per3", 3, 256, 0, 256, 44, 16, (WINO4, 3, 5, 3, (1, 2)), core=True),
    _r("w4-B2-256-256-12x48-per2", 2, 256, 0, 256, 12, 48, (WINO4, 2, 7, 2, (1,)), core=True),
    _r("w4-B2-256-256-20x80-per4-last2", 2, 256, 0, 256, 20, 80, (WINO4, 4, 3, 2, (1,)), core=True),
    _r("w4-B2-32+48-256-44x64-two-src-C0-32-last1", 2, 32, 48, 256, 44, 64, (WINO4, 3, 12, 1, (2,)), core=True),
    _r("w4-B3-96+48-256-68x16-two-src-ncib5", 3, 96, 48, 256, 68, 16, (WINO4, 3, 8, 3, (1, 2)), core=True),
    # ---- deeper shares: buffer parity over five and seven chunks, crossings at every kind of position --------------------------------
    _r("w2-B4-256-256-22x48-per5", 4, 256, 0, 256, 22, 48, (WINO, 5, 5, 2, (1, 3, 4))),
    _r("w4-B4-256-256-20x80-per7", 4, 256, 0, 256, 20, 80, (WINO4, 7, 1, 2, (1, 4, 5))),
    # ---- prologue on rows with crossings: the table reload in the middle of a share -------------------------------------------------
    _r("w2-B3-256-256-22x32-pro", 3, 256, 0, 256, 22, 32, (WINO, 3, 10, 3, (1, 2)), pro=True),
    _r("w4-B3-256-256-44x16-pro", 3, 256, 0, 256, 44, 16, (WINO4, 3, 5, 3, (1, 2)), pro=True),
    # ---- nearest x2 upsample ----------------------------------------------------------------------------------------------------------
    _r("w2-B3-256-256-up-11x16-to-22x32", 3, 256, 0, 256, 11, 16, (WINO, 3, 10, 3, (1, 2)), mode=U),
    _r("w4-B3-256-256-up-22x8-to-44x16", 3, 256, 0, 256, 22, 8, (WINO4, 3, 5, 3, (1, 2)), mode=U),
    # ---- accumulate into a prefilled dW -----------------------------------------------------------------------------------------------
    _r("w2-B3-256-256-22x16-accumulate", 3, 256, 0, 256, 22, 16, (WINO, 2, 15, 1, (1,)), acc=True),
    _r("w4-B2-256-256-12x48-accumulate", 2, 256, 0, 256, 12, 48, (WINO4, 2, 7, 2, (1,)), acc=True),
    # ---- src0, src1 and dY as channel slices of wider buffers -------------------------------------------------------------------------
    _r("w2-B4-64+80-256-22x16-sliced", 4, 64, 80, 256, 22, 16, (WINO, 2, 20, 2, (1,)), slc=3),
    _r("w4-B2-32+48-256-44x64-sliced", 2, 32, 48, 256, 44, 64, (WINO4, 3, 12, 1, (2,)), slc=3),
    # ---- inputs with a DC offset ------------------------------------------------------------------------------------------------------
    _r("w2-B3-256-256-22x16-dc", 3, 256, 0, 256, 22, 16, (WINO, 2, 15, 1, (1,)), dc=True),
    _r("w4-B2-256-256-12x48-dc", 2, 256, 0, 256, 12, 48, (WINO4, 2, 7, 2, (1,)), dc=True),
    # ---- off the ladder: the direct kernel --------------------------------------------------------------------------------------------
    _r("direct-B2-64-64-12x48-dy-4-byte-aligned", 2, 64, 0, 64, 12, 48, (DIRECT, 0, 0, 0, ()), dyoff=1),
    _r("direct-B2-48+16-64-12x16-two-src-C0-48", 2, 48, 16, 64, 12, 16, (DIRECT, 0, 0, 0, ())),
]

TOL = {WINO: 1e-5, WINO4: 2e-5, DIRECT: 1e-5}  # test_conv_wgrad_winograd_vs_fp64 (F(2x2), F(4x4)); test_conv_wgrad (direct)


def out_size(row):
    return (2 * row["Hin"], 2 * row["Win"]) if row["mode"] == U else (row["Hin"], row["Win"])


def dy_offset_floats(row):
    """distance in floats of dY's first element from the 16-byte-aligned start of its buffer"""
    Hout, Wout = out_size(row)
    return row["dyoff"] + (SLICE_LO * Hout * Wout if row["slc"] else 0)


def dy_bstride(row):
    Hout, Wout = out_size(row)
    return (row["Cout"] + row["slc"]) * Hout * Wout


def eligible(row, algo):
    """the eligibility functions of the two kernels (wino_wgrad_eligible, wino4_wgrad_eligible), restated"""
    Hout, Wout = out_size(row)
    Cin = row["C0"] + row["C1"]
    tr, cib, align = (2, 64, 2) if algo == WINO else (4, 32, 4)  # tile rows, channels per block, dY alignment in floats
    if row["Cout"] % 64 or Cin % 16 or Hout % tr or Wout % 16:
        return False
    if row["C1"] and row["C0"] % cib:
        return False
    if row["mode"] == U and (row["pro"] or row["C1"]):
        return False
    if row["pro"] and row["C1"]:
        return False
    return dy_offset_floats(row) % align == 0 and dy_bstride(row) % align == 0


def pick_algo(row):
    return WINO4 if eligible(row, WINO4) else (WINO if eligible(row, WINO) else DIRECT)


def geometry(row, algo=None):
    """dict of everything the rule says about the grid and the shares of the row on `algo` (default: the one the ladder picks)"""
    algo = pick_algo(row) if algo is None else algo
    B, Cout, Cin = row["B"], row["Cout"], row["C0"] + row["C1"]
    Hout, Wout = out_size(row)
    if algo == DIRECT:
        twl = 5 if Wout >= 32 else (4 if Wout >= 16 else 3)
        TW = 1 << twl
        TH = 128 // TW
        ntiles = -(-Wout // TW) * -(-Hout // TH)
        ck = 8 if Cin <= 8 else 16
        nchunks, ncob = -(-Cin // ck), -(-Cout // 64)
        nsplit = min(B * ntiles, max(1, 1536 // (nchunks * ncob)))
        return dict(algo=algo, ncob=ncob, ncib=nchunks, cib=ck, total=B * ntiles, nsplit=nsplit, per=0, used=nsplit, empty=0, last_share=0,
                    crossings=())
    tr, cib = (2, 64) if algo == WINO else (4, 32)
    ncob, ncib = Cout // 64, -(-Cin // cib)
    per_sample = (Hout // tr) * (Wout // 16)
    total = B * per_sample
    nsplit = min(total, max(1, 512 // (ncob * ncib)))
    per = -(-total // nsplit)
    used = -(-total // per)
    crossings = tuple(sorted({(b * per_sample) % per for b in range(1, B)} - {0}))
    return dict(algo=algo, ncob=ncob, ncib=ncib, cib=cib, total=total, nsplit=nsplit, per=per, used=used, empty=nsplit - used,
                last_share=total - (used - 1) * per, crossings=crossings)


def ws_splits(row):
    """idiff_conv2d_wgrad_ws_floats / (9 Cin Cout): the largest split count over the forms the shape could get, whatever dY's alignment
    (an upper bound of the launched form's nsplit, not a witness of it)"""
    Hout, Wout = out_size(row)
    n = geometry(row, DIRECT)["nsplit"]
    if row["Cout"] % 64 == 0:
        n = max(n, geometry(row, WINO)["nsplit"])
        if Hout % 4 == 0 and Wout % 16 == 0:
            n = max(n, geometry(row, WINO4)["nsplit"])
    return n


def expected(row):
    """(algo, per, empty, last_share, crossings): the claim the rule derives for a row"""
    g = geometry(row)
    return (g["algo"], g["per"], g["empty"], g["last_share"], g["crossings"])
