"""The launch-branch table of the three Winograd forward kernels behind idiff_conv2d_fwd -- conv_wino_kernel<MODE, SPEC, RAG>
(csrc/conv_wino.hip, F(2x2,3x3), 8x32-pixel items), conv_wino4_kernel<MODE, SPEC, RAG> (csrc/conv_wino4.hip, F(4x4,3x3), 16x32-pixel
items) and conv_wino4h_kernel<MODE, SPEC, RAG> (csrc/conv_wino4h.hip, F(4x4,3x3), 8x32-pixel half-patch items) -- shared by the GPU rows
of test_wino_fwd_gpu.py and their CPU mirror test_wino_fwd_cpu.py.  Plain data and pure Python; nothing here imports the library.

A row has the shape of a row of conv_branch_rows.py (ks = 3 throughout) plus `kernel`, so conv_branch_ref.make_inputs / reference /
tile_stats serve it unchanged.  claim = (kernel, MODE, SPEC, RAG).

The rules, from csrc/wino_common.h (launch_spec_ladder, persistent_grid), the three launch_conv_wino* and the eligibility checks
conv_wino_eligible / conv_wino4_items (+ the Cin >= 16 of the 16x32 kernel in idiff_conv2d_fwd):
  MODE    NORMAL or UPSAMPLE2 (output 2Hin x 2Win)
  SPEC    2 with a prologue, 3 with a second source, else 1; upsample is always 1 (neither is eligible there)
  RAG     Hout % TH or Wout % TW, TH x TW = 8x32 (WINO, WINO4H) or 16x32 (WINO4)
  items   per sample ceil(Wout/32) * ceil(Hout/TH) * ceil(Cout/64); a launch has total = B * items of them, walked by
          grid = ceil(total / per) persistent workgroups, per = ceil(total / slots), slots = CUs (2 * CUs for WINO4H); workgroup wg
          takes items wg, wg + grid, wg + 2 grid, ...; an item index counts channel block fastest, then patch column, patch row, sample

Item-stream rows (`stream`) have no B of their own: it is derived from the device's CU count (stream_facts) so that a workgroup walks
`per` items.  A total that is a multiple of per = 4 is no use there: the grid is then a multiple of the 27 items of a sample and the
item counter never carries."""
from conv_branch_rows import N, SLICE_LO, U, _float_offset, batch_stride, out_size  # noqa: F401

WINO, WINO4, WINO4H = 1, 3, 4  # IDIFF_CONV_ALGO_WINOGRAD, _WINOGRAD4, _WINOGRAD4H
KERNELS = (WINO, WINO4, WINO4H)
KERNEL_NAME = {WINO: "conv_wino_kernel", WINO4: "conv_wino4_kernel", WINO4H: "conv_wino4h_kernel"}
PATCH = {WINO: (8, 32), WINO4: (16, 32), WINO4H: (8, 32)}  # TH, TW
MIRROR_CUS = 256  # the CU count the CPU mirror checks the item-stream rows at (an MI355X)


def _r(name, kernel, mode, C0, C1, Cout, Hin, Win, claim, B=2, **kw):
    row = dict(name=name, kernel=kernel, ks=3, mode=mode, B=B, C0=C0, C1=C1, Cout=Cout, Hin=Hin, Win=Win, claim=(kernel,) + claim, pro=False,
               res=False, vec=False, aux=False, bias=True, stats=False, gn=0, slices={}, odd=(), dc=False, stream=None)
    assert set(kw) <= set(row), kw
    row.update(kw)
    if row["gn"]:
        row["stats"] = True
    return row


def _s(name, kernel, C0, C1, Cout, H, W, claim, per, short=False, **kw):
    return _r(name, kernel, N, C0, C1, Cout, H, W, claim, B=None, stream=dict(per=per, short=short), **kw)


ALL = dict(res=True, vec=True, aux=True, stats=True)  # every epilogue term at once (with the bias)

# claim = (MODE, SPEC, RAG); the kernel is prepended
ROWS = [
    # ---- conv_wino_kernel: F(2x2,3x3), 8x32 items, chunks of 8 input channels ----------------------------------------------------------
    _r("w2-n1-24x96-C8-one-chunk-Cout144-out-slice", WINO, N, 8, 0, 144, 24, 96, (N, 1, 0), slices={"out": 4}),
    _r("w2-n1-24x96-C16-Cout64-no-bias-odd-src0", WINO, N, 16, 0, 64, 24, 96, (N, 1, 0), bias=False, odd=("src0",)),
    _r("w2-n1-24x96-C16-Cout128-dc-stats", WINO, N, 16, 0, 128, 24, 96, (N, 1, 0), dc=True, stats=True),
    _r("w2-n1-12x40-C24-Cout48-res-src0-slice", WINO, N, 24, 0, 48, 12, 40, (N, 1, 1), res=True, slices={"src0": 4}),
    _r("w2-n1-10x24-C40-Cout16-vec", WINO, N, 40, 0, 16, 10, 24, (N, 1, 1), vec=True),
    _r("w2-n1-12x28-C8-Cout80-aux-slice", WINO, N, 8, 0, 80, 12, 28, (N, 1, 1), aux=True, slices={"aux": 4}),
    _r("w2-n2-24x96-C16-Cout64-pro-dc-gn", WINO, N, 16, 0, 64, 24, 96, (N, 2, 0), pro=True, dc=True, gn=8),
    _r("w2-n2-12x40-C24-Cout80-pro-stats-res-slice", WINO, N, 24, 0, 80, 12, 40, (N, 2, 1), pro=True, stats=True, res=True,
       slices={"res": 4}),
    _r("w2-n2-12x28-C8-Cout16-pro-narrow", WINO, N, 8, 0, 16, 12, 28, (N, 2, 1), pro=True),
    _r("w2-n3-24x96-C8+16-Cout128-all-src1-slice-gn", WINO, N, 8, 16, 128, 24, 96, (N, 3, 0), gn=4, slices={"src1": 4}, **ALL),
    _r("w2-n3-10x24-C16+8-Cout48-stats", WINO, N, 16, 8, 48, 10, 24, (N, 3, 1), stats=True),
    _r("w2-u1-12x48-C16-Cout64-res-slice", WINO, U, 16, 0, 64, 12, 48, (U, 1, 0), res=True, slices={"res": 8}),
    _r("w2-u1-6x14-C8-Cout144-stats", WINO, U, 8, 0, 144, 6, 14, (U, 1, 1), stats=True),
    # ---- conv_wino4_kernel: F(4x4,3x3), 16x32 items, chunks of 4 input channels, at least four of them ------------------------------------
    _r("w4-n1-48x96-C16-four-chunks-Cout144-out-slice", WINO4, N, 16, 0, 144, 48, 96, (N, 1, 0), slices={"out": 4}),
    _r("w4-n1-48x96-C16-Cout128-dc-stats", WINO4, N, 16, 0, 128, 48, 96, (N, 1, 0), dc=True, stats=True),
    _r("w4-n1-8x24-C16-Cout16-vec-lower-half-outside", WINO4, N, 16, 0, 16, 8, 24, (N, 1, 1), vec=True),
    _r("w4-n1-24x36-C24-Cout48-res-stats-src0-slice", WINO4, N, 24, 0, 48, 24, 36, (N, 1, 1), res=True, stats=True, slices={"src0": 4}),
    _r("w4-n1-20x44-C16-Cout80-aux-slice-upper-half-partial", WINO4, N, 16, 0, 80, 20, 44, (N, 1, 1), aux=True, slices={"aux": 4}),
    _r("w4-n1-28x96-C32-Cout64-no-bias-odd-src0-lower-half-partial", WINO4, N, 32, 0, 64, 28, 96, (N, 1, 1), bias=False, odd=("src0",)),
    _r("w4-n2-48x96-C16-Cout64-pro-dc-gn", WINO4, N, 16, 0, 64, 48, 96, (N, 2, 0), pro=True, dc=True, gn=8),
    _r("w4-n2-24x36-C24-Cout80-pro-stats-res-slice", WINO4, N, 24, 0, 80, 24, 36, (N, 2, 1), pro=True, stats=True, res=True,
       slices={"res": 4}),
    _r("w4-n2-20x24-C16-Cout48-pro-narrow", WINO4, N, 16, 0, 48, 20, 24, (N, 2, 1), pro=True),
    _r("w4-n3-48x96-C12+20-Cout128-all-src1-slice-gn", WINO4, N, 12, 20, 128, 48, 96, (N, 3, 0), gn=4, slices={"src1": 4}, **ALL),
    _r("w4-n3-28x44-C12+4-Cout48-stats", WINO4, N, 12, 4, 48, 28, 44, (N, 3, 1), stats=True),
    _r("w4-u1-24x48-C16-Cout64-res-slice", WINO4, U, 16, 0, 64, 24, 48, (U, 1, 0), res=True, slices={"res": 8}),
    _r("w4-u1-6x14-C16-Cout144-stats", WINO4, U, 16, 0, 144, 6, 14, (U, 1, 1), stats=True),
    # ---- conv_wino4h_kernel: F(4x4,3x3), 8x32 half-patch items, chunks of 4 input channels, an even number of them ------------------------
    _r("w4h-n1-24x96-C8-two-chunks-Cout144-out-slice", WINO4H, N, 8, 0, 144, 24, 96, (N, 1, 0), slices={"out": 4}),
    _r("w4h-n1-24x96-C16-Cout64-no-bias-odd-src0", WINO4H, N, 16, 0, 64, 24, 96, (N, 1, 0), bias=False, odd=("src0",)),
    _r("w4h-n1-24x96-C16-Cout128-dc-stats", WINO4H, N, 16, 0, 128, 24, 96, (N, 1, 0), dc=True, stats=True),
    _r("w4h-n1-12x40-C24-Cout48-res-src0-slice", WINO4H, N, 24, 0, 48, 12, 40, (N, 1, 1), res=True, slices={"src0": 4}),
    _r("w4h-n1-12x28-C40-Cout16-vec", WINO4H, N, 40, 0, 16, 12, 28, (N, 1, 1), vec=True),
    _r("w4h-n1-12x28-C8-Cout80-aux-slice", WINO4H, N, 8, 0, 80, 12, 28, (N, 1, 1), aux=True, slices={"aux": 4}),
    _r("w4h-n2-24x96-C16-Cout64-pro-dc-gn", WINO4H, N, 16, 0, 64, 24, 96, (N, 2, 0), pro=True, dc=True, gn=8),
    _r("w4h-n2-12x40-C24-Cout80-pro-stats-res-slice", WINO4H, N, 24, 0, 80, 12, 40, (N, 2, 1), pro=True, stats=True, res=True,
       slices={"res": 4}),
    _r("w4h-n2-12x28-C8-Cout16-pro-narrow", WINO4H, N, 8, 0, 16, 12, 28, (N, 2, 1), pro=True),
    _r("w4h-n3-24x96-C12+20-Cout128-all-src1-slice-gn", WINO4H, N, 12, 20, 128, 24, 96, (N, 3, 0), gn=4, slices={"src1": 4}, **ALL),
    _r("w4h-n3-12x40-C4+4-Cout48-stats", WINO4H, N, 4, 4, 48, 12, 40, (N, 3, 1), stats=True),
    _r("w4h-u1-12x48-C16-Cout64-res-slice", WINO4H, U, 16, 0, 64, 12, 48, (U, 1, 0), res=True, slices={"res": 8}),
    _r("w4h-u1-6x14-C8-Cout144-stats", WINO4H, U, 8, 0, 144, 6, 14, (U, 1, 1), stats=True),
]

# ---- item-stream rows: 27 items per sample (3 channel blocks x 3 patch columns x 3 patch rows), B from the CU count ------------------
EPI = dict(res=True, vec=True, stats=True)
ROWS += [
    _s("w2-stream-per4-plain", WINO, 8, 0, 144, 24, 96, (N, 1, 0), 4),
    _s("w2-stream-per4-pro", WINO, 8, 0, 144, 24, 96, (N, 2, 0), 4, pro=True),
    _s("w2-stream-per4-two-src", WINO, 8, 8, 144, 24, 96, (N, 3, 0), 4),
    _s("w2-stream-per4-epilogue-stats", WINO, 8, 0, 144, 24, 96, (N, 1, 0), 4, **EPI),
    _s("w2-stream-per4-short-last-workgroup-plain", WINO, 8, 0, 144, 24, 96, (N, 1, 0), 4, short=True),
    _s("w2-stream-per4-short-last-workgroup-pro-stats", WINO, 8, 0, 144, 24, 96, (N, 2, 0), 4, short=True, pro=True, stats=True),
    _s("w2-stream-per2-20x44-plain", WINO, 8, 0, 144, 20, 44, (N, 1, 1), 2),
    _s("w2-stream-per2-20x44-pro", WINO, 8, 0, 144, 20, 44, (N, 2, 1), 2, pro=True),
    _s("w2-stream-per2-20x44-two-src", WINO, 8, 8, 144, 20, 44, (N, 3, 1), 2),
    _s("w2-stream-per2-20x44-epilogue-stats", WINO, 8, 0, 144, 20, 44, (N, 1, 1), 2, **EPI),
    _s("w4-stream-per4-plain", WINO4, 16, 0, 144, 48, 96, (N, 1, 0), 4),
    _s("w4-stream-per4-pro", WINO4, 16, 0, 144, 48, 96, (N, 2, 0), 4, pro=True),
    _s("w4-stream-per4-two-src", WINO4, 4, 12, 144, 48, 96, (N, 3, 0), 4),
    _s("w4-stream-per4-epilogue-stats", WINO4, 16, 0, 144, 48, 96, (N, 1, 0), 4, **EPI),
    _s("w4-stream-per4-short-last-workgroup-plain", WINO4, 16, 0, 144, 48, 96, (N, 1, 0), 4, short=True),
    _s("w4-stream-per4-short-last-workgroup-pro-stats", WINO4, 16, 0, 144, 48, 96, (N, 2, 0), 4, short=True, pro=True, stats=True),
    _s("w4-stream-per2-20x44-plain", WINO4, 16, 0, 144, 20, 44, (N, 1, 1), 2),
    _s("w4-stream-per2-20x44-pro", WINO4, 16, 0, 144, 20, 44, (N, 2, 1), 2, pro=True),
    _s("w4-stream-per2-20x44-two-src", WINO4, 4, 12, 144, 20, 44, (N, 3, 1), 2),
    _s("w4-stream-per2-20x44-epilogue-stats", WINO4, 16, 0, 144, 20, 44, (N, 1, 1), 2, **EPI),
    _s("w4h-stream-per4-plain", WINO4H, 8, 0, 144, 24, 96, (N, 1, 0), 4),
    _s("w4h-stream-per4-pro", WINO4H, 8, 0, 144, 24, 96, (N, 2, 0), 4, pro=True),
    _s("w4h-stream-per4-two-src", WINO4H, 4, 4, 144, 24, 96, (N, 3, 0), 4),
    _s("w4h-stream-per4-epilogue-stats", WINO4H, 8, 0, 144, 24, 96, (N, 1, 0), 4, **EPI),
    _s("w4h-stream-per4-short-last-workgroup-plain", WINO4H, 8, 0, 144, 24, 96, (N, 1, 0), 4, short=True),
    _s("w4h-stream-per4-short-last-workgroup-pro-stats", WINO4H, 8, 0, 144, 24, 96, (N, 2, 0), 4, short=True, pro=True, stats=True),
    _s("w4h-stream-per2-20x44-plain", WINO4H, 8, 0, 144, 20, 44, (N, 1, 1), 2),
    _s("w4h-stream-per2-20x44-pro", WINO4H, 8, 0, 144, 20, 44, (N, 2, 1), 2, pro=True),
    _s("w4h-stream-per2-20x44-two-src", WINO4H, 4, 4, 144, 20, 44, (N, 3, 1), 2),
    _s("w4h-stream-per2-20x44-epilogue-stats", WINO4H, 8, 0, 144, 20, 44, (N, 1, 1), 2, **EPI),
]

# tuples of REACHABLE that no row claims, each with its reason: none -- every one is reachable with small shapes
LEFT_OUT = {}

REACHABLE = {(k, m, s, r) for k in KERNELS for (m, s) in ((N, 1), (N, 2), (N, 3), (U, 1)) for r in (0, 1)}  # 8 per kernel, 24


def expected_instantiation(row):
    """(kernel, MODE, SPEC, RAG) of the instantiation launch_conv_wino / _wino4 / _wino4h starts for this row"""
    k = row["kernel"]
    TH, TW = PATCH[k]
    Hout, Wout = out_size(row)
    spec = 1 if row["mode"] == U else 2 if row["pro"] else 3 if row["C1"] else 1
    return (k, row["mode"], spec, int(bool(Hout % TH or Wout % TW)))


def kernel_name(t):
    """the instantiation as the demangled kernel name of a trace spells its template arguments"""
    return "%s<%d, %d, %s>" % (KERNEL_NAME[t[0]], t[1], t[2], "true" if t[3] else "false")


def eligible(row, kernel):
    """conv_wino_eligible (WINO) / conv_wino4_items > 0 and, for the 16x32 kernel, Cin >= 16 (WINO4, WINO4H), for a row whose weight
    images and prologue rows are 16-byte aligned (those of every table row are)"""
    Hout, Wout = out_size(row)
    Cin = row["C0"] + row["C1"]
    f4 = kernel != WINO
    if row["ks"] != 3 or row["mode"] not in (N, U):
        return False
    if row["Cout"] % 16 or Cin % 8 or (kernel == WINO4 and Cin < 16) or row["C0"] % (4 if f4 else 8):
        return False
    if Hout % (4 if f4 else 2) or Wout % (4 if f4 else 2) or Wout < 24:
        return False
    if row["mode"] == U and (row["pro"] or row["C1"]):
        return False
    if row["pro"] and row["C1"]:
        return False
    al = 4 if f4 else 2  # floats: float4 / float2 epilogue accesses
    for name in ("out",) + tuple(n for n in ("res", "aux") if row[n]):
        if _float_offset(row, name, Hout * Wout) % al or batch_stride(row, name, row["Cout"], Hout * Wout) % al:
            return False
    return True


def items_per_sample(row, kernel):
    Hout, Wout = out_size(row)
    TH, TW = PATCH[kernel]
    ncob = -(-row["Cout"] // (32 if row["Cout"] <= 32 else 64))
    return ncob, -(-Wout // TW), -(-Hout // TH)


def geometry(row, kernel, num_cu, B=None):
    """the launch of a row at batch B (default: the row's): items per sample, total, slots, per, grid, and seq(wg): the items
    (sample, patch row, patch column, channel block) of workgroup wg in the order it walks them -- by plain division"""
    B = row["B"] if B is None else B
    ncob, tiles_x, tiles_y = items_per_sample(row, kernel)
    items = ncob * tiles_x * tiles_y
    total = B * items
    slots = 2 * num_cu if kernel == WINO4H else num_cu
    per = -(-total // slots)
    grid = -(-total // per)

    def seq(wg):
        out = []
        for item in range(wg, total, grid):
            out.append((item // items, item // (ncob * tiles_x) % tiles_y, item // ncob % tiles_x, item % ncob))
        return out

    return dict(items=items, total=total, slots=slots, per=per, grid=grid, ncob=ncob, tiles_x=tiles_x, tiles_y=tiles_y, seq=seq)


def changes(seq):
    """which of (sample, patch row, patch column, channel block) change between two consecutive items of a workgroup's sequence"""
    out = set()
    for p, q in zip(seq, seq[1:]):
        out |= {w for w, a, b in zip(("sample", "row", "column", "block"), p, q) if a != b}
    return out


def counter_walk(g, wg):
    """advance_item of conv_wino4.hip / conv_wino4h.hip restated: the mixed-radix counter with the constant increment `grid`.
    Returns (items, carries): the items it visits from `wg` on and which carries (into 'column', 'row', 'sample') happened."""
    ncob, tiles_x, tiles_y, G = g["ncob"], g["tiles_x"], g["tiles_y"], g["grid"]
    d_cob, r1 = G % ncob, G // ncob
    d_px, r2 = r1 % tiles_x, r1 // tiles_x
    d_py, d_b = r2 % tiles_y, r2 // tiles_y
    cob, r1 = wg % ncob, wg // ncob
    px, r2 = r1 % tiles_x, r1 // tiles_x
    py, b = r2 % tiles_y, r2 // tiles_y
    items, carries = [(b, py, px, cob)], set()
    for _ in range(wg + G, g["total"], G):
        cob += d_cob
        c = cob >= ncob
        cob -= ncob if c else 0
        carries |= {"column"} if c else set()
        px += d_px + c
        c = px >= tiles_x
        px -= tiles_x if c else 0
        carries |= {"row"} if c else set()
        py += d_py + c
        c = py >= tiles_y
        py -= tiles_y if c else 0
        carries |= {"sample"} if c else set()
        b += d_b + c
        items.append((b, py, px, cob))
    return items, carries


def is_partial(row, kernel, item):
    """the patch of an item (sample, patch row, patch column, channel block) reaches beyond the image"""
    Hout, Wout = out_size(row)
    TH, TW = PATCH[kernel]
    return (item[1] + 1) * TH > Hout or (item[2] + 1) * TW > Wout


def _facts(row, kernel, num_cu, B):
    g = geometry(row, kernel, num_cu, B)
    full, carries, crossing = [], set(), []
    for wg in range(g["grid"]):
        s = g["seq"](wg)
        walked, c = counter_walk(g, wg)
        assert walked == s, (row["name"], wg, "the mixed-radix counter leaves the item sequence")
        carries |= c
        if changes(s) == {"sample", "row", "column", "block"}:
            full.append(wg)
        if len({is_partial(row, kernel, i) for i in s}) == 2:
            crossing.append(wg)
    return B, g, full, carries, crossing


def stream_facts(row, kernel, num_cu):
    """what the tests assert of an item-stream row on a device of num_cu CUs: (B, geometry, the workgroups whose sequence changes
    all four coordinates, the carries of the counter over the whole launch, the workgroups whose sequence holds whole and partial
    patches).  B is the smallest batch at which a workgroup walks row['stream']['per'] items and the row does what it is for: per = 4,
    some workgroup changes all four coordinates; per = 2 (the ragged image), some workgroup crosses between whole and partial patches.
    (With per = 2 the grid is total / 2 = B * items / 2, a multiple of the channel blocks whenever a sample has an even number of
    patches, as 20x44 has: the block never changes inside a sequence there, so all four coordinates change only in the per = 4 rows.)
    `short`: the next such B whose total is no multiple of per -- the last workgroup ends early, by another number of items."""
    want, short = row["stream"]["per"], row["stream"]["short"]
    B, first = 1, None
    while True:
        g = geometry(row, kernel, num_cu, B)
        assert g["per"] <= want, (row["name"], num_cu, "no batch gives this per")
        if g["per"] == want:
            f = _facts(row, kernel, num_cu, B)
            if f[2] if want >= 4 else f[4]:
                if not short or (first is not None and g["total"] % want != 0):
                    return f
                first = B if first is None else first
        B += 1
