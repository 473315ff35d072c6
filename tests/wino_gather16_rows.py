"""Rows for the 16-byte gather of conv_wino4_kernel (csrc/conv_wino4.hip, the G16 form): the smallest shapes that reach each of its
paths, in the row format of wino_fwd_rows.py.  Shared by test_wino_gather16_gpu.py and scripts/record_wino_gather16_golden.py; plain
data, nothing here imports the library.

Which gather serves a row is decided in launch_rag: normal mode, no prologue, 16-byte aligned sources and batch strides of whole
float4 -> 16-byte pieces; else the dword gather.  Both compute the same sums in the same order: the same bits."""
from wino_fwd_rows import N, U, WINO4, _r

SEED0 = 9100  # make_inputs seed of row k: SEED0 + k

ROWS = [
    # one patch, the halo outside the image on all four sides, four chunks
    _r("g16-n1-16x32-C16-one-patch-halos-outside", WINO4, N, 16, 0, 32, 16, 32, (N, 1, 0), B=1, stats=True),
    # 2 x 2 patches: left / right halo columns from the neighbouring patch, top and bottom rows
    _r("g16-n1-32x64-C16-halos-from-neighbours", WINO4, N, 16, 0, 16, 32, 64, (N, 1, 0), B=1, stats=True),
    # ragged: patches at x0 = 32 whose pieces from column 40 on lie beyond Wout, masked stores
    _r("g16-n1-20x40-C16-ragged-pieces-beyond-Wout", WINO4, N, 16, 0, 16, 20, 40, (N, 1, 1), B=2, res=True, stats=True),
    # two sources, C0v = 24: chunks 0..5 from src0, 6..9 from src1
    _r("g16-n3-16x32-C24-and-C16-sources-change-at-chunk-6", WINO4, N, 24, 16, 32, 16, 32, (N, 3, 0), B=1, stats=True),
    # prologue with b != 0: silu(b) != 0, the padding must be zero AFTER the activation (this form keeps the dword gather)
    _r("g16-n2-16x32-C16-pro-nonzero-b", WINO4, N, 16, 0, 32, 16, 32, (N, 2, 0), B=1, pro=True, stats=True),
    # src0 four bytes past a 16-byte boundary: the dword gather, same bits as the aligned call
    _r("g16-n1-32x64-C16-src0-4-bytes-past-16", WINO4, N, 16, 0, 16, 32, 64, (N, 1, 0), B=1, stats=True, odd=("src0",)),
    # upsample: a replicated source is no contiguous piece -- the dword gather, unchanged
    _r("g16-u1-8x16-C16-upsample", WINO4, U, 16, 0, 16, 8, 16, (U, 1, 0), B=1, stats=True),
    # 3 x 128 = 384 items: more than one per workgroup on any device of fewer CUs -- the table is rewritten mid-stream
    _r("g16-n1-256x256-C16-B3-384-items", WINO4, N, 16, 0, 16, 256, 256, (N, 1, 0), B=3),
]
GOLDEN = [r["name"] for r in ROWS[:6]]  # recorded on the parent commit's build: tests/golden/wino_gather16/<name>.npz
ITEMS_BIG = 3 * (256 // 16) * (256 // 32)
