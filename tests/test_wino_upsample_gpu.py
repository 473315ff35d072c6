"""conv_wino4_kernel<1, 1, RAG> (csrc/conv_wino4.hip): the F(4x4,3x3) kernel in upsample mode leaves out the 11 Winograd positions that
are exactly +0 for a nearest x2 upsampled source (pos_live, csrc/wino_common.h; the rule itself: test_wino_upsample_cpu.py).  Every row
is asked for by name (a hard algo request; idiff_conv2d_last_algo() must name the kernel) and checked two ways:

1. bit equality (torch.equal, output and statistics) with the same library's normal-mode call on the materialised nearest-upsampled
   input, same weights, forced onto the same algorithm: that kernel multiplies all 36 positions.  On a build of the commit before the
   upsample form left the dead positions out this equality holds for all six rows (profiles/r26/README.md), so it pins the parent's bits.
2. a plain torch float64 evaluation on the CPU (conv_branch_ref.reference), with the F(4x4,3x3) tolerances of test_wino_fwd_gpu.py:
   4e-5 of the output range, statistics totals 4e-5, per tile 1e-4.

Rows: (a) 32x64 -> 64x128, 16 -> 16 channels, B 1: the least the kernel accepts (4 chunks, 16 items, one channel block masked to 16);
(b) 32x32 -> 64x64, 24 -> 80, B 2: two channel blocks, the second partial; (c) 36x68 -> 72x136, 16 -> 16: RAG, partial patches right and
bottom; (d) 128x128 -> 256x256, 16 -> 16, B 3: 384 items, workgroups that carry the pipeline from one item into the next; (e) as (b)
with bias and statistics; (f) as (a) with residual and per-(b, c) vector."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops  # noqa: E402

from conv_branch_ref import make_inputs, reference, tile_stats  # noqa: E402
from conv_guard_util import DEV, _check  # noqa: E402
from wino_fwd_rows import N, U, WINO4, eligible, expected_instantiation  # noqa: E402

TOL_OUT, TOL_SUM, TOL_TILE = 4e-5, 4e-5, 1e-4  # TOL_ALGO / TOL_SUM / TOL_TILE [WINO4] of test_wino_fwd_gpu.py


def _row(name, Hin, Win, Cin, Cout, B, rag, **kw):
    row = dict(name=name, kernel=WINO4, ks=3, mode=U, B=B, C0=Cin, C1=0, Cout=Cout, Hin=Hin, Win=Win, pro=False, res=False, vec=False,
               aux=False, bias=False, stats=False, gn=0, slices={}, odd=(), dc=False, claim=(WINO4, U, 1, rag))
    row.update(kw)
    return row


ROWS = [
    _row("a-32x64-C16-Cout16-least", 32, 64, 16, 16, 1, 0),
    _row("b-32x32-C24-Cout80-two-blocks", 32, 32, 24, 80, 2, 0),
    _row("c-36x68-C16-Cout16-ragged", 36, 68, 16, 16, 1, 1),
    _row("d-128x128-C16-Cout16-B3-384-items", 128, 128, 16, 16, 3, 0),
    _row("e-32x32-C24-Cout80-bias-stats", 32, 32, 24, 80, 2, 0, bias=True, stats=True),
    _row("f-32x64-C16-Cout16-res-vec", 32, 64, 16, 16, 1, 0, res=True, vec=True),
]


def _launch(row, inp, x, mode):
    """the row's conv of source x in `mode` on the F(4x4,3x3) kernel by name: (out, stats or None)"""
    lib = _lib.load()
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    r = ops.conv2d(x, ops.pack_conv_weight(inp["w"].to(DEV)), dev(inp["bias"]), 3, row["Cout"], mode=mode, res=dev(inp["res"]),
                   vec=dev(inp["vec"]), want_stats=row["stats"], algo=WINO4)
    torch.cuda.synchronize()
    assert lib.idiff_conv2d_last_algo() == WINO4, (row["name"], lib.idiff_conv2d_last_algo())
    return r if row["stats"] else (r, None)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_upsample_form_gives_the_bits_of_all_36_positions(row):
    assert ops.WINOGRAD and ops.WINOGRAD4, "tested at the process-wide switches' defaults"
    assert row["claim"] == expected_instantiation(row) and eligible(row, WINO4)
    if row["name"].startswith("d"):
        assert row["B"] * (2 * row["Hin"] // 16) * (2 * row["Win"] // 32) == 384
    inp = make_inputs(row, 2600 + [r["name"] for r in ROWS].index(row["name"]))
    x = inp["src0"].to(DEV)
    out, st = _launch(row, inp, x, U)
    # 1. the normal-mode kernel (all 36 positions) on the materialised upsample: the same bits
    xu = F.interpolate(x, scale_factor=2, mode="nearest").contiguous()
    assert torch.equal(xu[:, :, 1::2, 0::2], x) and torch.equal(xu[:, :, 0::2, 1::2], x)
    out36, st36 = _launch(dict(row, mode=N), inp, xu, N)
    assert out.shape == out36.shape == (row["B"], row["Cout"], 2 * row["Hin"], 2 * row["Win"])
    nbad = int((out.view(torch.int32) != out36.view(torch.int32)).sum())
    print(f"{row['name']}: {nbad} of {out.numel()} output words differ from the 36-position kernel")
    assert torch.equal(out, out36), f"{row['name']}: {nbad} output elements differ from the 36-position kernel"
    if row["stats"]:
        assert torch.equal(st, st36), f"{row['name']}: statistics differ from the 36-position kernel"
    # 2. fp64 on the CPU
    ref, raw = reference(row, inp)
    every = slice(None)
    Ho, Wo = out.shape[2:]
    tails = [("top row", (every, every, slice(0, 1))), ("bottom row", (every, every, slice(Ho - 1, Ho))),
             ("left column", (every, every, every, slice(0, 1))), ("right column", (every, every, every, slice(Wo - 1, Wo)))]
    _check(row["name"], "out", out, ref, TOL_OUT, tails)
    if row["stats"]:
        want = tile_stats(raw)
        s = st.double().cpu()
        assert tuple(s.shape) == tuple(want.shape)
        for w, what in ((0, "sum"), (1, "sumsq")):
            _check(row["name"], f"stats {what} total", s.sum(1)[..., w], want.sum(1)[..., w], TOL_SUM)
            _check(row["name"], f"stats {what} per tile", s[..., w], want[..., w], TOL_TILE)
