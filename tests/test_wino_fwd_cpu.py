"""CPU mirror of the Winograd forward table of test_wino_fwd_gpu.py, without a GPU and without the library: every row's claimed
instantiation follows from the launch rule restated in wino_fwd_rows.expected_instantiation, the rows claim all 24 reachable
instantiations, every row is a call its kernel's eligibility check accepts, the item-stream rows reach their `per`, their short last
workgroup and every carry of the item counter on a 256-CU device, and the Winograd form that floors the tolerances is the
convolution (fp64, 1e-12) -- a change of the rule, of a row or of a transform matrix trips here before any GPU is involved."""
import pytest
import torch
import torch.nn.functional as F

from conv_branch_ref import make_inputs, reference, tile_stats
from wino_fwd_rows import (KERNELS, LEFT_OUT, MIRROR_CUS, N, PATCH, REACHABLE, ROWS, U, WINO, WINO4, WINO4H, eligible, expected_instantiation,
                           geometry, kernel_name, out_size, stream_facts)
from winograd_form_ref import form_reference, winograd_conv3x3

IDS = [r["name"] for r in ROWS]
STREAM = [r for r in ROWS if r["stream"]]
TABLE = [r for r in ROWS if not r["stream"]]


def test_row_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_claim_follows_from_the_rule_and_the_row_is_eligible(row):
    assert row["claim"] == expected_instantiation(row), row["name"]
    assert row["claim"] in REACHABLE and row["claim"][0] == row["kernel"], row["name"]
    assert eligible(row, row["kernel"]), row["name"]
    assert not (row["pro"] and row["C1"]) and row["ks"] == 3
    if row["gn"]:
        assert row["Cout"] % row["gn"] == 0


def test_rows_claim_every_reachable_instantiation():
    assert len(REACHABLE) == 24 and all(sum(1 for t in REACHABLE if t[0] == k) == 8 for k in KERNELS)
    claimed = {r["claim"] for r in TABLE}
    assert claimed == REACHABLE, sorted(REACHABLE - claimed)
    assert LEFT_OUT == {}
    assert len({kernel_name(t) for t in REACHABLE}) == 24


def test_eligibility_rule_at_its_edges():
    """the rule itself, on variations of one row: what each kernel refuses"""
    base = next(r for r in ROWS if r["name"] == "w4-n1-48x96-C16-four-chunks-Cout144-out-slice")
    assert all(eligible(base, k) for k in KERNELS)
    v = lambda **kw: dict(base, **kw)  # noqa: E731
    assert [eligible(v(C0=8), k) for k in KERNELS] == [True, False, True]          # Cin 8: fewer than four chunks of the 16x32 kernel
    assert [eligible(v(C0=12, C1=4), k) for k in KERNELS] == [False, True, True]   # C0 % 8 (F(2x2)) / C0 % 4 (F(4x4))
    assert [eligible(v(Hin=50), k) for k in KERNELS] == [True, False, False]       # H even / H % 4
    assert not any(eligible(v(Win=20), k) for k in KERNELS) and not any(eligible(v(Cout=72), k) for k in KERNELS)
    assert not any(eligible(v(mode=U, pro=True), k) for k in KERNELS) and not any(eligible(v(mode=U, C0=8, C1=8), k) for k in KERNELS)
    assert [eligible(v(odd=("out",)), k) for k in KERNELS] == [False, False, False]
    assert [eligible(v(res=True, odd=("res",)), k) for k in KERNELS] == [False, False, False]


def test_table_covers_what_the_rows_are_for():
    for k in KERNELS:
        rows = [r for r in TABLE if r["kernel"] == k]
        TH, TW = PATCH[k]
        sizes = {out_size(r) for r in rows}
        assert (3 * TH, 3 * TW) in sizes, k                                         # a patch without an image edge
        assert any(out_size(r)[1] < TW for r in rows), k                            # image narrower than a patch
        for name in ("src0", "src1", "res", "aux", "out"):
            assert any(name in r["slices"] for r in rows), (k, name)
        assert any("src0" in r["odd"] for r in rows), k
        assert any(r["dc"] and r["pro"] for r in rows) and any(r["dc"] and not r["pro"] for r in rows), k
        assert {16, 48, 64, 80, 128, 144} <= {r["Cout"] for r in rows}, k
        assert any(r["gn"] for r in rows) and any(not r["bias"] for r in rows), k
        alone = lambda key: any(r[key] and not any(r[o] for o in ("res", "vec", "aux") if o != key) for r in rows)  # noqa: E731
        assert alone("res") and alone("vec") and alone("aux"), k
        assert any(r["res"] and r["vec"] and r["aux"] and r["stats"] and r["bias"] for r in rows), k
        assert any(r["mode"] == U and expected_instantiation(r)[3] for r in rows), k
        two = [r for r in rows if r["C1"]]
        ck = 8 if k == WINO else 4
        assert any(r["C1"] == ck for r in two), k                                   # the second source is a single chunk
        if k != WINO:
            assert any(r["C0"] % 8 == 4 for r in two), k                            # the sources meet inside an 8-channel pair
        # the limits on the rows' sizes
        for r in rows:
            Hout, Wout = out_size(r)
            assert r["B"] == 2 and max(r["C0"] + r["C1"], r["Cout"]) <= 144 and Hout * Wout <= 48 * 96, r["name"]
    chunks = lambda r: (r["C0"] + r["C1"]) // (8 if r["kernel"] == WINO else 4)  # noqa: E731
    assert {1, 3, 5} <= {chunks(r) for r in TABLE if r["kernel"] == WINO}
    assert min(chunks(r) for r in TABLE if r["kernel"] == WINO4) == 4 and min(chunks(r) for r in TABLE if r["kernel"] == WINO4H) == 2
    assert {(10, 24), (12, 40), (12, 28)} <= {out_size(r) for r in TABLE if r["kernel"] == WINO}
    h4 = {out_size(r)[0] for r in TABLE if r["kernel"] == WINO4}
    w4 = {out_size(r)[1] for r in TABLE if r["kernel"] == WINO4}
    assert {8, 24, 20, 28} <= h4 and {24, 36, 44} <= w4


@pytest.mark.parametrize("row", STREAM, ids=[r["name"] for r in STREAM])
def test_item_stream_rows_reach_their_pipeline_depth(row):
    k = row["kernel"]
    B, g, full, carries, crossing = stream_facts(row, k, MIRROR_CUS)
    want = row["stream"]["per"]
    assert g["per"] == want and g["grid"] <= g["slots"] == (512 if k == WINO4H else 256)
    assert g["items"] == (27 if want == 4 else (12 if k == WINO4 else 18))
    last = g["seq"](g["grid"] - 1)
    if row["stream"]["short"]:
        assert g["total"] % want != 0 and len(last) < want                          # ends early: the 16x32 kernel streams the null item
    assert len(g["seq"](0)) == want
    assert sorted(i for wg in range(g["grid"]) for i in g["seq"](wg)) == sorted(
        (b, y, x, c) for b in range(B) for y in range(g["tiles_y"]) for x in range(g["tiles_x"]) for c in range(g["ncob"]))
    if want == 4:
        assert carries == {"column", "row", "sample"}, (row["name"], carries)
        assert full, row["name"]                                                   # one workgroup changes all four coordinates
        assert B == {False: {WINO: 29, WINO4: 29, WINO4H: 57}, True: {WINO: 30, WINO4: 30, WINO4H: 58}}[row["stream"]["short"]][k]
    else:
        assert crossing, row["name"]                                               # whole and partial patches in one sequence
    assert B * row["Cout"] * row["Hin"] * row["Win"] * 4 < 80e6


def test_stream_rows_cover_the_variants():
    for k in KERNELS:
        for per in (4, 2):
            rows = [r for r in STREAM if r["kernel"] == k and r["stream"]["per"] == per and not r["stream"]["short"]]
            assert any(r["pro"] for r in rows) and any(r["C1"] for r in rows) and any(r["res"] and r["stats"] for r in rows), (k, per)
            assert any(not (r["pro"] or r["C1"] or r["res"] or r["stats"]) for r in rows), (k, per)
        assert any(r["stream"]["short"] for r in STREAM if r["kernel"] == k), k
        assert all(expected_instantiation(r)[3] == (r["stream"]["per"] == 2) for r in STREAM if r["kernel"] == k), k


def test_geometry_is_the_launchers_arithmetic():
    row = next(r for r in ROWS if r["name"] == "w2-n1-24x96-C8-one-chunk-Cout144-out-slice")
    g = geometry(row, WINO, 256)
    assert (g["items"], g["total"], g["per"], g["grid"]) == (27, 54, 1, 54) and g["seq"](5) == [(0, 0, 1, 2)]
    g = geometry(row, WINO, 256, B=29)
    assert (g["total"], g["per"], g["grid"]) == (783, 4, 196) and len(g["seq"](195)) == 3
    assert g["seq"](1) == [(0, 0, 0, 1), (7, 0, 2, 2), (14, 1, 2, 0), (21, 2, 1, 1)]
    g = geometry(row, WINO4H, 256, B=57)
    assert (g["total"], g["slots"], g["per"], g["grid"]) == (1539, 512, 4, 385)
    row16 = next(r for r in ROWS if r["name"] == "w2-n1-10x24-C40-Cout16-vec")
    assert geometry(row16, WINO, 256)["items"] == 2


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("shape", ["ragged", "upsampled"])
def test_winograd_form_in_fp64_is_the_convolution(m, shape):
    g = torch.Generator().manual_seed(9 + m)
    if shape == "ragged":
        x = torch.randn(2, 5, 10, 27, generator=g, dtype=torch.float64)
    else:
        x = F.interpolate(torch.randn(2, 5, 6, 14, generator=g, dtype=torch.float64), scale_factor=2, mode="nearest")
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64) / 45 ** 0.5
    ref = F.conv2d(x, w, None, padding=1)
    got = winograd_conv3x3(x, w, m)
    assert got.shape == ref.shape and got.dtype == torch.float64
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


@pytest.mark.parametrize("row", [r for r in TABLE if r["pro"] or r["mode"] == U or r["C1"]][::3], ids=lambda r: r["name"])
def test_form_reference_is_the_rows_reference_in_fp64(row):
    """prologue, virtual concat, upsample and the whole epilogue around the form"""
    inp = make_inputs(row, 7)
    ref, raw = reference(row, inp)
    out, fraw = form_reference(row, inp, 2 if row["kernel"] == WINO else 4, torch.float64)
    scale = float(ref.abs().max())
    assert float((out - ref).abs().max()) / scale < 1e-12 and float((fraw - raw).abs().max()) / float(raw.abs().max()) < 1e-12
    if row["stats"]:
        st = tile_stats(raw)
        Hout, Wout = out_size(row)
        assert st.shape[1] == -(-Hout // 8) * -(-Wout // 32)
        assert torch.allclose(tile_stats(fraw), st, rtol=1e-10, atol=1e-9)


@pytest.mark.parametrize("row", TABLE, ids=[r["name"] for r in TABLE])
def test_reference_is_computable_and_not_degenerate(row):
    inp = make_inputs(row, 3000 + IDS.index(row["name"]))
    out, raw = reference(row, inp)
    Hout, Wout = out_size(row)
    assert out.dtype == torch.float64 and tuple(out.shape) == (row["B"], row["Cout"], Hout, Wout)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1 and float(raw.abs().max()) > 0.1
    if row["mode"] == N:
        assert (Hout, Wout) == (row["Hin"], row["Win"])
