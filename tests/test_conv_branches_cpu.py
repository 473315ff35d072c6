"""CPU mirror of the direct-kernel branch table of test_conv_branches_gpu.py: every row's claimed instantiation follows from the
dispatch rule restated in conv_branch_rows.expected_branch, the rows claim every reachable instantiation, the host-only
idiff_conv2d_num_tiles agrees with the tile grid the statistics reference walks, and every row's fp64 reference is computable and
non-degenerate -- a change of the rule or of a row trips here before any GPU is involved."""
import pytest
import torch

from instancediff_amd import _lib

from conv_branch_ref import make_inputs, reference, tile_stats
from conv_branch_rows import LEFT_OUT, N, REACHABLE, ROWS, S, U, expected_branch, out_size, pick_twl, tile_shape

IDS = [r["name"] for r in ROWS]


def test_row_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_claim_follows_from_the_rule(row):
    assert row["claim"] == expected_branch(row), row["name"]
    assert row["claim"] in REACHABLE, row["name"]
    # the row is a call the header accepts
    assert row["ks"] in (1, 3, 7) and not (row["pro"] and row["C1"])
    if row["mode"] == S:
        assert row["ks"] == 1 and row["C1"] == 0 and row["Hin"] % 2 == 0 and row["Win"] % 2 == 0
    if row["mode"] == U:
        assert row["ks"] == 3
    if row["ks"] == 7:
        assert row["mode"] == N
    if row["gn"]:
        assert row["Cout"] % row["gn"] == 0


def test_rows_claim_every_reachable_instantiation():
    assert len(REACHABLE) == 65
    claimed = {r["claim"] for r in ROWS}
    assert claimed <= REACHABLE
    assert len(LEFT_OUT) <= 3 and all(isinstance(v, str) and v for v in LEFT_OUT.values())
    assert REACHABLE - claimed == set(LEFT_OUT), sorted(REACHABLE - claimed)


def test_table_covers_what_the_rows_are_for():
    """per (ks, mode): a DC-offset row and an `out` slice with a guard band; per table: every operand once as a slice, misaligned
    views, statistics from MB = 1 for every ks, every reason a 1x1 layer does not flatten"""
    fam = {}
    for r in ROWS:
        fam.setdefault((r["ks"], r["mode"]), []).append(r)
    assert set(fam) == {(3, N), (3, U), (1, N), (1, S), (7, N)}
    for key, rows in fam.items():
        assert any(r["dc"] for r in rows), key
        assert any("out" in r["slices"] for r in rows), key
        assert any(r["pro"] for r in rows), key
        assert any(r["stats"] for r in rows), key
    for name in ("src0", "src1", "res", "aux", "out"):
        assert any(name in r["slices"] for r in ROWS), name
    assert any("src0" in r["odd"] for r in ROWS) and any("wpk" in r["odd"] for r in ROWS)
    assert {r["ks"] for r in ROWS if r["stats"] and r["claim"][4] == 1} == {1, 3, 7}
    assert sum(1 for r in ROWS if r["gn"]) >= 2
    no_flat = [r for r in ROWS if r["claim"] == (1, N, 5, 1, 2, 0)]
    Hw = [out_size(r) for r in no_flat]
    assert any(r["stats"] for r in no_flat) and any((h * w) % 256 for h, w in Hw) and any(w < 32 for h, w in Hw)
    assert any("src0" in r["odd"] for r in no_flat)
    # the limits the issue sets on the rows' sizes
    for r in ROWS:
        big = r["name"] in ("c7n-t5-v1-m2-product-224x224-C2-stats", "c1n-flat-spec1-product-256-256-64x64-res-aux")
        Hout, Wout = out_size(r)
        assert r["B"] <= 3 and (big or (max(r["C0"] + r["C1"], r["Cout"]) <= 160 and Hout * Wout <= 64 * 96)), r["name"]


@pytest.mark.parametrize("Hout,Wout", sorted({out_size(r) for r in ROWS} | {(8, 23), (8, 24), (8, 15), (8, 16), (1, 1), (9, 33)}))
def test_num_tiles_is_the_grid_of_the_reference(Hout, Wout):
    TH, TW = tile_shape(pick_twl(Wout))
    assert TH * TW == 256
    assert _lib.load().idiff_conv2d_num_tiles(Hout, Wout) == -(-Hout // TH) * -(-Wout // TW)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_reference_is_computable_and_not_degenerate(row):
    inp = make_inputs(row, 1000 + IDS.index(row["name"]))
    out, raw = reference(row, inp)
    Hout, Wout = out_size(row)
    assert out.dtype == torch.float64 and tuple(out.shape) == (row["B"], row["Cout"], Hout, Wout)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1
    assert float(raw.abs().max()) > 0.1
    if row["stats"]:
        st = tile_stats(raw)
        assert st.shape[1] == _lib.load().idiff_conv2d_num_tiles(Hout, Wout)
        assert bool(torch.isfinite(st).all()) and float(st[..., 1].min()) > 0
        assert torch.allclose(st.sum(1)[..., 0], raw.sum(dim=(2, 3)), rtol=1e-12, atol=1e-9)
    if row["mode"] == U:
        assert (Hout, Wout) == (2 * row["Hin"], 2 * row["Win"])
