"""CPU mirror of the Winograd weight-gradient rows of test_wgrad_wino_gpu.py: every row's claim (algo, per, empty, last_share,
crossings) follows from the rule restated in wgrad_wino_rows; the host-only idiff_conv2d_wgrad_ws_floats returns the largest of the
rule's three split counts for every row (an upper bound: the launched nsplit itself is witnessed on the GPU); every row's fp64 reference is computable and non-degenerate; and the table covers, for each of the two
kernels, what the rows are for.  No kernel is launched here."""
import ctypes

import pytest
import torch

from instancediff_amd import _lib

from wgrad_wino_ref import make_inputs, reference
from wgrad_wino_rows import (DIRECT, MAX_B, MAX_CH, MAX_HW, ROWS, TOL, U, WINO, WINO4, eligible, expected, geometry, out_size, pick_algo,
                             ws_splits)

IDS = [r["name"] for r in ROWS]


def desc(row):
    """the descriptor of a row as far as idiff_conv2d_wgrad_ws_floats reads it: the dimensions, mode and kernel size"""
    d = _lib.ConvDesc()
    d.C0, d.C1 = row["C0"], row["C1"]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = row["B"], row["Hin"], row["Win"], row["mode"], 3, row["Cout"]
    return d


def test_row_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_claim_follows_from_the_rule(row):
    assert row["claim"] == expected(row), (row["name"], expected(row))
    g = geometry(row)
    algo, per, empty, last, crossings = row["claim"]
    assert algo in TOL
    # the row is a call the header accepts, within the size limits
    assert not (row["pro"] and row["C1"]) and not (row["slc"] and row["dyoff"])
    Hout, Wout = out_size(row)
    assert row["B"] <= MAX_B and max(row["C0"] + row["C1"], row["Cout"]) <= MAX_CH and Hout * Wout <= MAX_HW, row["name"]
    if algo == DIRECT:
        return
    # the shares tile the chunk list: full shares, one last share, empty splits
    assert g["nsplit"] == g["used"] + empty and (g["used"] - 1) * per + last == g["total"] and 1 <= last <= per
    assert all(1 <= p < per for p in crossings)
    if row["slc"]:
        assert row["B"] >= 2
    if row["core"]:
        assert not (row["pro"] or row["acc"] or row["slc"] or row["dc"] or row["mode"] == U)


def test_rule_at_its_edges():
    """the ladder's rungs one step off each core shape"""
    base = next(r for r in ROWS if r["name"] == "w4-B2-256-256-12x48-per2")
    assert pick_algo(base) == WINO4
    for dyoff, want in ((0, WINO4), (2, WINO), (1, DIRECT), (3, DIRECT), (4, WINO4)):
        assert pick_algo(dict(base, dyoff=dyoff)) == want, dyoff
    assert pick_algo(dict(base, Hin=14)) == WINO and pick_algo(dict(base, Hin=13)) == DIRECT
    assert pick_algo(dict(base, Win=40)) == DIRECT and pick_algo(dict(base, Cout=192)) == WINO4 and pick_algo(dict(base, Cout=96)) == DIRECT
    assert pick_algo(dict(base, C0=240)) == WINO4 and pick_algo(dict(base, C0=248)) == DIRECT
    two = dict(base, C0=64, C1=80)
    assert pick_algo(two) == WINO4 and pick_algo(dict(two, C0=32, C1=48)) == WINO4 and pick_algo(dict(two, C0=32, C1=48, Hin=14)) == DIRECT
    assert pick_algo(dict(two, Hin=14)) == WINO and pick_algo(dict(two, C0=48, C1=16)) == DIRECT
    assert pick_algo(dict(two, mode=U)) == DIRECT and pick_algo(dict(base, mode=U, pro=True)) == DIRECT and pick_algo(dict(base, mode=U)) == WINO4
    assert eligible(base, WINO)  # algo 3 is tried first


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_workspace_query_returns_the_rule(row):
    """idiff_conv2d_wgrad_ws_floats (host only) = 9 Cin Cout x the largest split count of the forms the shape could get, and so holds every
    split's partial image of dW on the form the row claims -- room for it, not proof of it"""
    lib = _lib.load()
    g = geometry(row)
    d = desc(row)
    Cin = row["C0"] + row["C1"]
    nws = lib.idiff_conv2d_wgrad_ws_floats(ctypes.byref(d))
    assert nws == ws_splits(row) * 9 * Cin * row["Cout"], (row["name"], nws, ws_splits(row))
    assert nws >= g["nsplit"] * 9 * Cin * row["Cout"]
    # dY's alignment moves a row down the ladder, never to a form with more splits than the workspace holds
    for dyoff in (0, 1, 2):
        assert geometry(dict(row, dyoff=dyoff, slc=0))["nsplit"] <= ws_splits(row)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_reference_is_computable_and_not_degenerate(row):
    inp = make_inputs(row)
    ref = reference(row, inp)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (row["Cout"], row["C0"] + row["C1"], 3, 3)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
    if row["pro"]:  # a table of the wrong sample is an O(1) change of the activation
        pa, pb = inp["pro"]
        assert float((pa[1:] - pa[:-1]).abs().min()) > 0.3 and float((pb[1:] - pb[:-1]).abs().min()) > 0.2


@pytest.mark.parametrize("algo", [WINO, WINO4], ids=["F2x2", "F4x4"])
def test_table_covers_what_the_rows_are_for(algo):
    rows = [r for r in ROWS if r["claim"][0] == algo]
    per = lambda r: r["claim"][1]  # noqa: E731
    cross = lambda r: r["claim"][4]  # noqa: E731
    assert any(per(r) >= 3 for r in rows) and any(per(r) == 2 for r in rows)
    assert any(r["claim"][2] > 0 for r in rows), "a row with empty splits"
    assert any(r["claim"][3] < per(r) for r in rows), "a row whose last used share is short"
    assert any(1 in cross(r) for r in rows) and any(max(cross(r), default=0) >= 2 for r in rows)
    assert any(r["pro"] and cross(r) for r in rows), "a prologue row whose table is reloaded inside a share"
    assert any(r["mode"] == U and per(r) >= 2 for r in rows)
    assert any(r["C1"] and (r["C0"] + r["C1"]) % geometry(r)["cib"] for r in rows), "a two-source row with a partial last ci block"
    assert any(r["slc"] and r["C1"] for r in rows) and any(r["acc"] for r in rows) and any(r["dc"] for r in rows)
    assert sum(1 for r in rows if r["core"]) >= 4


def test_table_covers_the_alignment_rungs():
    assert any(r["dyoff"] % 4 == 2 and r["claim"][0] == WINO and eligible(dict(r, dyoff=0), WINO4) for r in ROWS), "8-byte dY on a shape algo 3 tiles"
    assert any(r["dyoff"] % 2 == 1 and r["claim"][0] == DIRECT and eligible(dict(r, dyoff=0), WINO4) for r in ROWS), "4-byte dY: direct"
    assert any(r["C1"] and r["C0"] % 32 and r["claim"][0] == DIRECT and eligible(dict(r, C0=r["C0"] + r["C1"], C1=0), WINO4) for r in ROWS)
    assert any(r["C1"] and r["C0"] % 64 and r["claim"][0] == WINO4 and eligible(dict(r, C0=r["C0"] + r["C1"], C1=0), WINO) for r in ROWS)
