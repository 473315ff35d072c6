"""What the host side of the conv path guarantees since the forward call is "arguments, choice, launch" and the weight gradient sizes
its workspace by the kernels' own shape predicates -- on descriptors of made-up addresses, without a GPU: the rules of a descriptor's
mode are refused by idiff_conv2d_plan with their messages, a refused idiff_conv2d_plan / idiff_conv2d_fwd (refused before any HIP
call) leaves idiff_conv2d_last_algo() alone, and the workspace query holds the chosen weight-gradient form of every row of
wgrad_wino_rows (the bound beside the exact value of test_wgrad_wino_cpu)."""
import ctypes

import pytest

from instancediff_amd import _lib
from instancediff_amd._lib import ConvDesc

from wgrad_wino_rows import ROWS, geometry

E_BADARG = -1
N, U, S = 0, 1, 2  # IDIFF_CONV_NORMAL / UPSAMPLE2 / UNSHUFFLE2
WINOGRAD4 = 3


def fake_desc(ks, mode, Hin=16, Win=32, C0=32, C1=0, Cout=64, req=0, operands=0):
    """a descriptor the argument checks accept up to the rules under test: distinct 16-byte-aligned addresses that are never read"""
    Hout, Wout = (2 * Hin, 2 * Win) if mode == U else ((Hin // 2, Win // 2) if mode == S else (Hin, Win))
    d = ConvDesc()
    d.src0, d.src0_bstride, d.C0 = 0x10000000, C0 * Hin * Win, C0
    if C1:
        d.src1, d.src1_bstride, d.C1 = 0x14000000, C1 * Hin * Win, C1
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = 2, Hin, Win, mode, ks, Cout
    d.wpk, d.bias, d.out, d.out_bstride = 0x18000000, 0x1C000000, 0x20000000, Cout * Hout * Wout
    d.algo_request, d.operands = req, operands
    return d


REFUSED = [
    ("1x1-upsample", dict(ks=1, mode=U), "conv2d: upsample mode needs ks=3"),
    ("7x7-upsample", dict(ks=7, mode=U), "conv2d: ks=7 needs normal mode"),
    ("3x3-unshuffle", dict(ks=3, mode=S), "conv2d: unshuffle mode needs ks=1 and a single source"),
    ("7x7-unshuffle", dict(ks=7, mode=S), "conv2d: unshuffle mode needs ks=1 and a single source"),
    ("unshuffle-two-sources", dict(ks=1, mode=S, C1=32), "conv2d: unshuffle mode needs ks=1 and a single source"),
    ("unshuffle-odd-H", dict(ks=1, mode=S, Hin=15), "conv2d: unshuffle needs even H, W"),
    ("unshuffle-odd-W", dict(ks=1, mode=S, Win=31), "conv2d: unshuffle needs even H, W"),
    # refused by the choice, not by the descriptor's shape
    ("winograd4-by-name-on-1x1", dict(ks=1, mode=N, req=1 + WINOGRAD4), "conv2d: algo_request F(4x4,3x3) but the shape does not tile for it"),
    ("operands-2", dict(ks=3, mode=N, operands=2), "conv2d: bad operands 2"),
]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_accepted_pairs_plan(lib):
    for ks, mode in ((1, N), (1, S), (3, N), (3, U), (7, N)):
        assert lib.idiff_conv2d_plan(ctypes.byref(fake_desc(ks, mode))) >= 0, (ks, mode, lib.idiff_last_error())


@pytest.mark.parametrize("name,kw,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_plan_refuses_with_the_message(lib, name, kw, message):
    assert lib.idiff_conv2d_plan(ctypes.byref(fake_desc(**kw))) == E_BADARG
    assert lib.idiff_last_error().decode() == message


@pytest.mark.parametrize("name,kw,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_refused_call_leaves_last_algo(lib, name, kw, message):
    """both entry points refuse these before the first HIP call, so the forward entry is safe to call here"""
    keep = lib.idiff_conv2d_last_algo()
    d = fake_desc(**kw)
    assert lib.idiff_conv2d_plan(ctypes.byref(d)) == E_BADARG and lib.idiff_conv2d_last_algo() == keep
    assert lib.idiff_conv2d_fwd(ctypes.byref(d), None) == E_BADARG and lib.idiff_conv2d_last_algo() == keep
    assert lib.idiff_last_error().decode() == message


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_workspace_holds_the_chosen_form(lib, row):
    d = ConvDesc()
    d.C0, d.C1 = row["C0"], row["C1"]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = row["B"], row["Hin"], row["Win"], row["mode"], 3, row["Cout"]
    Cin = row["C0"] + row["C1"]
    assert lib.idiff_conv2d_wgrad_ws_floats(ctypes.byref(d)) >= geometry(row)["nsplit"] * 9 * Cin * row["Cout"], row["name"]
