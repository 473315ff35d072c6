"""CPU mirror of the matrix-core forward tables of test_mfma_fwd_gpu.py, without a GPU: every row's claimed instantiation follows from
the rule restated in mfma_fwd_rows.expected_instantiation, the rows claim all 14 reachable instantiations and cover what they are
for, idiff_conv2d_plan -- host code that never dereferences an operand -- answers mfma_fwd_rows.expected_algo for every row and every
case of the selection ladder on a descriptor of made-up addresses, the Python three-way split and the two weight-image layouts hold
their own invariants, and every row's references are computable and not degenerate.  A change of the selection rule, of a row or of
the split trips here before any GPU is involved."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from instancediff_amd import _lib
from instancediff_amd._lib import ConvDesc

from conv_branch_ref import make_inputs, reference, tile_stats
from conv_branch_rows import _float_offset, batch_stride
from mfma_fwd_ref import (bf16_image, bf16_references, contract_bound, conv_weight, hi16, int_inputs, rms, split3, stored_weight, x3_image)
from mfma_fwd_rows import (BF16, DIRECT, KERNELS, LADDER, LEFT_OUT, N, REACHABLE, ROWS, S, U, WINO, X3, bf16_eligible, cin, exact,
                           expected_algo, expected_instantiation, kernel_name, nchunks, out_size, src0_bstride, x3_eligible)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [r["name"] for r in ROWS]
XROWS = [r for r in ROWS if r["kernel"] == X3]
BROWS = [r for r in ROWS if r["kernel"] == BF16]
E_BADARG = -1


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "instancediff_amd", "csrc"), "-j", "4"], check=True)
    return _lib.load()


def test_row_names_are_unique():
    names = IDS + [r["name"] for r in LADDER]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_claim_follows_from_the_rule_and_the_row_is_eligible(row):
    assert row["claim"] == expected_instantiation(row), row["name"]
    assert row["claim"] in REACHABLE and row["claim"][0] == row["kernel"], row["name"]
    assert (x3_eligible(row) if row["kernel"] == X3 else bf16_eligible(row)), row["name"]
    assert expected_algo(row) == row["kernel"] == row["want"], row["name"]
    assert not (row["pro"] and row["C1"])
    if row["gn"]:
        assert row["Cout"] % row["gn"] == 0
    if row["stats"]:  # the statistics are compared with sums of the stored output: it must be conv + bias
        assert not (row["res"] or row["vec"] or row["aux"]), row["name"]


def test_rows_claim_every_reachable_instantiation():
    assert len(REACHABLE) == 14 and sum(1 for t in REACHABLE if t[0] == X3) == 8 and sum(1 for t in REACHABLE if t[0] == BF16) == 6
    claimed = {r["claim"] for r in ROWS}
    assert claimed == REACHABLE, sorted(REACHABLE - claimed)
    assert LEFT_OUT == {}
    assert {kernel_name(t) for t in REACHABLE} == {"conv1x1_x3_kernel<false>", "conv1x1_x3_kernel<true>", "conv_bf16_kernel<0>",
                                                   "conv_bf16_kernel<1>"}
    assert KERNELS == (X3, BF16)


def _octet_of_the_boundary(r):
    """(chunk, octet in the chunk) at which the second source of a two-source row begins"""
    return r["C0"] // 32, r["C0"] % 32 // 8


def test_table_covers_what_the_rows_are_for():
    # ---- bf16x3 ----
    nrm, uns = [r for r in XROWS if r["mode"] == N], [r for r in XROWS if r["mode"] == S]
    assert len(nrm) + len(uns) == len(XROWS)
    ch = {nchunks(r) for r in XROWS}
    assert {1, 2} <= ch and any(c >= 3 and c % 2 for c in ch) and any(c >= 4 and c % 2 == 0 for c in ch)
    assert {8, 16, 24} <= {cin(r) % 32 for r in XROWS}
    two = [r for r in nrm if r["C1"]]
    assert any((r["C0"], r["C1"]) == (8, 24) and nchunks(r) == 1 for r in two)      # the boundary in the first octet group of the only chunk
    later = [r for r in two if _octet_of_the_boundary(r)[0] >= 1 and _octet_of_the_boundary(r)[1] != 0]
    assert len(later) >= 2 and len({_octet_of_the_boundary(r) for r in later}) >= 2   # inside a later chunk at a non-zero octet
    assert {64, 128, 192} <= {r["Cout"] for r in XROWS}
    assert any(r["Cout"] >= 128 and (r["res"] or r["aux"]) and r["vec"] for r in XROWS)  # an epilogue error shows in block >= 1
    tiles = lambda r: out_size(r)[0] * out_size(r)[1] // 256  # noqa: E731
    assert any(tiles(r) >= 2 for r in nrm) and any(tiles(r) >= 2 for r in uns) and any(tiles(r) == 1 for r in XROWS)
    assert any(not r["bias"] for r in XROWS)
    for rows, roles in ((nrm, ("src0", "src1", "res", "aux", "out")), (uns, ("src0", "res", "out"))):
        assert any(r["vec"] for r in rows) and any(r["dc"] for r in rows)
        for name in roles:
            assert any(name in r["slices"] for r in rows), name
    assert any(r["C0"] == 8 and nchunks(r) == 1 for r in uns) and any(r["C0"] == 10 and cin(r) == 40 for r in uns)
    assert any((r["Hin"], r["Win"]) == (128, 8) and out_size(r)[1] == 4 for r in uns)     # a tile is 64 output rows
    assert any((r["Hin"], r["Win"]) == (128, 24) and 256 % out_size(r)[1] for r in uns)    # tiles 1 and 2 start mid-row
    assert any(r["transposed"] for r in nrm)
    for r in XROWS:  # the limits on the rows' sizes
        Hout, Wout = out_size(r)
        assert 256 <= Hout * Wout <= 768 and 64 <= r["Cout"] <= 192 and r["B"] in (2, 3), r["name"]
        if r["mode"] == N:
            assert Wout >= 32 and (Hout * Wout) % 256 == 0 and r["C0"] % 8 == 0, r["name"]
    assert sum(1 for r in XROWS if r["B"] == 3) == 1
    assert all(r["req"] == 1 + X3 and r["operands"] == 0 for r in XROWS)
    # ---- bf16 ----
    for m in (N, U):
        rows = [r for r in BROWS if r["mode"] == m]
        assert any(r["pro"] for r in rows) and any(r["C1"] for r in rows) and any(not r["pro"] and not r["C1"] for r in rows), m
    assert {(32, 0), (32, 32), (64, 32)} <= {(r["C0"], r["C1"]) for r in BROWS}
    assert {64, 128} == {r["Cout"] for r in BROWS}
    assert {(8, 32), (16, 64)} == {out_size(r) for r in BROWS}
    assert sum(1 for r in BROWS if r["B"] == 3) == 1
    for name in ("src0", "src1", "res", "aux", "out"):
        assert any(name in r["slices"] for r in BROWS), name
    assert any("src0" in r["odd"] for r in BROWS) and any(not r["bias"] for r in BROWS)
    assert any(r["stats"] and not r["gn"] for r in BROWS) and sum(1 for r in BROWS if r["gn"]) == 1
    tr = [r for r in BROWS if r["transposed"]]
    assert len(tr) == 1 and cin(tr[0]) % 32 == 0 and tr[0]["Cout"] % 64 == 0
    assert all(r["C0"] >= 64 for r in BROWS if r["pro"])
    assert all(r["req"] == 0 and r["operands"] == 1 for r in BROWS)
    assert sum(1 for r in ROWS if exact(r)) >= 16


def test_eligibility_rules_at_their_edges():
    """the restated rules on variations of one row each: what each kernel refuses"""
    base = next(r for r in ROWS if r["name"] == "x3-n00-8x32-C32-one-chunk-Cout64-plain")
    v = lambda **kw: dict(base, **kw)  # noqa: E731
    assert x3_eligible(base) and x3_eligible(v(C0=40)) and x3_eligible(v(C0=8, C1=24))
    for kw in (dict(C0=24), dict(C0=36), dict(C0=12, C1=20), dict(Cout=96), dict(Cout=32), dict(Hin=16, Win=16), dict(Hin=9), dict(pro=True),
               dict(stats=True), dict(odd=("src0",)), dict(odd=("wpk",)), dict(bs0_plus=2), dict(image=False), dict(ks=3)):
        assert not x3_eligible(v(**kw)), kw
    ub = next(r for r in ROWS if r["name"] == "x3-s00-16x64-C8-one-chunk-Cout64-plain")
    u = lambda **kw: dict(ub, **kw)  # noqa: E731
    assert x3_eligible(ub) and x3_eligible(u(C0=10)) and x3_eligible(u(odd=("wpk",)))   # no flattening rule in unshuffle mode
    for kw in (dict(C0=9), dict(C0=4), dict(Hin=18), dict(Hin=256, Win=12), dict(odd=("src0",)), dict(bs0_plus=2), dict(pro=True)):
        assert not x3_eligible(u(**kw)), kw
    bb = next(r for r in ROWS if r["name"] == "bf-n00-8x32-C32-one-chunk-Cout64-plain")
    b = lambda **kw: dict(bb, **kw)  # noqa: E731
    assert bf16_eligible(bb) and bf16_eligible(b(odd=("src0",))) and bf16_eligible(b(mode=U, Hin=4, Win=16, C1=32))
    for kw in (dict(C0=16, C1=48), dict(C0=48), dict(Cout=96), dict(Hin=12), dict(Win=48), dict(image=False), dict(ks=1)):
        assert not bf16_eligible(b(**kw)), kw


def test_ladder_wants_follow_from_the_rule():
    for c in LADDER:
        assert expected_algo(c) == c["want"], c["name"]
    wants = [c["want"] for c in LADDER]
    assert {X3, BF16, DIRECT, WINO, None} == set(wants) and wants.count(None) >= 6


# ---- idiff_conv2d_plan on made-up addresses -------------------------------------------------------------------------------------------
def _fake_desc(row):
    """the row's idiff_conv_desc over operands that do not exist: every pointer a distinct 16-byte-aligned address plus the row's offset"""
    base = iter(range(0x10000000, 0x70000000, 0x04000000))
    Hout, Wout = out_size(row)
    pin, pout = row["Hin"] * row["Win"], Hout * Wout
    addr = lambda name, plane: next(base) + 4 * _float_offset(row, name, plane)  # noqa: E731
    d = ConvDesc()
    d.src0, d.src0_bstride, d.C0 = addr("src0", pin), src0_bstride(row), row["C0"]
    if row["C1"]:
        d.src1, d.src1_bstride, d.C1 = addr("src1", pin), batch_stride(row, "src1", row["C1"], pin), row["C1"]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = row["B"], row["Hin"], row["Win"], row["mode"], row["ks"], row["Cout"]
    d.wpk = next(base) + (4 if "wpk" in row["odd"] else 0)
    if row["ks"] == 3:
        d.wwino, d.wwino4 = next(base), next(base)
    if row["image"]:
        if row["ks"] == 1:
            d.wx3 = next(base)
        else:
            d.wbf16 = next(base)
    if row["bias"]:
        d.bias = next(base)
    if row["pro"]:
        d.pro_a, d.pro_b = next(base), next(base)
    d.out, d.out_bstride = addr("out", pout), batch_stride(row, "out", row["Cout"], pout)
    if row["res"]:
        d.res, d.res_bstride = addr("res", pout), batch_stride(row, "res", row["Cout"], pout)
    if row["vec"]:
        d.vec = next(base)
    if row["aux"]:
        d.aux, d.aux_bstride, d.aux_a, d.aux_b = addr("aux", pout), batch_stride(row, "aux", row["Cout"], pout), next(base), next(base)
    if row["stats"]:
        d.stats = next(base)
    d.algo_request, d.operands = row["req"], row["operands"]
    return d


@pytest.mark.parametrize("row", ROWS + LADDER, ids=IDS + [c["name"] for c in LADDER])
def test_plan_answers_the_rule(built_lib, row):
    keep = built_lib.idiff_conv2d_last_algo()
    got = built_lib.idiff_conv2d_plan(ctypes.byref(_fake_desc(row)))
    want = expected_algo(row)
    assert got == (E_BADARG if want is None else want), (row["name"], got, want, built_lib.idiff_last_error())
    assert want == row["want"]
    assert built_lib.idiff_conv2d_last_algo() == keep  # a plan is no launch


# ---- the split and the weight images ------------------------------------------------------------------------------------------------
def _wide(shape, seed):
    """fp32 values whose magnitudes span 2^-60 .. 2^60"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp2(torch.randint(-60, 61, shape, generator=g).float())


def test_split_is_exact():
    x = _wide((1 << 20,), 1)
    p1, p2, p3 = split3(x)
    assert torch.equal(p1.double() + p2.double() + p3.double(), x.double())
    for p in (p1, p2, p3):  # each plane is a bf16 value
        assert torch.equal(hi16(p), p) and torch.equal(p.to(torch.bfloat16).float(), p)
    nz = x != 0
    assert bool((p2.abs()[nz] <= x.abs()[nz] * 2.0 ** -7).all()) and bool((p3.abs()[nz] <= x.abs()[nz] * 2.0 ** -15).all())
    # exponent-blind: scaling by a power of two scales every plane (values of order one: 2^-40 of their last plane is still normal)
    y = torch.randn(1 << 16, generator=torch.Generator().manual_seed(2))
    for s in (2.0 ** 40, 2.0 ** -40):
        for p, q in zip(split3(y * s), split3(y)):
            assert torch.equal(p, q * s)
    # an integer in [-2, 2] is its own first plane
    i = torch.arange(-2, 3).float()
    q1, q2, q3 = split3(i)
    assert torch.equal(q1, i) and not q2.any() and not q3.any()


@pytest.mark.parametrize("Cout,Cin", [(64, 32), (128, 40), (192, 104)])
def test_x3_image_layout(Cout, Cin):
    w = _wide((Cout, Cin), 2 + Cin)
    img = x3_image(w)
    ncc, ncob = -(-Cin // 32), Cout // 64
    assert img.dtype == torch.int16 and img.numel() == ncc * ncob * 3 * 4 * 64 * 8
    v = img.view(ncc, ncob, 3, 4, 64, 8)
    # the image read back by plain indexing: the three planes of element (co, ci) sum to it; zero beyond Cin
    back = (v.to(torch.int32) << 16).view(torch.float32).double().sum(2)  # [chunk][block][octet][co][8]
    full = back.permute(1, 3, 0, 2, 4).reshape(ncob * 64, ncc * 32)
    assert torch.equal(full[:, :Cin], w.double()) and not full[:, Cin:].any()
    assert not v.permute(0, 3, 5, 1, 2, 4).reshape(ncc * 32, -1)[Cin:].any()  # every plane, not only their sum
    co, ci = Cout - 3, Cin - 5
    p = [v[ci // 32, co // 64, k, ci % 32 // 8, co % 64, ci % 8] for k in range(3)]
    assert [int(t) for t in p] == [int(s.view(torch.int32) >> 16) for s in split3(w[co, ci].reshape(1))]


@pytest.mark.parametrize("transpose", [False, True])
def test_bf16_image_layout(transpose):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((96, 64, 3, 3) if transpose else (64, 96, 3, 3), generator=g)  # the conv is 96 -> 64 either way
    img = bf16_image(w, transpose)
    assert img.numel() == 3 * 1 * 9 * 4 * 64 * 8
    v = img.view(3, 1, 9, 4, 64, 8).view(torch.bfloat16).float()
    wc = conv_weight(w, transpose)
    assert tuple(wc.shape) == (64, 96, 3, 3)
    back = v[:, 0].permute(3, 0, 2, 4, 1).reshape(64, 96, 9)  # [co][chunk, octet, j][tap]
    assert torch.equal(back, wc.reshape(64, 96, 9).to(torch.bfloat16).float())
    if transpose:  # the data gradient: conv2d with the transposed image is conv_transpose2d with the stored weight
        dy = torch.randn(1, 96, 5, 7, generator=g, dtype=torch.float64)
        assert torch.allclose(F.conv2d(dy, wc.double(), padding=1), F.conv_transpose2d(dy, w.double(), padding=1), rtol=0, atol=1e-12)


# ---- references ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_reference_is_computable_and_not_degenerate(row):
    inp = make_inputs(row, 5000 + IDS.index(row["name"]))
    out, raw = reference(row, inp)
    Hout, Wout = out_size(row)
    assert out.dtype == torch.float64 and tuple(out.shape) == (row["B"], row["Cout"], Hout, Wout)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1 and float(raw.abs().max()) > 0.1
    assert tuple(inp["w"].shape) == (row["Cout"], cin(row), row["ks"], row["ks"])
    ws = stored_weight(row, inp)
    assert tuple(ws.shape[:2]) == ((cin(row), row["Cout"]) if row["transposed"] else (row["Cout"], cin(row)))
    if row["kernel"] == X3 and row["transposed"]:  # the fp64 product with the stored matrix transposed
        x = inp["src0"].double()
        ref = torch.einsum("oc,bchw->bohw", ws.reshape(cin(row), row["Cout"]).t().double(), x) + inp["bias"].double()[None, :, None, None]
        assert float((ref - raw).abs().max()) < 1e-12
    if row["kernel"] == BF16:
        refs = bf16_references(row, inp)
        assert float((refs["ref_f64"] - out).abs().max()) < 1e-12 * float(out.abs().max())  # the contract's reference is the row's
        rnd = rms(refs["ref_bf16"] - refs["ref_f64"])
        assert 1e-4 * rms(out) < rnd < 1e-2 * rms(out), (row["name"], rnd)                   # the rounding is there to be measured
        if row["pro"]:  # the rounded reference itself satisfies the rigorous bound against the unrounded one
            ref, bound = contract_bound(row, refs)
            assert ref is refs["ref_f64"] and bool(((refs["ref_bf16"] - ref).abs() <= bound).all()), row["name"]


@pytest.mark.parametrize("row", [r for r in ROWS if exact(r)], ids=[r["name"] for r in ROWS if exact(r)])
def test_exact_rows_are_exact_in_fp32(row):
    inp = int_inputs(row, 6000 + IDS.index(row["name"]))
    out, raw = reference(row, inp)
    assert float(out.abs().max()) <= 4 * cin(row) * row["ks"] ** 2 + 6 < 2 ** 24 and torch.equal(out, out.round())
    assert torch.equal(out.float().double(), out) and float(out.abs().max()) > 8
    p1, p2, p3 = split3(inp["src0"])
    assert torch.equal(p1, inp["src0"]) and not p2.any() and not p3.any()
    assert torch.equal(inp["w"].to(torch.bfloat16).float(), inp["w"])
    if row["stats"]:  # every partial sum of the statistics is an integer below 2^24
        st = tile_stats(raw)
        assert float(tile_stats(raw.abs())[..., 0].max()) < 2 ** 24 and float(st[..., 1].max()) < 2 ** 24
        assert torch.equal(st.float().double(), st)
