"""The two forward convolution kernels on the bf16 matrix cores -- conv1x1_x3_kernel<UNSH> (csrc/conv1x1_x3.hip, IDIFF_CONV_ALGO_X3,
its epilogue compiled per (RES, AUX)) and conv_bf16_kernel<MODE> (csrc/conv_bf16.hip, IDIFF_CONV_ALGO_BF16, opt-in) -- one table row
per launch branch (mfma_fwd_rows.ROWS: 14 of 14, mirrored without a GPU by test_mfma_fwd_cpu.py), the properties of the three-way
split, the two weight packers byte for byte, and the selection ladder that leads to the kernels, in the style of
test_wino_fwd_gpu.py.

Every row runs the HIP kernel through ops.conv2d (bf16x3: asked for by name; bf16: operands="bf16"); idiff_conv2d_plan on the same
descriptor before the launch and idiff_conv2d_last_algo() after it must both name the kernel.  The reference is a plain torch float64
evaluation on the CPU of the formula written in conv_branch_ref.py -- never another kernel of this library.  Every operand that is
written lies inside a sentinel-filled buffer that must be bit-intact around it afterwards; sources, residual, aux and output are
channel slices of wider buffers where the row says so.

Bounds (none chosen from what the kernels return):
  bf16x3 vs fp64   the project's 2e-6 of the output range (_conv_tol of test_ops_gpu.py); rows with DC inputs or an aux term take
                   max(that, 4 x the fp32-on-the-CPU error of the same formula), both numbers printed; the last channel block and the
                   last 256-pixel tile are also checked element by element
  bf16, no prologue  |got - ref_bf16| <= 5e-5 conv(|X~|,|W~|) + 4e-7 |ref_bf16| and rms(got - ref_bf16) <= 0.05 rms(ref_bf16 - ref_f64)
                   (test_conv_bf16_gpu._contract_checks)
  bf16, prologue   |got - ref_f64| <= 2^-8 conv(|X|,|W|) + 4e-7 |ref_f64| (silu_fast may flip a rounding: mfma_fwd_ref.contract_bound)
                   and the same rms rule
  statistics       against float64 sums of the stored output of the same call (rows with statistics add nothing but the bias):
                   1e-5 of the sum of magnitudes (test_conv_bf16_gpu), per tile and in total; the finalize outputs against
                   conv_branch_ref.gn_affine of that stored output at the project's 1e-5 (floored by its fp32 evaluation)
  exact rows, scaling, containment, packer bytes   equality"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops  # noqa: E402
from instancediff_amd._lib import ConvDesc  # noqa: E402
from instancediff_amd.ops import _bs, _stream  # noqa: E402

from conv_branch_ref import gn_affine, make_inputs, reference, tile_stats  # noqa: E402
from conv_guard_util import DEV, SENT, _buf, _check, _floor, _guard_intact, _pad, _rel  # noqa: E402
from mfma_fwd_ref import bf16_image, bf16_references, contract_bound, int_inputs, rms, stored_weight, x3_image  # noqa: E402
from mfma_fwd_rows import (BF16, DIRECT, LADDER, N, ROWS, S, WINO, X3, _float_offset, _row, batch_stride, exact, expected_algo,  # noqa: E402
                           expected_instantiation, out_size, src0_bstride)

E_BADARG = -1
TOL_ALGO = {DIRECT: 2e-6, WINO: 6e-6, X3: 2e-6}  # TOL_ALGO of test_conv_branches_gpu.py
TOL_SUM = 1e-5
IDS = [r["name"] for r in ROWS]
XROWS = [r for r in ROWS if r["kernel"] == X3]
BROWS = [r for r in ROWS if r["kernel"] == BF16]
EXACT = [r for r in ROWS if exact(r)]


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _strided(shape, bstride, src):
    """a [B, C, H, W] device tensor with batch stride `bstride` floats inside sentinels"""
    B, C, H, W = shape
    flat = torch.full((B * bstride + 8,), SENT, device=DEV, dtype=torch.float32)
    view = flat.as_strided(shape, (bstride, H * W, W, 1), 0)
    view.copy_(src)
    return view


def _pack_x3(w2d):
    """(flat, image): idiff_pack_conv1x1_x3 of a [Cout, Cin] matrix into an int16 buffer with a guard band on either side"""
    lib = _lib.load()
    Cout, Cin = w2d.shape
    n = lib.idiff_conv1x1_x3_image_bytes(Cout, Cin) // 2
    flat = torch.full((n + 64,), 0x5A5A, device=DEV, dtype=torch.int16)
    img = flat[32:32 + n]
    assert img.data_ptr() % 16 == 0
    _lib.check(lib.idiff_pack_conv1x1_x3(w2d.to(DEV).contiguous().data_ptr(), img.data_ptr(), Cout, Cin, _stream()), "pack_conv1x1_x3")
    torch.cuda.synchronize()
    return flat, img


def _operands(row, inp):
    """device operands of a row: (t, guards).  out, the statistics and the finalize outputs are always inside sentinel buffers"""
    lib = _lib.load()
    sl, odd = row["slices"], row["odd"]
    for k in list(sl) + list(odd):
        assert k in ("src0", "src1", "res", "aux", "out", "wpk"), k
    B, Cout, ks = row["B"], row["Cout"], row["ks"]
    Hout, Wout = out_size(row)
    plane = row["Hin"] * row["Win"]
    if row["bs0_plus"]:
        t = dict(x0=_strided(tuple(inp["src0"].shape), row["C0"] * plane + row["bs0_plus"], inp["src0"]))
    else:
        t = dict(x0=_buf(inp["src0"].shape, sl.get("src0", 0), "src0" in odd, inp["src0"])[1])
    assert _bs(t["x0"]) == src0_bstride(row)
    assert (t["x0"].data_ptr() % 16 == 0) == (_float_offset(row, "src0", plane) % 4 == 0)
    if row["C1"]:
        t["x1"] = _buf(inp["src1"].shape, sl.get("src1", 0), "src1" in odd, inp["src1"])[1]
        assert _bs(t["x1"]) == batch_stride(row, "src1", row["C1"], plane)
    w = stored_weight(row, inp).to(DEV).contiguous()
    wpk = ops.pack_conv_weight(w, transpose=row["transposed"], bf16=(ks == 3 and row["image"]))
    images = {k: getattr(wpk, k) for k in ("wino", "wino4", "x3", "bf16") if hasattr(wpk, k)}
    if ks == 1:
        if not row["image"]:
            images.pop("x3", None)
        elif "x3" not in images:  # a shape pack_conv_weight builds no split image for: the descriptor still carries one
            assert not row["transposed"]
            images["x3"] = _pack_x3(inp["w"].reshape(Cout, -1))[1]
    if "wpk" in odd:
        wflat = torch.zeros((wpk.numel() + 8,), device=DEV, dtype=torch.float32)
        wv = wflat[1:1 + wpk.numel()].view(wpk.shape)
        wv.copy_(wpk)
        wpk = wv
    else:
        wpk = wpk.clone()  # a plain tensor: the images travel in t["images"]
    assert (wpk.data_ptr() % 16 == 0) == ("wpk" not in odd)
    t["wpk"], t["images"] = wpk, images
    assert (ks == 1 and row["image"]) == ("x3" in images and ks == 1) and (ks == 3 and row["image"]) == ("bf16" in images)
    t["bias"] = None if inp["bias"] is None else inp["bias"].to(DEV)
    if row["pro"]:
        t["pro"] = tuple(v.to(DEV) for v in inp["pro"])
    if row["res"]:
        t["res"] = _buf(inp["res"].shape, sl.get("res", 0), "res" in odd, inp["res"])[1]
    if row["vec"]:
        t["vec"] = inp["vec"].to(DEV)
    if row["aux"]:
        a, aa, ab = inp["aux"]
        t["aux"] = (_buf(a.shape, sl.get("aux", 0), "aux" in odd, a)[1], aa.to(DEV), ab.to(DEV))
    oflat, t["out"] = _buf((B, Cout, Hout, Wout), sl.get("out", 0), "out" in odd)
    guards = [(oflat, t["out"], "out")]
    if row["stats"]:
        nt = lib.idiff_conv2d_num_tiles(Hout, Wout)
        sflat, t["stats"] = _pad((B, nt, Cout, 2))
        guards.append((sflat, t["stats"], "stats"))
    if row["gn"]:
        (fa, ga), (fb, gb) = _pad((B, Cout)), _pad((B, Cout))
        t["gn"] = dict(groups=row["gn"], gamma=inp["gamma"].to(DEV), beta=inp["beta"].to(DEV), a=ga, b=gb)
        guards += [(fa, ga, "gn a"), (fb, gb, "gn b")]
    return t, guards


def _weight(t):
    """the packed weight as ops.conv2d takes it: the direct image with the other images as attributes"""
    wpk = t["wpk"]
    for k, v in t["images"].items():
        setattr(wpk, k, v)
    return wpk


def _desc(row, t):
    """the idiff_conv_desc of a row's call over the device operands `t`, as ops.conv2d fills it"""
    d = ConvDesc()
    x0, out, im = t["x0"], t["out"], t["images"]
    d.src0, d.src0_bstride, d.C0 = x0.data_ptr(), _bs(x0), x0.shape[1]
    if t.get("x1") is not None:
        d.src1, d.src1_bstride, d.C1 = t["x1"].data_ptr(), _bs(t["x1"]), t["x1"].shape[1]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = x0.shape[0], x0.shape[2], x0.shape[3], row["mode"], row["ks"], row["Cout"]
    d.wpk = t["wpk"].data_ptr()
    if row["ks"] == 3 and "wino" in im:
        d.wwino = im["wino"].data_ptr()
        if "wino4" in im:
            d.wwino4 = im["wino4"].data_ptr()
    if row["ks"] == 1 and "x3" in im:
        d.wx3 = im["x3"].data_ptr()
    if row["ks"] == 3 and "bf16" in im:
        d.wbf16 = im["bf16"].data_ptr()
    if t["bias"] is not None:
        d.bias = t["bias"].data_ptr()
    if t.get("pro") is not None:
        d.pro_a, d.pro_b = (v.data_ptr() for v in t["pro"])
    d.out, d.out_bstride = out.data_ptr(), _bs(out)
    if t.get("res") is not None:
        d.res, d.res_bstride = t["res"].data_ptr(), _bs(t["res"])
    if t.get("vec") is not None:
        d.vec = t["vec"].data_ptr()
    if t.get("aux") is not None:
        a, aa, ab = t["aux"]
        d.aux, d.aux_bstride, d.aux_a, d.aux_b = a.data_ptr(), _bs(a), aa.data_ptr(), ab.data_ptr()
    if t.get("stats") is not None:
        d.stats = t["stats"].data_ptr()
    if t.get("gn") is not None:
        g = t["gn"]
        d.gn_groups, d.gn_eps, d.gn_gamma, d.gn_beta = g["groups"], 1e-5, g["gamma"].data_ptr(), g["beta"].data_ptr()
        d.gn_out_a, d.gn_out_b = g["a"].data_ptr(), g["b"].data_ptr()
    d.algo_request, d.operands = row["req"], row["operands"]
    return d


def _plan_and_run(row, t):
    """idiff_conv2d_plan on the row's descriptor names the kernel; ops.conv2d launches it; idiff_conv2d_last_algo() names it again"""
    lib = _lib.load()
    kernel = row["kernel"]
    assert ops.X3, "the kernels are tested at the process-wide switches' defaults"
    planned = lib.idiff_conv2d_plan(ctypes.byref(_desc(row, t)))
    assert planned == kernel, (row["name"], planned, lib.idiff_last_error())
    kw = dict(src1=t.get("x1"), mode=row["mode"], out=t["out"], pro=t.get("pro"), res=t.get("res"), vec=t.get("vec"), aux=t.get("aux"))
    if kernel == X3:
        kw["algo"] = ops.CONV_ALGO_X3
    else:
        kw["operands"] = "bf16"
    if row["gn"]:
        g = t["gn"]
        kw["gn"] = dict(groups=g["groups"], gamma=g["gamma"], beta=g["beta"], bufs=[t["stats"], g["a"], g["b"]])
    got = ops.conv2d(t["x0"], _weight(t), t["bias"], row["ks"], row["Cout"], want_stats=row["stats"], **kw)
    torch.cuda.synchronize()
    assert lib.idiff_conv2d_last_algo() == kernel, (row["name"], lib.idiff_conv2d_last_algo())
    stats = None
    if row["gn"]:
        got, gnab, stats = got
        assert gnab[0].data_ptr() == t["gn"]["a"].data_ptr() and stats.data_ptr() == t["stats"].data_ptr()
    elif row["stats"]:
        got, stats = got  # ops.conv2d places the statistics itself unless a finalize rides along
    assert got.data_ptr() == t["out"].data_ptr()
    return stats


def _guards(name, guards, stats_placed=True):
    for flat, view, what in guards:
        if what == "stats" and not stats_placed:
            assert bool((flat == SENT).all())  # this call's statistics went to a tensor of ops.conv2d's own
            continue
        _guard_intact(flat, view, f"{name} {what}")


# ---- 1. the bf16x3 table ------------------------------------------------------------------------------------------------------------
def _x3_tails(row):
    """the last channel block and the last 256-pixel tile of [B, Cout, Hout * Wout]"""
    Hout, Wout = out_size(row)
    every = slice(None)
    return [("last channel block", (every, slice(row["Cout"] - 64, None))), ("last tile", (every, every, slice(Hout * Wout - 256, None)))]


def _flat3(v):
    return v.reshape(v.shape[0], v.shape[1], -1)


@pytest.mark.parametrize("row", XROWS, ids=[r["name"] for r in XROWS])
def test_bf16x3_branch(row):
    name = row["name"]
    assert row["claim"] == expected_instantiation(row) and expected_algo(row) == X3
    inp = make_inputs(row, 5000 + IDS.index(name))
    t, guards = _operands(row, inp)
    _plan_and_run(row, t)
    ref, _ = reference(row, inp)
    tol = TOL_ALGO[X3]
    if row["dc"] or row["aux"]:
        tol = _floor(tol, reference(row, inp, torch.float32)[0], ref)
    _check(name, "out", _flat3(t["out"]), _flat3(ref), tol, _x3_tails(row), base=TOL_ALGO[X3])
    _guards(name, guards)


# ---- 2. the bf16 table --------------------------------------------------------------------------------------------------------------
def _contract(name, row, inp, got):
    """the rounding contract of a bf16 launch (mfma_fwd_ref.contract_bound) and the rms rule; prints the figures"""
    refs = bf16_references(row, inp)
    got = got.detach().double().cpu()
    ref, bound = contract_bound(row, refs)
    err = (got - ref).abs()
    rms_err, rms_rnd = rms(got - refs["ref_bf16"]), rms(refs["ref_bf16"] - refs["ref_f64"])
    print(f"{name} out: rel {_rel(got, refs['ref_f64']):.2e} vs fp64, {_rel(got, refs['ref_bf16']):.2e} vs bf16-rounded fp64; worst "
          f"error / bound {float((err / bound).max()):.3f} ({'2^-8, unrounded' if row['pro'] else '5e-5, rounded'}); rms {rms_err:.2e} "
          f"of the rounding's {rms_rnd:.2e} ({rms_err / rms_rnd:.4f}, limit 0.05)")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (name, float((err / bound).max()))
    assert rms_err <= 0.05 * rms_rnd, (name, rms_err, rms_rnd)


def _stats_of_the_stored_output(name, row, inp, t, stats):
    """tile statistics and finalize outputs against float64 sums of the launch's own stored output (= conv + bias on these rows).
    test_conv_bf16_gpu.py holds the totals to 1e-5 of the sum of magnitudes; a tile is held to the same figure: its 256 values pass
    through a chain of four, a 16-lane butterfly and a sum over four waves, at most 11 fp32 roundings = 7e-7 of the magnitudes"""
    assert not (row["res"] or row["vec"] or row["aux"])
    y = t["out"].detach().double().cpu()
    st, sa = tile_stats(y), tile_stats(y.abs())
    s = stats.detach().double().cpu()
    assert tuple(s.shape) == tuple(st.shape), (s.shape, st.shape)
    for what, got, ref, mag in (("per tile", s, st, sa), ("total", s.sum(1), st.sum(1), sa.sum(1))):
        e0, e1 = (got[..., 0] - ref[..., 0]).abs(), (got[..., 1] - ref[..., 1]).abs()
        r0, r1 = float((e0 / mag[..., 0]).max()), float((e1 / ref[..., 1]).max())
        print(f"{name} stats {what}: sum {r0:.2e} of the magnitudes, sumsq {r1:.2e} (limit 1e-5)")
        assert bool((e0 <= 1e-5 * mag[..., 0] + 1e-6).all()) and bool((e1 <= 1e-5 * ref[..., 1] + 1e-6).all()), (name, what)
    if row["gn"]:
        a, b = gn_affine(y, row["gn"], inp["gamma"], inp["beta"])
        a32, b32 = gn_affine(y.float(), row["gn"], inp["gamma"], inp["beta"])
        _check(name, "gn a", t["gn"]["a"], a, _floor(TOL_SUM, a32, a), base=TOL_SUM)
        _check(name, "gn b", t["gn"]["b"], b, _floor(TOL_SUM, b32, b), base=TOL_SUM)


@pytest.mark.parametrize("row", BROWS, ids=[r["name"] for r in BROWS])
def test_bf16_branch(row):
    name = row["name"]
    assert row["claim"] == expected_instantiation(row) and expected_algo(row) == BF16
    inp = make_inputs(row, 5000 + IDS.index(name))
    t, guards = _operands(row, inp)
    stats = _plan_and_run(row, t)
    _contract(name, row, inp, t["out"])
    _guards(name, guards, stats_placed=bool(row["gn"]))
    if row["stats"]:
        _stats_of_the_stored_output(name, row, inp, t, stats)


# ---- 3. exact rows: integer operands, no tolerance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", EXACT, ids=[r["name"] for r in EXACT])
def test_exact_integer_row(row):
    """operands in [-2, 2]: every value is its own first bf16 plane (and its own bf16 rounding), every sum is exact in fp32 -- the
    result equals the fp64 reference bit for bit, which pins every index of the staging, the fragment order and the epilogue"""
    name = row["name"]
    row = dict(row, gn=0, dc=False)
    inp = int_inputs(row, 6000 + IDS.index(name))
    t, guards = _operands(row, inp)
    stats = _plan_and_run(row, t)
    ref, raw = reference(row, inp)
    got = t["out"].cpu()
    bad = (got != ref.float()).nonzero()
    assert torch.equal(got, ref.float()), f"{name}: {len(bad)} elements differ, the first at {bad[0].tolist()}"
    _guards(name, guards, stats_placed=False)
    if row["stats"]:
        st = tile_stats(raw)
        assert float(tile_stats(raw.abs())[..., 0].max()) < 2 ** 24 and float(st[..., 1].max()) < 2 ** 24
        assert torch.equal(stats.cpu(), st.float()), f"{name}: tile statistics of integer sums differ"


# ---- 4. properties of the split -------------------------------------------------------------------------------------------------------
def _p(name, mode, C0, Cout, Hin, Win):
    return _row(name, X3, 1, mode, C0, 0, Cout, Hin, Win, (X3, int(mode == S), 0, 0), req=1 + X3, want=X3, bias=False)


# row, then the input element (b, c, y, x) the containment test poisons
PROP = [(_p("split-normal-C64-Cout64-8x32", N, 64, 64, 8, 32), (1, 37, 5, 19)),
        (_p("split-unshuffle-C16-Cout64-16x64", S, 16, 64, 16, 64), (1, 9, 11, 45))]


def _plain(row, x, wpk):
    out = ops.conv2d(x.to(DEV), wpk, None, 1, row["Cout"], mode=row["mode"], algo=ops.CONV_ALGO_X3)
    torch.cuda.synchronize()
    assert _lib.load().idiff_conv2d_last_algo() == X3
    return out.cpu()


@pytest.mark.parametrize("row,where", PROP, ids=[p[0]["name"] for p in PROP])
def test_split_scales_by_powers_of_two(row, where):
    """conv(x * 2^40) == conv(x) * 2^40 and the same for 2^-40, bit for bit: the split is exponent-blind and both runs stay far inside
    the normal range of fp32 and bf16"""
    assert expected_algo(row) == X3
    inp = make_inputs(row, 77)
    wpk = ops.pack_conv_weight(inp["w"].to(DEV))
    base = _plain(row, inp["src0"], wpk)
    ref, _ = reference(row, inp)
    _check(row["name"], "out", base, ref, TOL_ALGO[X3])
    for s in (2.0 ** 40, 2.0 ** -40):
        x = inp["src0"] * s
        assert torch.equal(x / s, inp["src0"]) and float(x.abs()[x != 0].min()) > 2.0 ** -80
        got = _plain(row, x, wpk)
        assert torch.equal(got, base * s), f"{row['name']}: scaling the input by {s:g} changes {int((got != base * s).sum())} results"


@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("row,where", PROP, ids=[p[0]["name"] for p in PROP])
def test_split_contains_non_finite_values(row, where, poison):
    """one non-finite input element: every output channel at its pixel of its sample is non-finite, every other output element keeps
    its bits (the training step's non-finite guard relies on it)"""
    inp = make_inputs(row, 78)
    wpk = ops.pack_conv_weight(inp["w"].to(DEV))
    base = _plain(row, inp["src0"], wpk)
    assert bool(torch.isfinite(base).all())
    b, c, y, x = where
    xin = inp["src0"].clone()
    xin[b, c, y, x] = poison
    got = _plain(row, xin, wpk)
    oy, ox = (y // 2, x // 2) if row["mode"] == S else (y, x)
    assert not bool(torch.isfinite(got[b, :, oy, ox]).any()), f"{row['name']}: finite results at the poisoned pixel"
    got[b, :, oy, ox] = base[b, :, oy, ox]
    assert torch.equal(got.view(torch.int32), base.view(torch.int32)), f"{row['name']}: the non-finite value spread to other pixels"


# ---- 5. the packers, byte for byte ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout,Cin", [(64, 32), (128, 40), (192, 104)])
def test_pack_x3_image_bytes(Cout, Cin):
    g = torch.Generator().manual_seed(Cout + Cin)
    w = torch.randn(Cout, Cin, generator=g) * torch.exp2(torch.randint(-60, 61, (Cout, Cin), generator=g).float())
    flat, img = _pack_x3(w)
    want = x3_image(w)
    assert img.numel() == want.numel() and torch.equal(img.cpu(), want)
    assert bool((flat[:32] == 0x5A5A).all()) and bool((flat[32 + img.numel():] == 0x5A5A).all()), "the packer wrote outside the image"
    ncc = -(-Cin // 32)
    assert not img.cpu().view(ncc, Cout // 64, 3, 4, 64, 8).permute(0, 3, 5, 1, 2, 4).reshape(ncc * 32, -1)[Cin:].any()  # zero beyond Cin


@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transposed"])
def test_pack_bf16_image_bytes(transpose):
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    w = torch.randn((96, 128, 3, 3) if transpose else (128, 96, 3, 3), generator=g)  # the conv is 96 -> 128 either way
    n = lib.idiff_conv_weight_bf16_bytes(w.shape[0], w.shape[1], int(transpose)) // 2
    flat = torch.full((n + 64,), 0x5A5A, device=DEV, dtype=torch.int16)
    img = flat[32:32 + n]
    _lib.check(lib.idiff_pack_conv_weight_bf16(w.to(DEV).data_ptr(), img.data_ptr(), w.shape[0], w.shape[1], int(transpose), _stream()), "pack")
    torch.cuda.synchronize()
    want = bf16_image(w, transpose)
    assert n == want.numel() and torch.equal(img.cpu(), want)
    assert bool((flat[:32] == 0x5A5A).all()) and bool((flat[32 + n:] == 0x5A5A).all()), "the packer wrote outside the image"


# ---- 6. the selection ladder, with real tensors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LADDER, ids=[c["name"] for c in LADDER])
def test_selection_ladder(case):
    lib = _lib.load()
    name, want = case["name"], case["want"]
    assert ops.WINOGRAD and ops.WINOGRAD4 and ops.X3, "the ladder is tested at the process-wide switches' defaults"
    assert expected_algo(case) == want
    inp = make_inputs(case, 7000 + [c["name"] for c in LADDER].index(name))
    t, guards = _operands(case, inp)
    d = _desc(case, t)
    planned = lib.idiff_conv2d_plan(ctypes.byref(d))
    rc = lib.idiff_conv2d_fwd(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    if want is None:
        assert planned == E_BADARG and rc == E_BADARG, (name, planned, rc)
        for flat, view, what in guards:
            assert bool((flat == SENT).all()), f"{name}: a refused call wrote to {what}"
        return
    assert rc == 0, (name, rc, lib.idiff_last_error())
    assert planned == want and lib.idiff_conv2d_last_algo() == want, (name, planned, lib.idiff_conv2d_last_algo(), want)
    if want == BF16:
        _contract(name, case, inp, t["out"])
    else:
        ref, _ = reference(case, inp)
        tol = TOL_ALGO[want]
        if case["pro"]:
            assert want == DIRECT
            tol = _floor(tol, reference(case, inp, torch.float32)[0], ref)
        _check(name, "out", t["out"], ref, tol, base=TOL_ALGO[want])
    _guards(name, guards)
    assert math.isfinite(float(t["out"].abs().max()))
