"""The three 3x3 Winograd forward kernels -- conv_wino_kernel (csrc/conv_wino.hip, F(2x2,3x3)), conv_wino4_kernel (csrc/conv_wino4.hip,
F(4x4,3x3), 16x32 items) and conv_wino4h_kernel (csrc/conv_wino4h.hip, F(4x4,3x3), half-patch items), each <MODE, SPEC, RAG> -- one
table row per launch branch (wino_fwd_rows.ROWS: 24 of 24 instantiations, mirrored without a GPU by test_wino_fwd_cpu.py), the
multi-item pipeline of their persistent workgroups at a batch derived from the device's CU count, and the edges of their eligibility
checks, in the style of test_conv_branches_gpu.py.

Every row runs the HIP kernel, asked for by name (a hard algo_request; idiff_conv2d_plan and idiff_conv2d_last_algo() must both name
it), and compares it with a plain torch float64 evaluation on the CPU of the formula written in conv_branch_ref.py.  No row's
reference is another kernel of this library.  Every operand that is written lies inside a sentinel-filled buffer that must be
bit-intact around it afterwards; sources, residual, aux and output are channel slices of wider buffers where the row says so.

Metric: max|got - ref| / max|ref| per output tensor; the last partial patch column, patch row and channel block and the one-pixel
border ring of the image are also checked element by element against tol * max|ref|.  Tolerances are the project's existing ones
(_conv_tol of test_ops_gpu.py): 6e-6 of the output range for F(2x2,3x3), 4e-5 for F(4x4,3x3); statistics totals 1e-5 / 4e-5, per
tile 2e-5 / 1e-4.  Rows whose inputs carry a DC offset or that run silu_fast (prologue, aux term) take max(that, 4 x the error of the
same Winograd form evaluated in fp32 torch on the CPU (winograd_form_ref.py) against the fp64 reference, on the row's own inputs);
both numbers are printed.  No bound was chosen from what the kernels return."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops  # noqa: E402
from instancediff_amd._lib import ConvDesc  # noqa: E402
from instancediff_amd.ops import _bs, _stream  # noqa: E402

from conv_branch_ref import gn_affine, make_inputs, reference, tile_stats  # noqa: E402
from conv_guard_util import DEV, SENT, _buf, _check, _floor, _guard_intact, _pad  # noqa: E402
from wino_fwd_rows import (N, PATCH, ROWS, U, WINO, WINO4, WINO4H, _float_offset, batch_stride, eligible, expected_instantiation,  # noqa: E402
                           out_size, stream_facts)
from winograd_form_ref import form_reference  # noqa: E402

E_BADARG = -1
DIRECT = 0
TOL_ALGO = {DIRECT: 2e-6, WINO: 6e-6, WINO4: 4e-5, WINO4H: 4e-5}  # _conv_tol of test_ops_gpu.py
TOL_SUM = {DIRECT: 1e-5, WINO: 1e-5, WINO4: 4e-5, WINO4H: 4e-5}
TOL_TILE = {DIRECT: 2e-5, WINO: 2e-5, WINO4: 1e-4, WINO4H: 1e-4}
FORM = {WINO: 2, WINO4: 4, WINO4H: 4}
IDS = [r["name"] for r in ROWS]
TABLE = [r for r in ROWS if not r["stream"]]
STREAM = [r for r in ROWS if r["stream"]]


def _num_cu():
    cu, wave = ctypes.c_int(0), ctypes.c_int(0)
    name = ctypes.create_string_buffer(64)
    assert _lib.load().idiff_device_info(ctypes.byref(cu), ctypes.byref(wave), name, 64) == 0
    return cu.value


def _call(row, t, req, b=None):
    """the idiff_conv_desc of a row over the device operands `t` (sample b alone when given), planned and launched with algo_request
    `req`: (plan's answer, the call's return code)"""
    lib = _lib.load()
    one = (lambda v: v) if b is None else (lambda v: None if v is None else v[b:b + 1])
    d = ConvDesc()
    x0, x1, out = one(t["x0"]), one(t.get("x1")), one(t["out"])
    d.src0, d.src0_bstride, d.C0 = x0.data_ptr(), _bs(t["x0"]), x0.shape[1]
    if x1 is not None:
        d.src1, d.src1_bstride, d.C1 = x1.data_ptr(), _bs(t["x1"]), x1.shape[1]
    d.B, d.Hin, d.Win, d.mode, d.ks, d.Cout = x0.shape[0], x0.shape[2], x0.shape[3], row["mode"], 3, row["Cout"]
    wpk = t["wpk"]
    d.wpk, d.wwino, d.wwino4 = wpk.data_ptr(), wpk.wino.data_ptr(), wpk.wino4.data_ptr()
    if t.get("bias") is not None:
        d.bias = t["bias"].data_ptr()
    if t.get("pro") is not None:
        d.pro_a, d.pro_b = (one(v).data_ptr() for v in t["pro"])
    d.out, d.out_bstride = out.data_ptr(), t.get("out_bs", None) or _bs(t["out"])
    if t.get("res") is not None:
        d.res, d.res_bstride = one(t["res"]).data_ptr(), _bs(t["res"])
    if t.get("vec") is not None:
        d.vec = one(t["vec"]).data_ptr()
    if t.get("aux") is not None:
        a, aa, ab = t["aux"]
        d.aux, d.aux_bstride, d.aux_a, d.aux_b = one(a).data_ptr(), t.get("aux_bs", None) or _bs(a), one(aa).data_ptr(), one(ab).data_ptr()
    if t.get("stats") is not None:
        d.stats = one(t["stats"]).data_ptr()
    if t.get("gn") is not None:
        g = t["gn"]
        d.gn_groups, d.gn_eps, d.gn_gamma, d.gn_beta = g["groups"], 1e-5, g["gamma"].data_ptr(), g["beta"].data_ptr()
        d.gn_out_a, d.gn_out_b = one(g["a"]).data_ptr(), one(g["b"]).data_ptr()
    d.algo_request = req
    planned = lib.idiff_conv2d_plan(ctypes.byref(d))
    rc = lib.idiff_conv2d_fwd(ctypes.byref(d), _stream())
    return planned, rc


def _operands(row, inp):
    """device operands of a row: (t, guards).  out, the statistics and the finalize outputs are always inside sentinel buffers"""
    lib = _lib.load()
    sl, odd = row["slices"], row["odd"]
    for k in list(sl) + list(odd):
        assert k in ("src0", "src1", "res", "aux", "out"), k
    B, Cout = row["B"], row["Cout"]
    Hout, Wout = out_size(row)
    t = dict(x0=_buf(inp["src0"].shape, sl.get("src0", 0), "src0" in odd, inp["src0"])[1])
    assert _bs(t["x0"]) == batch_stride(row, "src0", row["C0"], row["Hin"] * row["Win"])
    assert (t["x0"].data_ptr() % 16 == 0) == (_float_offset(row, "src0", row["Hin"] * row["Win"]) % 4 == 0)
    if row["C1"]:
        t["x1"] = _buf(inp["src1"].shape, sl.get("src1", 0), "src1" in odd, inp["src1"])[1]
    t["wpk"] = ops.pack_conv_weight(inp["w"].to(DEV))
    assert hasattr(t["wpk"], "wino") and hasattr(t["wpk"], "wino4")
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
        assert nt == -(-Hout // 8) * -(-Wout // 32)
        sflat, t["stats"] = _pad((B, nt, Cout, 2))
        guards.append((sflat, t["stats"], "stats"))
    if row["gn"]:
        (fa, ga), (fb, gb) = _pad((B, Cout)), _pad((B, Cout))
        t["gn"] = dict(groups=row["gn"], gamma=inp["gamma"].to(DEV), beta=inp["beta"].to(DEV), a=ga, b=gb)
        guards += [(fa, ga, "gn a"), (fb, gb, "gn b")]
    return t, guards


def _tails(row, kernel, Hout, Wout):
    """the last partial patch column, patch row and channel block of a row's output and the one-pixel border ring of the image (where
    a padding or prologue-mask error shows)"""
    TH, TW = PATCH[kernel] if kernel != DIRECT else (8, 32)
    every = slice(None)
    out = [("top row", (every, every, slice(0, 1))), ("bottom row", (every, every, slice(Hout - 1, Hout))),
           ("left column", (every, every, every, slice(0, 1))), ("right column", (every, every, every, slice(Wout - 1, Wout)))]
    if Wout % TW:
        out.append(("last patch column", (every, every, every, slice((Wout // TW) * TW, None))))
    if Hout % TH:
        out.append(("last patch row", (every, every, slice((Hout // TH) * TH, None))))
    if row["Cout"] % 64:
        out.append(("last channel block", (every, slice((row["Cout"] // 64) * 64, None))))
    return out


def _compare(row, kernel, inp, t, guards, sub=None):
    """out, statistics and finalize outputs of a launched row against fp64; `sub`: the samples the fp32 floor is taken on (all)"""
    name = row["name"]
    Hout, Wout = out_size(row)
    ref, raw = reference(row, inp)
    loose = row["dc"] or row["pro"] or row["aux"]
    pick = (lambda v: v) if sub is None else (lambda v: v[sub])
    tol, raw32 = TOL_ALGO[kernel], None
    if loose:
        if sub is not None:
            inp_s = {k: (None if v is None else tuple(pick(x) for x in v) if isinstance(v, tuple) else v if k in ("w", "bias", "gamma", "beta")
                         else pick(v)) for k, v in inp.items()}
        else:
            inp_s = inp
        if kernel == DIRECT:
            ref32, raw32 = reference(row, inp_s, torch.float32)
        else:
            ref32, raw32 = form_reference(row, inp_s, FORM[kernel], torch.float32)
        tol = _floor(TOL_ALGO[kernel], ref32, pick(ref))
    _check(name, "out", t["out"], ref, tol, _tails(row, kernel, Hout, Wout), base=TOL_ALGO[kernel])
    for flat, view, what in guards:
        _guard_intact(flat, view, f"{name} {what}")
    if row["stats"]:
        st = tile_stats(raw)
        s = t["stats"].double().cpu()
        assert tuple(s.shape) == tuple(st.shape), (s.shape, st.shape)
        for w, what in ((0, "sum"), (1, "sumsq")):
            tsum, ttile = TOL_SUM[kernel], TOL_TILE[kernel]
            if row["dc"] or row["pro"]:
                st32, sts = tile_stats(raw32), pick(st)
                tsum, ttile = _floor(tsum, st32.sum(1)[..., w], sts.sum(1)[..., w]), _floor(ttile, st32[..., w], sts[..., w])
            _check(name, f"stats {what} total", s.sum(1)[..., w], st.sum(1)[..., w], tsum, base=TOL_SUM[kernel])
            _check(name, f"stats {what} per tile", s[..., w], st[..., w], ttile, base=TOL_TILE[kernel])
    if row["gn"]:
        a, b = gn_affine(raw, row["gn"], inp["gamma"], inp["beta"])
        a32, b32 = gn_affine(raw32 if raw32 is not None else raw.float(), row["gn"], inp["gamma"], inp["beta"])
        _check(name, "gn a", t["gn"]["a"], a, _floor(TOL_SUM[kernel], a32, a), base=TOL_SUM[kernel])
        _check(name, "gn b", t["gn"]["b"], b, _floor(TOL_SUM[kernel], b32, b), base=TOL_SUM[kernel])


def _written(t):
    return [t["out"]] + [t[k] for k in ("stats",) if t.get(k) is not None] + ([t["gn"]["a"], t["gn"]["b"]] if t.get("gn") else [])


def _run_twice(row, kernel, t):
    """the row on `kernel` by name; the same call a second time gives the same bits"""
    lib = _lib.load()
    assert ops.WINOGRAD and ops.WINOGRAD4, "the Winograd kernels are tested at the process-wide switches' defaults"
    planned, rc = _call(row, t, 1 + kernel)
    assert rc == 0, (row["name"], rc, lib.idiff_last_error())
    assert planned == kernel and lib.idiff_conv2d_last_algo() == kernel, (row["name"], planned, lib.idiff_conv2d_last_algo())
    first = [v.clone() for v in _written(t)]
    for v in _written(t):
        v.fill_(SENT)
    planned, rc = _call(row, t, 1 + kernel)
    torch.cuda.synchronize()
    assert rc == 0 and planned == kernel and lib.idiff_conv2d_last_algo() == kernel
    for a, b in zip(first, _written(t)):
        assert torch.equal(a, b), f"{row['name']}: the same call twice gives different bits"


# ---- 1. one row per instantiation <MODE, SPEC, RAG> of each kernel ----------------------------------------------------------------
@pytest.mark.parametrize("row", TABLE, ids=[r["name"] for r in TABLE])
def test_winograd_kernel_branch(row):
    kernel = row["kernel"]
    assert row["claim"] == expected_instantiation(row) and eligible(row, kernel)
    inp = make_inputs(row, 3000 + IDS.index(row["name"]))
    t, guards = _operands(row, inp)
    _run_twice(row, kernel, t)
    _compare(row, kernel, inp, t, guards)


# ---- 2. the item stream of a persistent workgroup ---------------------------------------------------------------------------------
@pytest.mark.parametrize("row", STREAM, ids=[r["name"] for r in STREAM])
def test_winograd_item_stream(row):
    """B from the device's CU count so that every workgroup walks `per` items (three in flight at per = 4: every table parity of
    conv_wino.hip, every carry of the item counter of the F(4x4,3x3) kernels; per = 2 on the ragged image: whole and partial patches in
    one sequence).  Samples 0, the middle one and the last, convolved alone, give the bits they get inside the batch."""
    kernel = row["kernel"]
    B, g, full, carries, crossing = stream_facts(row, kernel, _num_cu())
    want = row["stream"]["per"]
    assert g["per"] == want, (row["name"], g["per"])
    if want >= 4:
        assert full and carries == {"column", "row", "sample"}, (row["name"], carries)
    else:
        assert crossing, row["name"]
    if row["stream"]["short"]:
        assert g["total"] % want != 0 and len(g["seq"](g["grid"] - 1)) < want
    row = dict(row, B=B)
    assert row["claim"] == expected_instantiation(row) and eligible(row, kernel)
    print(f"{row['name']}: B {B}, {g['total']} items on {g['grid']} workgroups, {want} each; carries {sorted(carries)}")
    inp = make_inputs(row, 3000 + IDS.index(row["name"]))
    t, guards = _operands(row, inp)
    _run_twice(row, kernel, t)
    picks = [0, B // 2, B - 1]
    _compare(row, kernel, inp, t, guards, sub=picks)
    for b in picks:
        one = dict(t)
        oflat, one["out"] = _buf((B,) + tuple(t["out"].shape[1:]))
        g1 = [(oflat, one["out"][b:b + 1], "out of one sample")]
        if row["stats"]:
            sflat, one["stats"] = _pad(tuple(t["stats"].shape))
            g1.append((sflat, one["stats"][b:b + 1], "stats of one sample"))
        planned, rc = _call(row, one, 1 + kernel, b=b)
        torch.cuda.synchronize()
        assert rc == 0 and planned == kernel and _lib.load().idiff_conv2d_last_algo() == kernel
        for flat, view, what in g1:
            _guard_intact(flat, view, f"{row['name']} {what} {b}")
        assert torch.equal(one["out"][b], t["out"][b]), f"{row['name']}: sample {b} alone differs from the sample inside the batch"
        if row["stats"]:
            assert torch.equal(one["stats"][b], t["stats"][b]), f"{row['name']}: statistics of sample {b} alone differ"


# ---- 3. the edges of the eligibility checks: raw idiff_conv_desc calls, as test_selection_ladder ------------------------------------
def _soft(a):
    return -(1 + a)


def _hard(a):
    return 1 + a


def _e(name, req, want, tweak, **kw):
    row = dict(name=name, kernel=None, ks=3, mode=N, B=2, C0=32, C1=0, Cout=64, Hin=32, Win=32, pro=False, res=False, vec=False, aux=False,
               bias=True, stats=False, gn=0, slices={}, odd=(), dc=False, stream=None)
    row.update(kw)
    return (row, req, want, tweak)


# row, algo_request, the kernel that must serve the call (None: IDIFF_E_BADARG and nothing written), the operand that is off
EDGES = [
    _e("out-bstride-2-mod-4-soft-16x32-lands-on-F2x2", _soft(WINO4), WINO, "out_bs+2"),
    _e("out-bstride-2-mod-4-soft-half-patch-lands-on-F2x2", _soft(WINO4H), WINO, "out_bs+2"),
    _e("out-bstride-2-mod-4-hard-16x32-refused", _hard(WINO4), None, "out_bs+2"),
    _e("out-bstride-2-mod-4-hard-half-patch-refused", _hard(WINO4H), None, "out_bs+2"),
    _e("out-bstride-odd-lands-on-direct", 0, DIRECT, "out_bs+1"),
    _e("out-bstride-odd-hard-F2x2-refused", _hard(WINO), None, "out_bs+1"),
    _e("res-8-not-16-byte-aligned-F2x2-serves", _soft(WINO4H), WINO, "res+2", res=True),
    _e("aux-bstride-odd-direct-serves", 0, DIRECT, "aux_bs+1", aux=True),
    _e("pro_a-4-bytes-past-16-F4x4-refused-F2x2-takes", _soft(WINO4H), WINO, "pro_a+1", pro=True),
    _e("pro_b-4-bytes-past-16-hard-16x32-refused", _hard(WINO4), None, "pro_b+1", pro=True),
    _e("aligned-soft-half-patch-taken", _soft(WINO4H), WINO4H, None, pro=True, res=True, aux=True),
    _e("prologue-upsample-hard-F2x2-refused", _hard(WINO), None, None, pro=True, mode=U, Hin=16, Win=16),
    _e("prologue-upsample-hard-16x32-refused", _hard(WINO4), None, None, pro=True, mode=U, Hin=16, Win=16),
    _e("prologue-upsample-hard-half-patch-refused", _hard(WINO4H), None, None, pro=True, mode=U, Hin=16, Win=16),
    _e("prologue-upsample-library-choice-direct", 0, DIRECT, None, pro=True, mode=U, Hin=16, Win=16),
    _e("prologue-second-source-hard-F2x2-refused", _hard(WINO), None, "pro+src1", C0=16, C1=16),
    _e("prologue-second-source-hard-16x32-refused", _hard(WINO4), None, "pro+src1", C0=16, C1=16),
    _e("prologue-second-source-hard-half-patch-refused", _hard(WINO4H), None, "pro+src1", C0=16, C1=16),
]


def _strided(shape, bstride, off, src=None):
    """(flat, view): [B, C, H, W] with batch stride `bstride` floats, `off` floats past a 16-byte boundary, inside sentinels"""
    B, C, H, W = shape
    flat = torch.full((off + B * bstride + 8,), SENT, device=DEV, dtype=torch.float32)
    view = flat.as_strided(shape, (bstride, H * W, W, 1), off)
    if src is not None:
        view.copy_(src)
    return flat, view


@pytest.mark.parametrize("row,req,want,tweak", EDGES, ids=[e[0]["name"] for e in EDGES])
def test_winograd_eligibility_edge(row, req, want, tweak):
    lib = _lib.load()
    name = row["name"]
    assert ops.WINOGRAD and ops.WINOGRAD4 and ops.X3, "the ladder is tested at the process-wide switches' defaults"
    inp = make_inputs(row, 7000 + [e[0]["name"] for e in EDGES].index(name))
    if tweak == "pro+src1":  # a call the header refuses outright: make_inputs draws no prologue for a two-source row
        g = torch.Generator().manual_seed(1)
        inp["pro"] = (torch.randn(row["B"], row["C0"], generator=g), torch.randn(row["B"], row["C0"], generator=g))
    t, guards = _operands(row, inp)
    if tweak == "pro+src1":
        t["pro"] = tuple(v.to(DEV) for v in inp["pro"])
    B, Cout = row["B"], row["Cout"]
    Hout, Wout = out_size(row)
    dense = Cout * Hout * Wout
    if tweak in ("out_bs+2", "out_bs+1"):
        oflat, t["out"] = _strided((B, Cout, Hout, Wout), dense + int(tweak[-1]), 0)
        guards = [(oflat, t["out"], "out")]
        assert _bs(t["out"]) % 4 == int(tweak[-1])
    elif tweak == "res+2":
        t["res"] = _strided((B, Cout, Hout, Wout), dense, 2, inp["res"])[1]
        assert t["res"].data_ptr() % 16 == 8
    elif tweak == "aux_bs+1":
        t["aux"] = (_strided((B, Cout, Hout, Wout), dense + 1, 0, inp["aux"][0])[1],) + t["aux"][1:]
        assert _bs(t["aux"][0]) % 2 == 1
    elif tweak in ("pro_a+1", "pro_b+1"):
        i = 0 if tweak == "pro_a+1" else 1
        flat = torch.zeros(B * row["C0"] + 8, device=DEV)
        v = flat[1:1 + B * row["C0"]].view(B, row["C0"])
        v.copy_(t["pro"][i])
        t["pro"] = tuple(v if j == i else p for j, p in enumerate(t["pro"]))
        assert t["pro"][i].data_ptr() % 16 == 4
    planned, rc = _call(row, t, req)
    torch.cuda.synchronize()
    if want is None:
        assert planned == E_BADARG and rc == E_BADARG, (name, planned, rc)
        for flat, view, what in guards:
            assert bool((flat == SENT).all()), f"{name}: a refused call wrote to {what}"
        return
    assert rc == 0, (name, rc, lib.idiff_last_error())
    assert planned == want and lib.idiff_conv2d_last_algo() == want, (name, planned, lib.idiff_conv2d_last_algo(), want)
    inp_ref = dict(inp)
    _compare(row, want, inp_ref, t, guards)
