"""The token-side, normalisation and attention kernels every denoising step runs besides the convolutions (csrc/attention.hip,
csrc/elementwise.hip, csrc/smm.hip), one table row per branch or limit of their host launchers, in the style of
test_train_kernels_gpu.py: every row runs the HIP kernel through its ops.* wrapper (the raw idiff_* entry point only where the wrapper
hides the argument under test: a NULL option, a stride, a rejection) and compares it with a plain torch float64 evaluation of the
formula written out here.  No row's reference is another kernel of this library.

Metric: max|got - ref| / max|ref| per output tensor; on rows with a tail (a size that is not a multiple of the kernel's tile, block or
lane width) also elementwise |got - ref| <= tol * max|ref| on the last partial tile alone.  Where the ragged range is a KEY range (no
spatial tail in the output) the kernel also runs without the ragged keys and its result must move by what the fp64 reference moves.

Tolerances are those the first-generation tests already use per entry point (LIN 3e-6, ATT 5e-6, XAT 1e-5, LNT 3e-6, GNT 5e-6,
MEM 5e-6).  A row whose reduction is longer or worse conditioned than anything those ran takes max(that, 4 x the error of the SAME
formula evaluated in fp32 torch on the CPU against the fp64 reference) -- _floor(); 4 covers another summation order on the device.
Offset-heavy rows use the conditioning factor _cond of the training tables.  No bound was chosen from what the kernels return.

Launcher constants read from the sources: LIN_ROWS = 8, layernorm_rows 4 rows per workgroup, chan_layernorm 64 pixels per workgroup,
LT_ROWS = 8, LM_ROWS = 16, LM_KPAD = 4, LM_WAVES = 8, MP_PX = 64, SM_KMAX = 8."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops  # noqa: E402
from instancediff_amd._lib import check  # noqa: E402
from instancediff_amd.ops import _bs, _p, _stream  # noqa: E402

from step_split_rows import SPLIT_ROWS, split_rule, witnessed_nsplit  # noqa: E402

DEV = "cuda"
EPS = 1e-5
LIN, ATT, XAT, LNT, GNT, MEM = 3e-6, 5e-6, 1e-5, 3e-6, 5e-6, 5e-6
LIN_ROWS, LT_ROWS, LM_ROWS, LM_KPAD, LM_WAVES, MP_PX, SM_KMAX = 8, 8, 16, 4, 8, 64, 8
E_BADARG, E_UNSUPPORTED = -1, -2


# ---- helpers (those of test_train_kernels_gpu.py) -------------------------------------------------------------------------------
def _cond(tol, off, spr):
    """the large-magnitude rows (values offset +- spread): x - mean loses log2(offset / spread) bits, so every fp32 rounding of the
    normalisation is amplified by offset / spread; four such roundings (mean, variance, x - mean, the product with rstd)"""
    return max(tol, 4 * (abs(off) / spr) * 2.0 ** -24) if off else tol


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, g, offset=0.0, spread=1.0):
    return torch.randn(shape, generator=g) * spread + offset


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _check(row, name, got, ref, tol, tail=None):
    """normwise max error of one output; with `tail` (an index into both) also every element of that region against tol * max|ref|"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (row, name, got.shape, ref.shape)
    scale = float(ref.abs().max().clamp_min(1e-12))
    e = float((got - ref).abs().max()) / scale
    msg = f"{row} {name}: rel {e:.2e} (tol {tol:.1e})"
    et = None
    if tail is not None:
        assert got[tail].numel() > 0, (row, name, "empty tail")
        et = float((got[tail] - ref[tail]).abs().max()) / scale
        msg += f", tail {et:.2e}"
    print(msg)
    assert math.isfinite(e) and e <= tol, msg
    if tail is not None:
        assert et <= tol, msg


def _floor(tol, f32, ref):
    """max(project tolerance, 4 x the fp32-on-the-CPU error of the same formula against fp64)"""
    return max(tol, 4 * _rel(f32, ref))


def _moves(row, name, got_full, got_cut, ref_full, ref_cut, tol):
    """the ragged keys are proven to contribute: the reference moves by well over the tolerance when they are removed, and the kernel
    moves by the same amount"""
    gf, gc, rf, rc = (t.detach().double().cpu() for t in (got_full, got_cut, ref_full, ref_cut))
    scale = float(rf.abs().max().clamp_min(1e-12))
    moved = float((rf - rc).abs().max()) / scale
    e = float(((gf - gc) - (rf - rc)).abs().max()) / scale
    print(f"{row} {name}: reference moves {moved:.2e} without the ragged keys, kernel differs from that by {e:.2e}")
    assert moved >= 20 * tol, f"{row}: the ragged keys carry too little weight to be seen ({moved:.2e})"
    assert e <= 2 * tol, f"{row} {name}: moves {e:.2e} off the reference's (tol {2 * tol:.1e})"


def _slice(shape, extra, g, offset=0.0, spread=1.0):
    """an NCHW tensor whose samples are a channel slice [1:1+C] of a bigger buffer when extra > 0 (batch stride > C*H*W)"""
    B, Cc = shape[:2]
    if not extra:
        return _rand(shape, g, offset, spread).to(DEV)
    big = _rand((B, Cc + extra) + tuple(shape[2:]), g, offset, spread).to(DEV)
    return big[:, 1:1 + Cc]


def _odd(t):
    """t's values in a buffer that starts one float after a 16-byte boundary (same shape and strides)"""
    span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    flat = torch.zeros((span + 5,), device=DEV, dtype=torch.float32)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + span].as_strided(t.shape, t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _rejects(call, code):
    """a rejection row: the documented code, a message, and no launch"""
    lib = _lib.load()
    n0 = lib.idiff_launch_count()
    rc = call(lib)
    assert rc == code, (rc, code, lib.idiff_last_error())
    assert lib.idiff_last_error()
    assert lib.idiff_launch_count() == n0


def silu64(x):
    return x * torch.sigmoid(x)


def _act(x, a):
    return {ops.ACT_NONE: lambda v: v, ops.ACT_SILU: silu64, ops.ACT_GELU: F.gelu}[a](x)


def _attn_ref(q, k, v, heads, scale):
    """softmax(q k^T * scale) v per head; q [B,N,C], k, v [B,M,C] (any float type) -> (out [B,N,C], scores [B,heads,N,M])"""
    B, N, C = q.shape
    M = k.shape[1]
    dh = C // heads
    s = torch.einsum('bnhd,bmhd->bhnm', q.reshape(B, N, heads, dh), k.reshape(B, M, heads, dh)) * scale
    return torch.einsum('bhnm,bmhd->bnhd', s.softmax(-1), v.reshape(B, M, heads, dh)).reshape(B, N, C), s


# =====================================================================================================
# 1. attention over context tokens (idiff_attn_ctx_fwd): attn_ctx_kernel<16 | 32 | 64> by dh = C / heads, 256 pixels per workgroup
#    (`p >= N` returns), the M tokens in a loop (M <= 32, 2 M dh floats of LDS).
#    dh x M crossed; N walks {1, 255, 256, 257, 4096}: N < 256 (one partial workgroup), N % 256 == 0 (no tail), N = 257 (a tail of one).
# =====================================================================================================
_CTX_N = [1, 255, 256, 257, 4096]
CTX_ROWS = [(f"attn_ctx-dh{dh}-M{M}-N{_CTX_N[i % 5]}-B{1 + i % 2}-heads{1 if i % 3 == 0 else 4}", dh, M, _CTX_N[i % 5], 1 + i % 2,
             1 if i % 3 == 0 else 4) for i, (dh, M) in enumerate(itertools.product((16, 32, 64), (1, 2, 31, 32)))]
CTX_ROWS += [("attn_ctx-dh64-M32-N257-B1-heads1", 64, 32, 257, 1, 1), ("attn_ctx-dh16-M32-N255-B2-heads4", 16, 32, 255, 2, 4),
             ("attn_ctx-dh32-M32-N1-B1-heads1", 32, 32, 1, 1, 1)]


@pytest.mark.parametrize("row,dh,M,N,B,heads", [pytest.param(*r, id=r[0]) for r in CTX_ROWS])
def test_attn_ctx(row, dh, M, N, B, heads):
    g = _g(1000 + dh + M + N)
    C = dh * heads
    q = _rand((B, C, 1, N), g)
    q[0, :dh] *= 3.0  # some peaky rows
    k, v = _rand((B, M, C), g), _rand((B, M, C), g)
    scale = dh ** -0.5
    ref, _ = _attn_ref(q.double().reshape(B, C, N).permute(0, 2, 1), k.double(), v.double(), heads, scale)
    out = ops.attn_ctx(q.to(DEV), k.to(DEV), v.to(DEV), heads, scale)
    tail = (slice(None), slice(None), slice((N - 1) // 256 * 256, None)) if N % 256 else None
    _check(row, "out", out.reshape(B, C, N), ref.permute(0, 2, 1), ATT, tail)
    if M > 1:  # the last token is in the sum: without it the result moves as the reference does
        ref1, _ = _attn_ref(q.double().reshape(B, C, N).permute(0, 2, 1), k.double()[:, :M - 1], v.double()[:, :M - 1], heads, scale)
        out1 = ops.attn_ctx(q.to(DEV), k[:, :M - 1].contiguous().to(DEV), v[:, :M - 1].contiguous().to(DEV), heads, scale)
        _moves(row, "last token", out.reshape(B, C, N), out1.reshape(B, C, N), ref.permute(0, 2, 1), ref1.permute(0, 2, 1), ATT)


# =====================================================================================================
# token-major attention (idiff_attn_tokens_fwd / _grouped_fwd): attn_tokens_kernel, a wave per (b, head, query), lane = key
#   (`lane < M`, M <= 64), dh = C / heads a runtime loop bound, row strides ldq / ldkv.  Nq is a grid dimension only (the launcher does
#   not look at it: the header's former `Nq <= 64` was never a limit of the kernel; Nq = 100 below).
#   M = 64: a full wave; 33, 63: a partial one; M = 1, Nq = 1: one live lane.  dh = 24: not a power of two.  packed: q / k / v are column
#   slices of two buffers with ldq != ldkv, both > C -- through the raw entry point (the wrapper passes ld = C).
# =====================================================================================================
TOK_ROWS = [
    # id, B, heads, dh, Nq, M, packed
    ("attn_tokens-M1-Nq1-dh8-B1-heads1", 1, 1, 8, 1, 1, False),
    ("attn_tokens-M1-Nq64-dh64", 2, 4, 64, 64, 1, False),
    ("attn_tokens-M33-Nq1-dh24", 2, 4, 24, 1, 33, False),
    ("attn_tokens-M33-Nq64-dh8-packed", 3, 4, 8, 64, 33, True),
    ("attn_tokens-M63-Nq64-dh24-packed", 2, 2, 24, 64, 63, True),
    ("attn_tokens-M63-Nq1-dh64-B1-heads1", 1, 1, 64, 1, 63, False),
    ("attn_tokens-M64-Nq1-dh8", 2, 4, 8, 1, 64, False),
    ("attn_tokens-M64-Nq64-dh64-packed", 2, 4, 64, 64, 64, True),
    ("attn_tokens-M64-Nq64-dh24", 1, 3, 24, 64, 64, False),
    ("attn_tokens-M5-Nq100-dh64-Nq-is-not-limited", 1, 4, 64, 100, 5, False),
]


def _tok_operands(B, heads, dh, Nq, M, packed, g):
    """(q, k, v device views, ldq, ldkv, host q, k, v)"""
    C = heads * dh
    q, k, v = _rand((B, Nq, C), g), _rand((B, M, C), g), _rand((B, M, C), g)
    q[0, 0] *= 3.0
    if not packed:
        return q.to(DEV), k.to(DEV), v.to(DEV), C, C, q, k, v
    ldq, ldkv = C + 12, 2 * C + 20
    bq = _rand((B, Nq, ldq), g, 7.0).to(DEV)
    bkv = _rand((B, M, ldkv), g, -7.0).to(DEV)
    qv, kv_, vv = bq[:, :, 4:4 + C], bkv[:, :, 8:8 + C], bkv[:, :, 12 + C:12 + 2 * C]
    qv.copy_(q), kv_.copy_(k), vv.copy_(v)
    return qv, kv_, vv, ldq, ldkv, q, k, v


def _tok_raw(qd, kd, vd, B, Nq, M, C, heads, scale, ldq, ldkv):
    out = torch.empty((B, Nq, C), device=DEV, dtype=torch.float32)
    check(_lib.load().idiff_attn_tokens_fwd(_p(qd), _p(kd), _p(vd), _p(out), B, Nq, M, C, heads, scale, ldq, ldkv, _stream()), "attn_tokens_fwd")
    return out


@pytest.mark.parametrize("row,B,heads,dh,Nq,M,packed", [pytest.param(*r, id=r[0]) for r in TOK_ROWS])
def test_attn_tokens(row, B, heads, dh, Nq, M, packed):
    g = _g(1100 + dh + Nq + M)
    C = heads * dh
    scale = dh ** -0.5
    qd, kd, vd, ldq, ldkv, q, k, v = _tok_operands(B, heads, dh, Nq, M, packed, g)
    assert (ldq != ldkv and ldq > C and ldkv > C) == packed
    ref, _ = _attn_ref(q.double(), k.double(), v.double(), heads, scale)
    out = _tok_raw(qd, kd, vd, B, Nq, M, C, heads, scale, ldq, ldkv) if packed else ops.attn_tokens(qd, kd, vd, heads, scale)
    _check(row, "out", out, ref, ATT)
    if M > 1:  # lanes are keys: without the last key (the last live lane) the result moves as the reference does; the strides stay
        ref1, _ = _attn_ref(q.double(), k.double()[:, :M - 1], v.double()[:, :M - 1], heads, scale)
        if packed:
            # the same buffers, M - 1 rows per sample: the batch stride of k / v is M * ldkv, so this needs its own copy
            _, k1, v1, _, _, _, _, _ = _tok_operands(B, heads, dh, Nq, M - 1, True, _g(1))
            k1.copy_(k[:, :M - 1]), v1.copy_(v[:, :M - 1])
            out1 = _tok_raw(qd, k1, v1, B, Nq, M - 1, C, heads, scale, ldq, ldkv)
        else:
            out1 = ops.attn_tokens(qd, k[:, :M - 1].contiguous().to(DEV), v[:, :M - 1].contiguous().to(DEV), heads, scale)
        _moves(row, "last key", out, out1, ref, ref1, ATT)


@pytest.mark.parametrize("row,ngroups,B,Nq,C,heads", [
    pytest.param("attn_tokens_grouped-1-group", 1, 2, 5, 96, 4, id="attn_tokens_grouped-1-group"),
    pytest.param("attn_tokens_grouped-16-groups-Nq64", _lib.LINEAR_MAX_GROUPS, 2, 64, 256, 4, id="attn_tokens_grouped-16-groups-Nq64")])
def test_attn_tokens_grouped(row, ngroups, B, Nq, C, heads):
    """attn_tokens_grouped_kernel (grid.y = group): bit-equal to the single launches AND within tolerance of fp64"""
    g = _g(1200 + ngroups)
    scale = (C // heads) ** -0.5
    qkvs = [_rand((B, Nq, 3 * C), g) for _ in range(ngroups)]
    outs = ops.attn_tokens_packed_grouped([t.to(DEV) for t in qkvs], heads, scale)
    assert len(outs) == ngroups
    for i, (t, o) in enumerate(zip(qkvs, outs)):
        assert torch.equal(o, ops.attn_tokens_packed(t.to(DEV), heads, scale)), (row, i)
        qq, kk, vv = t.double().split(C, dim=-1)
        _check(row, f"group {i}", o, _attn_ref(qq, kk, vv, heads, scale)[0], ATT)


# =====================================================================================================
# 2. self-attention (idiff_attn_self_fwd): attn_self_kernel<64 | 32> by dh, 128 queries per workgroup (4 waves x 32), 32-key blocks,
#    online softmax whose O-rescale is skipped when alpha == 1 in every lane of the wave.
#    N = 4: one partial key block, one partial query wave; 124 / 132: ragged last key block and query tile; 128: exactly one workgroup.
#    structures: "rand" random scores; "first": every query's maximum sits in key block 0 (no rescale after the first block);
#    "rising": every 32-key block raises every query's maximum (rescale in every block); "pm80": scores of magnitude ~80.
#    Each structure is verified on the fp64 scores before the kernel runs.
# =====================================================================================================
SELF_ROWS = [(f"attn_self-dh{dh}-N{N}-{st}-B{B}-heads{heads}", dh, N, st, B, heads) for dh, N, st, B, heads in [
    (64, 4, "rand", 1, 1), (32, 4, "rand", 2, 4), (64, 32, "rand", 2, 4), (32, 32, "first", 1, 1), (64, 124, "rand", 2, 2),
    (32, 124, "rising", 1, 4), (64, 128, "first", 1, 4), (32, 128, "rand", 2, 4), (64, 132, "rising", 1, 1), (32, 132, "rand", 2, 4),
    (64, 132, "first", 2, 2), (64, 1024, "rand", 2, 4), (32, 1024, "rand", 1, 4), (64, 1024, "first", 1, 2), (32, 1024, "first", 1, 2),
    (64, 1024, "rising", 1, 2), (32, 1024, "rising", 1, 2), (64, 1024, "pm80", 1, 4), (32, 1024, "pm80", 1, 4)]]


def _self_qkv(dh, N, st, B, heads, g):
    """q, k, v [B, N, C] (host, fp32) with the score structure `st`"""
    C = dh * heads
    u = torch.ones(dh) / math.sqrt(dh)
    q, k, v = _rand((B, N, C), g), _rand((B, N, C), g), _rand((B, N, C), g)
    if st == "rand":
        q[0] *= 3.0
    elif st == "pm80":
        q *= 16.0  # scores ~ N(0, 16^2): their extremes over the 4 M scores of the row reach +-80
    else:
        qh, kh = q.view(B, N, heads, dh), k.view(B, N, heads, dh)
        qh.mul_(0.3).add_(2.0 * u * math.sqrt(dh) ** 0.5)
        kh.mul_(0.3)
        if st == "first":
            kh[:, 0] = 6.0 * u * math.sqrt(dh) ** 0.5
        else:
            kh.add_((torch.arange(N) // 32).float()[None, :, None, None] * 1.5 * u * math.sqrt(dh) ** 0.5)
    return q, k, v


@pytest.mark.parametrize("row,dh,N,st,B,heads", [pytest.param(*r, id=r[0]) for r in SELF_ROWS])
def test_attn_self(row, dh, N, st, B, heads):
    g = _g(2000 + dh + N + len(st))
    C = dh * heads
    scale = dh ** -0.5
    q, k, v = _self_qkv(dh, N, st, B, heads, g)
    ref, s = _attn_ref(q.double(), k.double(), v.double(), heads, scale)  # s [B, heads, N, N]
    nkb = -(-N // 32)
    if st in ("first", "rising") or st == "pm80":
        pad = torch.full((B, heads, N, nkb * 32 - N), -math.inf, dtype=torch.float64)
        bmax = torch.cat([s, pad], -1).reshape(B, heads, N, nkb, 32).max(-1).values  # per-block maximum of every query
        if st == "first":
            assert bool((s.argmax(-1) < 32).all())
            if nkb > 1:
                assert bool((bmax[..., 0:1] > bmax[..., 1:]).all())
        elif st == "rising":
            assert nkb > 1 and bool((bmax[..., 1:] > bmax[..., :-1]).all())
        else:
            assert 60.0 < float(s.abs().max()) < 130.0
    tol = ATT
    if float(s.abs().max()) > 16.0:
        # the first-generation tests ran scores of magnitude <= ~16.  A score of magnitude |s| carries an fp32 rounding of ~|s| * 2^-24
        # per term of its dot product, which the exponential turns into a RELATIVE error of the weight: at |s| ~ 80 to 90 (the pm80
        # rows, and the last blocks of the rising rows at N = 1024) that alone passes 5e-6.  The bound then comes from the same formula
        # in fp32 on the CPU (_floor); the condition looks at the fp64 reference scores only.
        tol = _floor(ATT, _attn_ref(q, k, v, heads, scale)[0], ref)
    qkv = torch.cat([q, k, v], -1).permute(0, 2, 1).reshape(B, 3 * C, 1, N).contiguous()
    out, lse = ops.attn_self(qkv.to(DEV), heads, scale, want_lse=True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    qt = slice((N - 1) // 128 * 128, None) if N % 128 else None
    _check(row, "out", out.reshape(B, C, N), ref.permute(0, 2, 1), tol, None if qt is None else (slice(None), slice(None), qt))
    _check(row, "lse", lse, torch.logsumexp(s, -1), tol, None if qt is None else (slice(None), slice(None), qt))
    N0 = N // 32 * 32
    if N % 32 and N0 and st == "rand":  # ragged last key block: the first N0 queries without those keys
        ref0, _ = _attn_ref(q.double()[:, :N0], k.double()[:, :N0], v.double()[:, :N0], heads, scale)
        qkv0 = torch.cat([q[:, :N0], k[:, :N0], v[:, :N0]], -1).permute(0, 2, 1).reshape(B, 3 * C, 1, N0).contiguous()
        out0 = ops.attn_self(qkv0.to(DEV), heads, scale)
        _moves(row, "ragged key block", out.reshape(B, C, N)[:, :, :N0], out0.reshape(B, C, N0), ref.permute(0, 2, 1)[:, :, :N0],
               ref0.permute(0, 2, 1), ATT)


# =====================================================================================================
# 3. ScoreMapModule cross-attention (idiff_smm_xattn_fwd, idiff_smm_xattn_lse_fwd / _cm_lse_fwd): the split table of
#    step_split_rows.py (nkb = 1; k floored to 2; kps = 3 | 4 for Cm = 72: smm_xattn_kernel<18> | smm_xattn_w_kernel<72>; k capped at 64
#    with a short last split; N % 32 != 0), Cm in {72, 136, 256} -> <18 | w72>, <34>, <64>, rows = Nq * heads in {1, 20, 32}.
#    Witness: idiff_smm_xattn_ws_floats / (B (Cm + 2) 32) = the split count; kps follows from it.
#    The largest rows: rows x Cm x N fp64 = 20 x 256 x 131 232: about 1.3 G multiply-adds for the two products, a second or two on 16
#    host threads.  Their sum over 131 232 keys is longer than anything the first-generation tests ran: _floor().
# =====================================================================================================
def _xattn_ref(qf, mem, scale):
    s = torch.einsum('brc,bcn->brn', qf, mem) * scale
    return torch.einsum('brn,bcn->brc', s.softmax(-1), mem), torch.logsumexp(s, -1)


@pytest.mark.parametrize("row,Cm,qh,B,N,ns,kps,boost", [pytest.param(*r, id=r[0]) for r in SPLIT_ROWS])
def test_smm_xattn(row, Cm, qh, B, N, ns, kps, boost):
    lib = _lib.load()
    Nq, heads = qh
    rows = Nq * heads
    assert witnessed_nsplit(lib, B, Nq, heads, Cm, N) == ns and split_rule(N) == (ns, kps)
    nkb = -(-N // 32)
    assert -(-nkb // kps) == ns
    if Cm == 72:
        assert ("wform" in row) == (kps >= 4) and ("k18" in row) == (kps < 4)
    g = _g(3000 + Cm + N)
    scale = 0.125
    qf = _rand((B, rows, Cm), g, 0.0, 0.3)
    mem = _rand((B, Cm, N), g)
    N0 = (ns - 1) * kps * 32 if ns > 1 else N // 32 * 32  # keys before the last split / before the ragged last block
    ragged = (N % 32 != 0 or nkb % kps != 0) and 0 < N0 < N
    if ragged:
        mem[:, :, N0:] *= boost
    ref, rlse = _xattn_ref(qf.double(), mem.double(), scale)
    tol = _floor(XAT, _xattn_ref(qf, mem, scale)[0], ref) if N > 65536 else XAT
    qd, md = qf.to(DEV), mem.to(DEV)
    out = ops.smm_xattn(qd.reshape(B, Nq, heads, Cm), md, scale).reshape(B, rows, Cm)
    _check(row, "o", out, ref, tol)
    # the training-path entry point of the same launcher: o again and the log-sum-exp of the scaled scores
    ws = torch.empty((lib.idiff_smm_xattn_ws_floats(B, rows, 1, Cm, N),), device=DEV, dtype=torch.float32)
    o2, lse = torch.empty_like(qd), torch.empty((B, rows), device=DEV, dtype=torch.float32)
    if Cm == 256:
        check(lib.idiff_smm_xattn_lse_fwd(_p(qd), _p(md), _p(o2), _p(lse), _p(ws), B, rows, N, scale, _stream()), "smm_xattn_lse_fwd")
    else:
        check(lib.idiff_smm_xattn_cm_lse_fwd(_p(qd), _p(md), _p(o2), _p(lse), _p(ws), B, rows, Cm, N, scale, _stream()), "smm_xattn_cm_lse_fwd")
    _check(row, "o (lse form)", o2, ref, tol)
    _check(row, "lse", lse, rlse, tol)
    if ragged:
        ref0, _ = _xattn_ref(qf.double(), mem.double()[:, :, :N0], scale)
        out0 = ops.smm_xattn(qd.reshape(B, Nq, heads, Cm), md[:, :, :N0].contiguous(), scale).reshape(B, rows, Cm)
        _moves(row, "last split / ragged block", out, out0, ref, ref0, tol)


# =====================================================================================================
# 4. normalisation and elementwise
# idiff_affine_silu_add: affine_silu_add_kernel<true> (float4) when HW % 4 == 0, every batch stride % 4 == 0 and h / out / res 16-byte
#   aligned, else <false> (scalar).  The id names the form; the test re-derives it from the operands it built.
# =====================================================================================================
ASA_ROWS = [
    # id, B, C, HW, a/b, res, vec, extra channels (batch strides > C*HW on h, res, out), odd-offset buffers, expects vec4
    ("asa-scalar-HW1", 2, 5, 1, True, True, True, 0, False, False),
    ("asa-scalar-HW63-slices", 2, 3, 63, True, True, True, 2, False, False),
    ("asa-vec4-HW64-slices", 3, 4, 64, True, True, True, 2, False, True),
    ("asa-scalar-HW1023", 1, 3, 1023, True, True, True, 0, False, False),
    ("asa-scalar-HW64-odd-element-offset", 2, 4, 64, True, True, True, 0, True, False),
    ("asa-scalar-HW1024-odd-element-offset-slices", 2, 3, 1024, True, True, True, 1, True, False),
    ("asa-vec4-HW64-no-ab", 2, 4, 64, False, True, True, 0, False, True),
    ("asa-vec4-HW64-no-res", 2, 4, 64, True, False, True, 1, False, True),
    ("asa-vec4-HW64-no-vec", 2, 4, 64, True, True, False, 0, False, True),
    ("asa-scalar-HW63-no-ab", 2, 4, 63, False, True, True, 0, False, False),
    ("asa-scalar-HW63-no-res", 2, 4, 63, True, False, True, 1, False, False),
    ("asa-scalar-HW63-no-vec", 2, 4, 63, True, True, False, 0, False, False),
    ("asa-vec4-HW1024-C64", 2, 64, 1024, True, True, True, 3, False, True),
]


@pytest.mark.parametrize("row,B,C,HW,ab,res,vec,extra,odd,vec4", [pytest.param(*r, id=r[0]) for r in ASA_ROWS])
def test_affine_silu_add(row, B, C, HW, ab, res, vec, extra, odd, vec4):
    g = _g(4000 + HW + C)
    mk = (lambda t: _odd(t)) if odd else (lambda t: t)
    h = mk(_slice((B, C, 1, HW), extra, g))
    r = mk(_slice((B, C, 1, HW), extra, g)) if res else None
    out = mk(_slice((B, C, 1, HW), extra, g, 99.0))
    a, b = (_rand((B, C), g, 1.0, 0.5).to(DEV), _rand((B, C), g).to(DEV)) if ab else (None, None)
    vv = _rand((B, C), g).to(DEV) if vec else None
    if extra and B > 1:
        assert _bs(h) > C * HW and _bs(out) > C * HW
    ptrs = h.data_ptr() | out.data_ptr() | (r.data_ptr() if res else 0)
    assert vec4 == (HW % 4 == 0 and _bs(h) % 4 == 0 and _bs(out) % 4 == 0 and (not res or _bs(r) % 4 == 0) and ptrs % 16 == 0)
    t = h.double()
    if ab:
        t = silu64(a.double()[:, :, None, None] * t + b.double()[:, :, None, None])
    ref = t + (r.double() if res else 0.0) + (vv.double()[:, :, None, None] if vec else 0.0)
    got = ops.affine_silu_add(h, (a, b) if ab else None, res=r, vec=vv, out=out)
    assert got.data_ptr() == out.data_ptr()
    _check(row, "out", out, ref, GNT, (slice(None), slice(None), slice(None), slice((HW - 1) // 4 * 4, None)))


# =====================================================================================================
# idiff_chan_layernorm_fwd: chan_layernorm_kernel<32> (C <= 128), <64> (C <= 256), <0> (above), 64 pixels per workgroup, optional
#   mean_rstd.  Already pinned by test_train_kernels_gpu.py::test_chan_layernorm, which asserts `out` (y) against fp64 with mean_rstd
#   requested: cln_bwd-fused32-tpw1-single-partial-tile-B1 (<32>, C = 100, HW = 63), cln_bwd-fused32-tpw1-B3-slice (<32>, sliced
#   input), cln_bwd-fused64-tpw8-partial (<64>, C = 200, HW = 4355), cln_bwd-unfused-C300-B3-slice (<0>, C = 300, HW = 1025, sliced
#   input), cln_bwd-fused64-tpw8-offset10 (offset-heavy, C = 256).  Not repeated here.  New: the boundaries C = 1, 128 | 129, 256 | 257,
#   HW = 1 and 4096, no mean_rstd, a sliced OUTPUT (raw call), an offset-heavy row on <0> without mean_rstd.
# =====================================================================================================
CLN_ROWS = [
    # id, B, C, HW, extra channels on x, sliced out, mean_rstd, offset, spread
    ("cln-k32-C1-HW65-mr", 2, 1, 65, 0, False, True, 0.0, 1.0),
    ("cln-k32-C128-HW63-no-mr-xslice", 2, 128, 63, 3, False, False, 0.0, 1.0),
    ("cln-k32-C100-HW1-outslice-mr", 3, 100, 1, 0, True, True, 0.0, 1.0),
    ("cln-k64-C129-HW65-no-mr", 2, 129, 65, 0, False, False, 0.0, 1.0),
    ("cln-k64-C256-HW4096-mr-xslice-outslice", 2, 256, 4096, 2, True, True, 0.0, 1.0),
    ("cln-k64-C256-HW1-no-mr", 1, 256, 1, 0, False, False, 0.0, 1.0),
    ("cln-k0-C257-HW63-mr", 2, 257, 63, 0, False, True, 0.0, 1.0),
    ("cln-k0-C300-HW1-no-mr-outslice", 2, 300, 1, 0, True, False, 0.0, 1.0),
    ("cln-k0-C257-HW4096-no-mr-xslice", 1, 257, 4096, 1, False, False, 0.0, 1.0),
    ("cln-k0-C300-HW65-offset10-no-mr", 2, 300, 65, 0, False, False, 10.0, 0.1),
    ("cln-k32-C128-HW65-offset10-mr", 2, 128, 65, 0, False, True, 10.0, 0.1),
]


@pytest.mark.parametrize("row,B,C,HW,extra,oslice,mr,off,spr", [pytest.param(*r, id=r[0]) for r in CLN_ROWS])
def test_chan_layernorm(row, B, C, HW, extra, oslice, mr, off, spr):
    lib = _lib.load()
    assert ("k32" in row) == (C <= 128) and ("k64" in row) == (128 < C <= 256) and ("k0" in row) == (C > 256)
    g = _g(4100 + C + HW)
    x = _slice((B, C, 1, HW), extra, g, off, spr)
    ga, be = _rand((C,), g, 1.0, 0.5).to(DEV), _rand((C,), g).to(DEV)
    out = _slice((B, C, 1, HW), 2 if oslice else 0, g, 55.0)
    mrt = torch.empty((B, HW, 2), device=DEV, dtype=torch.float32) if mr else None
    check(lib.idiff_chan_layernorm_fwd(_p(x), _bs(x), _p(ga), _p(be), _p(out), _bs(out), B, C, HW, EPS, _p(mrt), _stream()), "chan_layernorm")
    xd = x.double().reshape(B, C, HW)
    ref = F.layer_norm(xd.permute(0, 2, 1), (C,), ga.double(), be.double(), EPS).permute(0, 2, 1)
    tail = (slice(None), slice(None), slice((HW - 1) // 64 * 64, None)) if HW % 64 else None
    tol = _cond(LNT, off, spr)
    _check(row, "out", out.reshape(B, C, HW), ref, tol, tail)
    if mr:
        _check(row, "mean", mrt[..., 0], xd.mean(1), tol)
        _check(row, "rstd", mrt[..., 1], 1 / torch.sqrt(xd.var(1, unbiased=False) + EPS), tol)


# =====================================================================================================
# idiff_gn_finalize: gn_finalize_kernel, a workgroup per (b, group); thread = (channel of the group, tile phase) with 256 / cpg phases,
#   fp64 sums of the ntiles partials; cpg = C / groups <= 256; film NULL | [B, 2C] with row stride film_ld; mean_rstd optional.
#   Synthetic partials: fp32 numbers whose fp64 sums the reference forms itself (torch.sum in fp64 over the same values -- exact to
#   fp64 rounding).  ntiles = 1 and the tile count of a 256 x 256 map (idiff_conv2d_num_tiles).  The offset-heavy row (mean 10, spread
#   0.1) is the case the fp64 finalize exists for: var = E[x^2] - mean^2 cancels seven digits.
# =====================================================================================================
GNF_ROWS = [
    # id, B, C, groups, (H, W) of the map (ntiles from the library) or None (1 tile), film, film_ld - 2C, mean_rstd, offset, spread
    ("gnf-cpg1-ntiles1-film-mr", 2, 8, 8, None, True, 0, True, 0.0, 1.0),
    ("gnf-cpg8-ntiles1-nofilm-no-mr", 3, 64, 8, None, False, 0, False, 0.0, 1.0),
    ("gnf-cpg256-ntiles1-film-ld-padded", 2, 512, 2, None, True, 24, True, 0.0, 1.0),
    ("gnf-cpg1-map256x256-nofilm-mr", 1, 4, 4, (256, 256), False, 0, True, 0.0, 1.0),
    ("gnf-cpg8-map256x256-film-ld-padded-no-mr", 2, 64, 8, (256, 256), True, 8, False, 0.0, 1.0),
    ("gnf-cpg256-map256x256-film-mr", 1, 256, 1, (256, 256), True, 0, True, 0.0, 1.0),
    ("gnf-cpg3-map64x64-nofilm-mr", 2, 12, 4, (64, 64), False, 0, True, 0.0, 1.0),
    ("gnf-cpg8-map256x256-offset10-film-mr", 2, 64, 8, (256, 256), True, 0, True, 10.0, 0.1),
]


def _gn_ref(stats, groups, HW, gamma, beta, film, eps):
    """a, b, mean, rstd in fp64 from the partials [B, nt, C, 2] (the header's formula)"""
    B, nt, C, _ = stats.shape
    cpg = C // groups
    sd = stats.double().sum(1).reshape(B, groups, cpg, 2).sum(2)
    cnt = cpg * HW
    mean = sd[..., 0] / cnt
    var = (sd[..., 1] / cnt - mean * mean).clamp_min(0.0)
    rstd = 1 / torch.sqrt(var + eps)
    mc, rc = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    a = rc * gamma.double()
    b = beta.double() - mc * a
    if film is not None:
        sc, sh = 1 + film.double()[:, :C], film.double()[:, C:2 * C]
        a, b = a * sc, b * sc + sh
    return a, b, mean, rstd


@pytest.mark.parametrize("row,B,C,groups,hw,film,fpad,mr,off,spr", [pytest.param(*r, id=r[0]) for r in GNF_ROWS])
def test_gn_finalize_synthetic(row, B, C, groups, hw, film, fpad, mr, off, spr):
    lib = _lib.load()
    g = _g(4200 + C + groups)
    nt = lib.idiff_conv2d_num_tiles(*hw) if hw else 1
    HW = hw[0] * hw[1] if hw else 48
    assert C // groups <= 256 and nt >= 1
    per = HW / nt  # pixels behind one partial
    m = _rand((B, nt, C), g, off, spr * 0.05)              # the tile means
    sq = (m * m + spr * spr * (1 + 0.1 * _rand((B, nt, C), g))).clamp_min(0)
    stats = torch.stack([m * per, sq * per], -1).contiguous()  # fp32 partial (sum, sum of squares)
    ga, be = _rand((C,), g, 1.0, 0.5), _rand((C,), g)
    fl = None
    if film:
        fl = (_rand((B, 2 * C + fpad), g) * 0.3).to(DEV)[:, :2 * C]
        assert fl.stride(0) == 2 * C + fpad
    a, b, mean, rstd = _gn_ref(stats, groups, HW, ga, be, fl.cpu() if film else None, EPS)
    got = ops.gn_finalize(stats.to(DEV), groups, HW, ga.to(DEV), be.to(DEV), film=fl, eps=EPS, want_mean_rstd=mr)
    tol = _cond(GNT, off, spr)
    _check(row, "a", got[0], a, tol)
    _check(row, "b", got[1], b, tol)
    if mr:
        _check(row, "mean", got[2][..., 0], mean, tol)
        _check(row, "rstd", got[2][..., 1], rstd, tol)


@pytest.mark.parametrize("row,Cout,groups,H,W,film", [
    pytest.param("gnf-conv-cpg8-32x32-film", 64, 8, 32, 32, True, id="gnf-conv-cpg8-32x32-film"),
    pytest.param("gnf-conv-cpg1-24x40-nofilm", 16, 16, 24, 40, False, id="gnf-conv-cpg1-24x40-nofilm")])
def test_gn_finalize_conv_partials(row, Cout, groups, H, W, film):
    """partials produced by a real conv (idiff_conv2d_fwd with `stats`): the statistics of the map the conv wrote, in fp64"""
    g = _g(4300 + Cout)
    B = 2
    x = _rand((B, 16, H, W), g).to(DEV)
    w = (_rand((Cout, 16, 3, 3), g) / 12).to(DEV)
    ga, be = _rand((Cout,), g, 1.0, 0.5).to(DEV), _rand((Cout,), g).to(DEV)
    fl = (_rand((B, 2 * Cout + 4), g) * 0.3).to(DEV)[:, :2 * Cout] if film else None
    hd, stats = ops.conv2d(x, ops.pack_conv_weight(w), None, 3, Cout, want_stats=True)
    a, b, mr = ops.gn_finalize(stats, groups, H * W, ga, be, film=fl, eps=EPS, want_mean_rstd=True)
    hg = hd.double().reshape(B, groups, -1)
    mean, rstd = hg.mean(-1), 1 / torch.sqrt(hg.var(-1, unbiased=False) + EPS)
    cpg = Cout // groups
    ra = rstd.repeat_interleave(cpg, 1) * ga.double()
    rb = be.double() - mean.repeat_interleave(cpg, 1) * ra
    if film:
        sc, sh = 1 + fl.double()[:, :Cout], fl.double()[:, Cout:]
        ra, rb = ra * sc, rb * sc + sh
    _check(row, "a", a, ra, GNT)
    _check(row, "b", b, rb, GNT)
    _check(row, "mean", mr[..., 0], mean, GNT)
    _check(row, "rstd", mr[..., 1], rstd, GNT)
    ref = F.group_norm(hd.double(), groups, ga.double(), be.double(), EPS)
    if film:
        ref = ref * sc[:, :, None, None] + sh[:, :, None, None]
    _check(row, "silu(a h + b)", ops.affine_silu_add(hd, (a, b)), silu64(ref), GNT)


# =====================================================================================================
# idiff_layernorm_rows_fwd: layernorm_rows_kernel, a wave per row, 4 rows per workgroup (`r >= R` returns), lanes stride over C.
#   test_train_kernels_gpu.py::test_layernorm_rows asserts `out` for (R, C) = (1001, 256), (7, 512), (13, 200) column slice, (1, 100),
#   (515, 256) offset-heavy.  New: R in {1, 3, 4, 5}, C in {1, 63, 64, 65, 1000}, mean_rstd requested / not, NULL gamma / beta (raw).
# =====================================================================================================
LNR_ROWS = [
    # id, R, C, extra columns (x a column slice), mean_rstd, gamma/beta present
    ("lnr-R1-C1", 1, 1, 0, True, True), ("lnr-R3-C63-colslice", 3, 63, 5, False, True), ("lnr-R4-C64", 4, 64, 0, True, True),
    ("lnr-R5-C65-colslice-no-affine", 5, 65, 3, True, False), ("lnr-R5-C1000", 5, 1000, 0, False, True), ("lnr-R3-C1000-colslice", 3, 1000, 24, True, True),
]


@pytest.mark.parametrize("row,R,C,extra,mr,affine", [pytest.param(*r, id=r[0]) for r in LNR_ROWS])
def test_layernorm_rows(row, R, C, extra, mr, affine):
    lib = _lib.load()
    g = _g(4400 + R + C)
    x = _rand((R, C + extra), g).to(DEV)[:, extra // 2:extra // 2 + C]
    ga, be = (_rand((C,), g, 1.0, 0.5).to(DEV), _rand((C,), g).to(DEV)) if affine else (None, None)
    ref = F.layer_norm(x.double(), (C,), ga.double() if affine else None, be.double() if affine else None, EPS)
    tail = (slice((R - 1) // 4 * 4, None), slice((C - 1) // 64 * 64, None))
    if affine:
        got = ops.layernorm_rows(x, ga, be, EPS, want_mean_rstd=mr)
        out, mrt = got if mr else (got, None)
    else:
        out = torch.empty((R, C + 2), device=DEV)[:, :C]  # strided output too
        mrt = torch.empty((R, 2), device=DEV) if mr else None
        check(lib.idiff_layernorm_rows_fwd(_p(x), x.stride(0), None, None, _p(out), out.stride(0), R, C, EPS, _p(mrt), _stream()), "layernorm_rows")
    _check(row, "out", out, ref, LNT, tail)
    if mr:
        _check(row, "mean", mrt[:, 0], x.double().mean(1), LNT)
        _check(row, "rstd", mrt[:, 1], 1 / torch.sqrt(x.double().var(1, unbiased=False) + EPS), LNT)


# =====================================================================================================
# idiff_linear_fwd: linear_kernel, a wave per (output n, chunk of LIN_ROWS = 8 rows), 4 outputs per workgroup (`n >= N` returns),
#   lanes stride over K.  R in {1, 3, 4, 5} and around LIN_ROWS (7, 8, 9), N in {1, 3, 4, 5}, K in {1, 63, 64, 65, 1000}; all nine
#   act_in / act_out pairs; each of bias / res / gscale absent; strided x, w, res, out.
# =====================================================================================================
_ACTS = list(itertools.product((ops.ACT_NONE, ops.ACT_SILU, ops.ACT_GELU), repeat=2))
_LR, _LN, _LK = [1, 3, 4, 5, 7, 8, 9, 17], [1, 3, 4, 5], [1, 63, 64, 65, 1000]
LINF_ROWS = [(f"linear-R{_LR[i % 8]}-N{_LN[i % 4]}-K{_LK[i % 5]}-act{ai}{ao}-{'strided' if i % 2 else 'dense'}"
              f"{'-nobias' if i % 3 == 0 else ''}{'-nores' if i % 3 == 1 else ''}{'-nogscale' if i % 3 == 2 else ''}",
              _LR[i % 8], _LN[i % 4], _LK[i % 5], ai, ao, bool(i % 2), i % 3) for i, (ai, ao) in enumerate(_ACTS + _ACTS[:6])]
LINF_ROWS.append(("linear-R9-N77-K300-act12-strided-all-operands", 9, 77, 300, 1, 2, True, 3))


@pytest.mark.parametrize("row,R,N,K,ai,ao,strided,absent", [pytest.param(*r, id=r[0]) for r in LINF_ROWS])
def test_linear_fwd(row, R, N, K, ai, ao, strided, absent):
    g = _g(4500 + R + N + K)
    pad = 7 if strided else 0
    x = _rand((R, K + pad), g).to(DEV)[:, pad // 2:pad // 2 + K]
    w = (_rand((N, K + pad), g) / math.sqrt(K)).to(DEV)[:, pad // 3:pad // 3 + K]
    bias = _rand((N,), g).to(DEV) if absent != 0 else None
    res = _rand((R, N + pad), g).to(DEV)[:, pad // 2:pad // 2 + N] if absent != 1 else None
    gs = _rand((N,), g).to(DEV) if absent != 2 else None
    out = torch.full((R, N + pad), 77.0, device=DEV)[:, pad // 4:pad // 4 + N]
    ref = _act(x.double(), ai) @ w.double().T
    if bias is not None:
        ref = ref + bias.double()
    if gs is not None:
        ref = gs.double() * ref
    if res is not None:
        ref = ref + res.double()
    ref = _act(ref, ao)
    ops.linear(x, w, bias, res=res, gscale=gs, act_in=ai, act_out=ao, out=out)
    _check(row, "out", out, ref, LIN, (slice((R - 1) // LIN_ROWS * LIN_ROWS, None), slice((N - 1) // 4 * 4, None)))


# =====================================================================================================
# 5. transposed-weight linear (linear_t_launch in csrc/smm.hip).  The matrix-core kernel (linear_t_mfma_kernel, LM_ROWS = 16 rows per
#    workgroup) runs when N % 4 == 0 && ldw % 4 == 0 && w_hs % 4 == 0 && wT 16-byte aligned && lds_m <= 160 KiB with
#    lds_m = (16 (K + 4) + 8 * 1024) * 4 bytes (K <= 2044); else the vector kernel (linear_t_kernel, LT_ROWS = 8 rows per workgroup,
#    lds = (8 K + 2048) * 4 bytes).  LDS above 64 KiB (hipFuncSetAttribute): matrix-core K >= 509, vector K >= 1793.  No query names
#    the kernel taken: each row re-derives the launcher's condition from the operands it built and asserts what its id says.
#    Limits: the vector kernel's LDS passes the 160 KiB a workgroup can have at K = 4865.  The launcher used to accept K <= 8192 and
#    ask for up to 264 KiB; it now returns IDIFF_E_UNSUPPORTED there (K = 4864 accepted, 4865 and 8192 rejected, 8193 IDIFF_E_BADARG);
#    the issue's `K = 8192 accepted` row is dropped for that reason: no kernel of the launcher can host it.
#    Rows with K >= 1024 sum longer than the first-generation tests did (K <= 1024 at 3e-6): _floor().
# =====================================================================================================
def _lt_path(N, ldw, ptr, K, w_hs=0):
    lds_m = (LM_ROWS * (K + LM_KPAD) + LM_WAVES * 4 * 64 * 4) * 4
    mfma = N % 4 == 0 and ldw % 4 == 0 and w_hs % 4 == 0 and ptr % 16 == 0 and lds_m <= 160 * 1024
    return ("mfma", lds_m) if mfma else ("vector", (LT_ROWS * K + 4 * LT_ROWS * 64) * 4)


LT_ROWS_TABLE = [
    # id, R, K, N, extra weight columns (ldw = N + that), weight view starts one float in, expected path, LDS above 64 KiB
    ("lt-mfma-R15-K256-N256", 15, 256, 256, 0, False, "mfma", False),
    ("lt-mfma-R16-K64-N72", 16, 64, 72, 0, False, "mfma", False),
    ("lt-mfma-R17-K300-N100-ldw-padded-by-4", 17, 300, 100, 4, False, "mfma", False),
    ("lt-vector-N%4-R7-K300-N77", 7, 300, 77, 0, False, "vector", False),
    ("lt-vector-N%4-R9-K64-N1", 9, 64, 1, 0, False, "vector", False),
    ("lt-vector-ldw%4-R8-K256-N64-ldw67", 8, 256, 64, 3, False, "vector", False),
    ("lt-vector-wT-misaligned-R9-K256-N64", 9, 256, 64, 4, True, "vector", False),
    ("lt-mfma-lds-above-64K-R17-K1024-N256", 17, 1024, 256, 0, False, "mfma", True),
    ("lt-mfma-lds-160K-R33-K2044-N64", 33, 2044, 64, 0, False, "mfma", True),
    ("lt-vector-lds_m-above-160K-R17-K2045-N64", 17, 2045, 64, 0, False, "vector", True),
    ("lt-vector-lds_m-above-160K-R9-K2048-N128", 9, 2048, 128, 0, False, "vector", True),
    ("lt-vector-N%4-lds-above-64K-R9-K1800-N70", 9, 1800, 70, 0, False, "vector", True),
    ("lt-vector-lds-160K-R9-K4864-N64", 9, 4864, 64, 0, False, "vector", True),
]


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("row,R,K,N,wpad,mis,path,big", [pytest.param(*r, id=r[0]) for r in LT_ROWS_TABLE])
def test_linear_t(row, R, K, N, wpad, mis, path, big, ln):
    g = _g(5000 + R + K + N)
    x = _rand((R, K + 8), g).to(DEV)[:, 3:3 + K]
    wT = (_rand((K, N + wpad), g) / math.sqrt(K)).to(DEV)
    if mis:
        wT = _odd(wT)
    wT = wT[:, :N]
    bias, gs = _rand((N,), g).to(DEV), _rand((N,), g).to(DEV)
    res = _rand((R, N + 5), g).to(DEV)[:, 2:2 + N]
    out = torch.full((R, N + 3), 77.0, device=DEV)[:, 1:1 + N]
    got_path, lds = _lt_path(N, wT.stride(0), wT.data_ptr(), K)
    assert got_path == path and (lds > 64 * 1024) == big and lds <= 160 * 1024, (got_path, lds)
    lnp = (_rand((K,), g, 1.0, 0.5).to(DEV), _rand((K,), g).to(DEV), EPS) if ln else None
    ai = ops.ACT_NONE if ln else ops.ACT_SILU

    def formula(dt):
        xx = x.to(dt).cpu()
        xx = F.layer_norm(xx, (K,), lnp[0].to(dt).cpu(), lnp[1].to(dt).cpu(), EPS) if ln else _act(xx, ai)
        return F.gelu(res.to(dt).cpu() + gs.to(dt).cpu() * (xx @ wT.to(dt).cpu() + bias.to(dt).cpu()))
    ref = formula(torch.float64)
    tol = _floor(LIN, formula(torch.float32), ref) if K >= 1024 else LIN
    ops.linear_t(x, wT, bias, res=res, gscale=gs, act_in=ai, act_out=ops.ACT_GELU, out=out, ln=lnp)
    rows = LM_ROWS if path == "mfma" else LT_ROWS
    _check(row, "out", out, ref, tol, (slice((R - 1) // rows * rows, None), slice((N - 1) // 64 * 64, None)))
    # every optional operand absent
    out2 = ops.linear_t(x, wT, ln=lnp)
    xx = F.layer_norm(x.double(), (K,), lnp[0].double(), lnp[1].double(), EPS) if ln else x.double()
    _check(row, "out (no bias / res / gscale / act)", out2, xx @ wT.double(), tol)


def test_linear_t_heads_strides():
    """idiff_linear_t_heads_fwd with non-trivial head strides on both paths: w_hs % 4 == 0 (matrix-core) and w_hs = 66 (vector)"""
    g = _g(5100)
    R, heads, K, N = 19, 3, 40, 24
    for w_hs, path in ((K * 28, "mfma"), (66, "vector")):
        x = _rand((R, heads * 44 + 3), g).to(DEV)             # x_hs = 44 > K
        wT = _rand((heads * K + 4, 28), g).to(DEV)            # ldw = 28 > N
        bias = _rand((heads * 30,), g).to(DEV)                # b_hs = 30 > N
        out = torch.full((R, heads * 32), 77.0, device=DEV)   # o_hs = 32 > N
        assert _lt_path(N, 28, wT.data_ptr(), K, w_hs)[0] == path
        ops.linear_t_heads(x, wT, bias, out, heads, K, N, x_hs=44, w_hs=w_hs, b_hs=30, o_hs=32)
        flat = wT.reshape(-1).double()
        for h in range(heads):
            wh = torch.stack([flat[h * w_hs + kk * 28:h * w_hs + kk * 28 + N] for kk in range(K)])
            ref = x[:, h * 44:h * 44 + K].double() @ wh + bias[h * 30:h * 30 + N].double()
            _check(f"lt_heads-{path}-head{h}", "out", out[:, h * 32:h * 32 + N], ref, LIN, (slice(16, None),))
            assert bool((out[:, h * 32 + N:(h + 1) * 32] == 77.0).all())


def test_linear_t_grouped_mixed():
    """idiff_linear_t_grouped_fwd: groups of different (R, K, N), LayerNorm and plain groups mixed, strided operands -- against fp64
    (the bit-equality with the single launches is test_ops2_gpu.py's)"""
    g = _g(5200)
    groups, refs = [], []
    for R, K, N, ln, res, gs, ai, ao in ((80, 256, 768, True, False, False, 0, 0), (17, 64, 72, False, True, True, 1, 2), (1, 1000, 4, True, True, False, 0, 1),
                                           (33, 136, 64, False, False, False, 2, 0), (16, 1024, 256, True, False, True, 0, 2), (5, 8, 260, False, True, False, 0, 0)):
        x = _rand((R, K + 8), g).to(DEV)[:, 4:4 + K]
        wT = (_rand((K, N + 4), g) / math.sqrt(K)).to(DEV)[:, :N]
        kw = dict(x=x, wT=wT, bias=_rand((N,), g).to(DEV), act_in=ai, act_out=ao, out=torch.full((R, N + 2), 77.0, device=DEV)[:, :N])
        xx = x.double()
        if ln:
            kw["ln"] = (_rand((K,), g, 1.0, 0.5).to(DEV), _rand((K,), g).to(DEV), EPS)
            xx = F.layer_norm(xx, (K,), kw["ln"][0].double(), kw["ln"][1].double(), EPS)
        ref = _act(xx, ai) @ wT.double() + kw["bias"].double()
        if gs:
            kw["gscale"] = _rand((N,), g).to(DEV)
            ref = kw["gscale"].double() * ref
        if res:
            kw["res"] = _rand((R, N + 6), g).to(DEV)[:, 3:3 + N]
            ref = ref + kw["res"].double()
        groups.append(kw)
        refs.append(_act(ref, ao))
    outs = ops.linear_t_grouped(groups)
    for i, (o, r) in enumerate(zip(outs, refs)):
        R, N = r.shape
        _check(f"lt_grouped-group{i}", "out", o, r, LIN, (slice((R - 1) // LM_ROWS * LM_ROWS, None), slice((N - 1) // 64 * 64, None)))


# =====================================================================================================
# 6. score map, memory projection, time MLP
# idiff_scoremap_fwd: K <= SM_KMAX = 8; the shape set of test_ops_gpu.py covers both kernels; new: K = 1 and K = 8 on both forms.
# =====================================================================================================
@pytest.mark.parametrize("row,K,HW,vec4", [pytest.param(f"scoremap-K{K}-HW{HW}-{'vec4' if HW % 4 == 0 else 'scalar'}", K, HW, HW % 4 == 0,
                                                        id=f"scoremap-K{K}-HW{HW}-{'vec4' if HW % 4 == 0 else 'scalar'}")
                                           for K, HW in ((1, 1028), (1, 63), (8, 1028), (8, 257))])
def test_scoremap(row, K, HW, vec4):
    g = _g(6000 + K + HW)
    B, C = 2, 66
    x = _slice((B, C, 1, HW), 2, g, 0.3, 1.5)
    tv = _rand((B, K, C), g).to(DEV)
    idx = torch.randint(0, K, (B,), generator=g).to(torch.int32).to(DEV)
    assert vec4 == (HW % 4 == 0 and _bs(x) % 4 == 0 and x.data_ptr() % 16 == 0)
    ref = torch.einsum('bchw,bkc->bkhw', F.normalize(x.double(), dim=1), F.normalize(tv.double(), dim=2))
    sm, sel = ops.scoremap(x, tv, idx)
    tail = (slice(None), slice(None), slice(None), slice((HW - 1) // (1024 if vec4 else 256) * (1024 if vec4 else 256), None))
    _check(row, "score", sm, ref, LNT, tail)
    _check(row, "sel", sel, ref[torch.arange(B), idx.long().cpu()][:, None], LNT, tail)


# =====================================================================================================
# idiff_smm_memproj_fwd: smm_memproj_kernel, MP_PX = 64 pixels per workgroup, C even <= 512, LDS (C + 6) * 256 bytes through
#   hipFuncSetAttribute (133 KiB at C = 512).  C = 2 (the smallest), 66 (not a multiple of 32), 512; N below MP_PX (one partial
#   workgroup) and just above (a tail of 4); a sliced input.
# =====================================================================================================
@pytest.mark.parametrize("row,B,C,N,extra", [pytest.param(f"memproj-C{C}-N{N}{'-slice' if e else ''}", B, C, N, e, id=f"memproj-C{C}-N{N}{'-slice' if e else ''}")
                                             for B, C, N, e in ((2, 2, 60, 0), (2, 66, 68, 4), (1, 512, 60, 0), (2, 512, 68, 4), (1, 66, 1028, 0))])
def test_smm_memproj(row, B, C, N, extra):
    g = _g(6100 + C + N)
    x = _slice((B, C, 1, N), extra, g, 0.3, 2.0)
    g1, b1 = _rand((C,), g), _rand((C,), g)
    w = _rand((256, C), g) / math.sqrt(C)
    bias, g2, b2 = _rand((256,), g), _rand((256,), g), _rand((256,), g)
    tok = x.double().cpu().reshape(B, C, N).permute(0, 2, 1)
    ref = F.layer_norm(F.linear(F.layer_norm(tok, (C,), g1.double(), b1.double(), EPS), w.double(), bias.double()), (256,), g2.double(),
                       b2.double(), EPS).permute(0, 2, 1)
    wpk = ops.pack_conv_weight(w.reshape(256, C, 1, 1).contiguous().to(DEV))
    out = ops.smm_memproj(x, g1.to(DEV), b1.to(DEV), wpk, bias.to(DEV), g2.to(DEV), b2.to(DEV), EPS)
    _check(row, "mem", out, ref, MEM, (slice(None), slice(None), slice((N - 1) // MP_PX * MP_PX, None)))


# =====================================================================================================
# idiff_smm_memproj_compact_fwd: smm_memproj_gram_kernel<16> (C = 64) / <32> (C = 128), rows [xhat * rstd (C) ; rstd ; zeros up to Cm).
#   Reference: the header's definition in fp64 -- xhat = LayerNorm_C(feat), z = W xhat + bias, rstd = 1 / sqrt(var_256(z) + eps2) --
#   i.e. LayerNorm -> Linear -> LayerNorm mapped through the documented affine image, not the full-memory kernel.
# =====================================================================================================
@pytest.mark.parametrize("row,C,Cm,N", [pytest.param(f"memproj_compact-C{C}-Cm{Cm}-N{N}", C, Cm, N, id=f"memproj_compact-C{C}-Cm{Cm}-N{N}")
                                        for C, Cm, N in ((64, 65, 60), (64, 72, 68), (64, 255, 132), (128, 129, 68), (128, 136, 60), (128, 255, 1028))])
def test_smm_memproj_compact(row, C, Cm, N):
    g = _g(6200 + C + Cm)
    B = 2
    x = _slice((B, C, 1, N), 4, g, 0.2, 1.5)
    g1, b1 = _rand((C,), g, 1.0, 0.5), _rand((C,), g, 0.0, 0.5)
    w, bias = _rand((256, C), g) / math.sqrt(C), _rand((256,), g, 0.0, 0.5)
    tok = x.double().cpu().reshape(B, C, N).permute(0, 2, 1)
    xhat = F.layer_norm(tok, (C,), g1.double(), b1.double(), EPS)
    z = F.linear(xhat, w.double(), bias.double())
    rstd = 1 / torch.sqrt(z.var(-1, unbiased=False) + EPS)
    ref = torch.zeros((B, Cm, N), dtype=torch.float64)
    ref[:, :C] = (xhat * rstd[..., None]).permute(0, 2, 1)
    ref[:, C] = rstd
    gram, hvec, evar = ops.memory_variance_form(w.to(DEV), bias.to(DEV))
    out = ops.smm_memproj_compact(x, g1.to(DEV), b1.to(DEV), gram, hvec, evar, Cm, EPS, EPS)
    _check(row, "compact memory", out, ref, MEM, (slice(None), slice(None), slice((N - 1) // MP_PX * MP_PX, None)))
    assert float(out[:, C + 1:].abs().max()) == 0.0 if Cm > C + 1 else True
    # the documented affine image: g2 * ((Wc xhat + bc) * rstd) + b2 = LayerNorm_256(z)
    Wc, bc = w.double() - w.double().mean(0, keepdim=True), bias.double() - bias.double().mean()
    img = torch.einsum('oc,bcn->bon', Wc, out[:, :C].double().cpu()) + bc[None, :, None] * out[:, C:C + 1].double().cpu()
    _check(row, "affine image", img, F.layer_norm(z, (256,), None, None, EPS).permute(0, 2, 1), MEM)


# =====================================================================================================
# idiff_time_mlp_fwd: time_mlp_kernel, grid (8, B), 32 outputs per workgroup (`n < nout`), nout <= 256, freqs NULL | table.
#   Formula: w2 . GELU(w0 . [sin(a) ; cos(a)] + b0) + b2 with a = t * f; the product t * f is the fp32 product (the kernel's
#   __fmul_rn, the CPU path's fp32 multiply) -- everything after it in fp64.  With freqs = NULL the device evaluates
#   f = exp(-ln(1e4) i / 31) itself in fp32: at t = 998 an fp32 rounding of f moves the angle by up to 998 * 2^-24 ~ 6e-5, hence the
#   2e-4 the existing time_embed test allows for device-side frequencies.
# =====================================================================================================
@pytest.mark.parametrize("table", [True, False], ids=["freq-table", "freq-null"])
@pytest.mark.parametrize("nout", [1, 64, 250, 256])
def test_time_mlp(nout, table):
    g = _g(6300 + nout)
    t = torch.tensor([0.0, 1.0, 37.0, 998.0])
    freq = torch.exp(torch.arange(32, dtype=torch.float32) * (-math.log(10000.0) / 31))
    w0, b0 = _rand((256, 64), g, 0.0, 0.1), _rand((256,), g, 0.0, 0.1)
    w2, b2 = _rand((nout, 256), g, 0.0, 0.1), _rand((nout,), g, 0.0, 0.1)
    a = (t[:, None] * freq[None]).double()
    ref = F.gelu(torch.cat([a.sin(), a.cos()], -1) @ w0.double().T + b0.double()) @ w2.double().T + b2.double()
    out = ops.time_mlp(t.to(DEV), freq.to(DEV) if table else None, w0.to(DEV), b0.to(DEV), w2.to(DEV), b2.to(DEV))
    row = f"time_mlp-nout{nout}-{'table' if table else 'null'}"
    _check(row, "temb", out, ref, LIN if table else 2e-4, (slice(None), slice((nout - 1) // 32 * 32, None)))


# =====================================================================================================
# 7. rejections: real device pointers, the documented return code, a message, no launch
# =====================================================================================================
def _buf(n=1 << 16):
    return torch.zeros((n,), device=DEV, dtype=torch.float32)


REJECT_ROWS = [
    ("attn_ctx-M33", E_BADARG, lambda L, b, s: L.idiff_attn_ctx_fwd(b, b, b, b, 1, 64, 16, 33, 1, 0.1, s)),
    ("attn_ctx-M0", E_BADARG, lambda L, b, s: L.idiff_attn_ctx_fwd(b, b, b, b, 1, 64, 16, 0, 1, 0.1, s)),
    ("attn_ctx-dh48", E_UNSUPPORTED, lambda L, b, s: L.idiff_attn_ctx_fwd(b, b, b, b, 1, 48, 16, 4, 1, 0.1, s)),
    ("attn_tokens-M65", E_BADARG, lambda L, b, s: L.idiff_attn_tokens_fwd(b, b, b, b, 1, 4, 65, 64, 1, 0.1, 64, 64, s)),
    ("attn_tokens-ldq-below-C", E_BADARG, lambda L, b, s: L.idiff_attn_tokens_fwd(b, b, b, b, 1, 4, 4, 64, 1, 0.1, 63, 64, s)),
    ("attn_self-dh48", E_BADARG, lambda L, b, s: L.idiff_attn_self_fwd(b, b, None, 1, 48, 64, 1, 0.1, s)),
    ("attn_self-N30-not-multiple-of-4", E_BADARG, lambda L, b, s: L.idiff_attn_self_fwd(b, b, None, 1, 64, 30, 1, 0.1, s)),
    ("smm_xattn-Cm100", E_BADARG, lambda L, b, s: L.idiff_smm_xattn_fwd(b, b, b, b, 1, 5, 4, 100, 64, 0.1, s)),
    ("smm_xattn-rows33", E_BADARG, lambda L, b, s: L.idiff_smm_xattn_fwd(b, b, b, b, 1, 11, 3, 72, 64, 0.1, s)),
    ("smm_xattn-N30-not-multiple-of-4", E_BADARG, lambda L, b, s: L.idiff_smm_xattn_fwd(b, b, b, b, 1, 5, 4, 72, 30, 0.1, s)),
    ("affine_silu_add-a-without-b", E_BADARG, lambda L, b, s: L.idiff_affine_silu_add(b, 64, b, None, None, 0, None, b, 64, 1, 1, 64, s)),
    ("gn_finalize-cpg257", E_BADARG, lambda L, b, s: L.idiff_gn_finalize(b, 1, 1, 257, 1, 16, b, b, None, 0, 1e-5, b, b, None, s)),
    ("linear_fwd-ldx-below-K", E_BADARG, lambda L, b, s: L.idiff_linear_fwd(b, 7, b, 8, None, None, 0, None, b, 8, 2, 8, 8, 0, 0, s)),
    ("linear_t-K8193", E_BADARG, lambda L, b, s: L.idiff_linear_t_fwd(b, 8193, b, 4, None, None, 0, None, b, 4, 1, 8193, 4, 0, 0, s)),
    ("linear_t-K8192-more-LDS-than-a-workgroup-has", E_UNSUPPORTED, lambda L, b, s: L.idiff_linear_t_fwd(b, 8192, b, 4, None, None, 0, None, b, 4, 1, 8192, 4, 0, 0, s)),
    ("linear_t-K4865-vector-LDS-above-160K", E_UNSUPPORTED, lambda L, b, s: L.idiff_linear_t_fwd(b, 4865, b, 4, None, None, 0, None, b, 4, 1, 4865, 4, 0, 0, s)),
    ("linear_t_ln-null-beta", E_BADARG, lambda L, b, s: L.idiff_linear_t_ln_fwd(b, 8, b, None, 1e-5, b, 4, None, None, 0, None, b, 4, 1, 8, 4, 0, s)),
    ("scoremap-K9", E_BADARG, lambda L, b, s: L.idiff_scoremap_fwd(b, 64 * 16, b, b, None, None, 1, 16, 64, 9, s)),
    ("scoremap-K0", E_BADARG, lambda L, b, s: L.idiff_scoremap_fwd(b, 64 * 16, b, b, None, None, 1, 16, 64, 0, s)),
    ("smm_memproj-C514", E_BADARG, lambda L, b, s: L.idiff_smm_memproj_fwd(b, 514 * 64, b, b, b, b, b, b, b, 1, 514, 64, 1e-5, s)),
    ("smm_memproj-C65-odd", E_BADARG, lambda L, b, s: L.idiff_smm_memproj_fwd(b, 65 * 64, b, b, b, b, b, b, b, 1, 65, 64, 1e-5, s)),
    ("smm_memproj-N62-not-multiple-of-4", E_BADARG, lambda L, b, s: L.idiff_smm_memproj_fwd(b, 64 * 62, b, b, b, b, b, b, b, 1, 64, 62, 1e-5, s)),
    ("smm_memproj_compact-C96", E_BADARG, lambda L, b, s: L.idiff_smm_memproj_compact_fwd(b, 96 * 64, b, b, b, b, 0.1, b, 1, 96, 64, 136, 1e-5, 1e-5, s)),
    ("smm_memproj_compact-Cm-equals-C", E_BADARG, lambda L, b, s: L.idiff_smm_memproj_compact_fwd(b, 64 * 64, b, b, b, b, 0.1, b, 1, 64, 64, 64, 1e-5, 1e-5, s)),
    ("time_mlp-nout257", E_BADARG, lambda L, b, s: L.idiff_time_mlp_fwd(b, None, b, b, b, b, b, 1, 64, 256, 257, s)),
    ("time_mlp-hid128", E_BADARG, lambda L, b, s: L.idiff_time_mlp_fwd(b, None, b, b, b, b, b, 1, 64, 128, 64, s)),
]


@pytest.mark.parametrize("row,code,call", [pytest.param(*r, id="reject-" + r[0]) for r in REJECT_ROWS])
def test_rejections(row, code, call):
    buf = _buf()
    torch.cuda.synchronize()
    _rejects(lambda L: call(L, _p(buf), _stream()), code)


def test_attn_tokens_grouped_rejects_17_groups():
    buf = _buf()
    n = _lib.LINEAR_MAX_GROUPS + 1
    arr = (ctypes.c_void_p * n)(*([buf.data_ptr()] * n))
    _rejects(lambda L: L.idiff_attn_tokens_grouped_fwd(arr, arr, arr, arr, n, 1, 4, 4, 64, 1, 0.1, 64, 64, _stream()), E_BADARG)
