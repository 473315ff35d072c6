"""The opt-in bf16-operand 3x3 convs (IDIFF_CONV_ALGO_BF16, csrc/conv_bf16.hip, csrc/conv_bf16_wgrad.hip) against their numerics
contract: operands gathered in fp32 as the f32 kernels gather them (concat, x2 upsample, prologue, zero padding), each operand and
weight rounded once to bf16 (nearest even), products summed in fp32, fp32 epilogue.  The oracle helpers (bf16 rounding, float64
convs) live here."""
import collections
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instancediff_amd import _lib, ops, pipeline, train_ops  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = ops.CONV_ALGO_BF16


# ---- oracle helpers ---------------------------------------------------------------------------------------------------------------
def rne_bf16(t):
    """fp32 -> bf16 (round to nearest even) -> float64"""
    return t.float().to(torch.bfloat16).double()


def gather(src0, src1, mode, pro):
    """the conv's input operand X~ in fp32 (CPU): prologue silu(a*x+b) on src0, virtual concat, nearest x2 upsample"""
    x = src0.float().cpu()
    if pro is not None:
        a, b = pro[0].cpu()[:, :, None, None], pro[1].cpu()[:, :, None, None]
        x = F.silu(a * x + b)
    if src1 is not None:
        x = torch.cat([x, src1.float().cpu()], 1)
    if mode == ops.CONV_UPSAMPLE2:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return x


def conv64(x, w):
    return F.conv2d(x.double(), w.double(), padding=1)


def wgrad64(x, dy, wshape):
    return torch.nn.grad.conv2d_weight(x.double(), wshape, dy.double(), padding=1)


def ints(*shape, g):
    return torch.randint(-2, 3, shape, generator=g).float()


def fwd_bf16(src0, w, bias=None, src1=None, mode=ops.CONV_NORMAL, **kw):
    wpk = ops.pack_conv_weight(w.to(DEV).contiguous(), bf16=True)
    return ops.conv2d(src0, wpk, bias, 3, w.shape[0], src1=src1, mode=mode, operands="bf16", **kw)


def dgrad_bf16(dy, w):
    wT = ops.pack_conv_weight(w.to(DEV).contiguous(), transpose=True, bf16=True)
    return ops.conv2d(dy, wT, None, 3, w.shape[1], operands="bf16")


def lib():
    return _lib.load()


# (mode, C0, C1, Cout, Hin, Win): the UNet's channel counts, skip concats, non-square images
SHAPES = [
    (ops.CONV_NORMAL, 64, 0, 64, 32, 32),
    (ops.CONV_NORMAL, 128, 0, 128, 16, 64),
    (ops.CONV_NORMAL, 256, 256, 256, 8, 32),
    (ops.CONV_NORMAL, 128, 64, 64, 24, 32),
    (ops.CONV_NORMAL, 64, 0, 128, 40, 96),
    (ops.CONV_UPSAMPLE2, 256, 0, 256, 8, 16),
    (ops.CONV_UPSAMPLE2, 128, 0, 64, 16, 32),
]


# ---- 1. exact indexing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,C0,C1,Cout,H,W", SHAPES)
def test_exact_integer_operands(mode, C0, C1, Cout, H, W):
    """integer operands in [-2, 2]: every product and partial sum is exact in fp32 and bf16, so forward, data gradient and weight
    gradient equal the float64 conv bit for bit"""
    g = torch.Generator().manual_seed(C0 * 7 + Cout + H + mode)
    B = 2
    s0 = ints(B, C0, H, W, g=g)
    s1 = ints(B, C1, H, W, g=g) if C1 else None
    w = ints(Cout, C0 + C1, 3, 3, g=g)
    x = gather(s0, s1, mode, None)
    Ho, Wo = x.shape[2:]
    y = fwd_bf16(s0.to(DEV), w, src1=None if s1 is None else s1.to(DEV), mode=mode)
    assert lib().idiff_conv2d_last_algo() == BF16
    assert torch.equal(y.cpu(), conv64(x, w).float())
    dy = ints(B, Cout, Ho, Wo, g=g)
    if (C0 + C1) % 64 == 0:  # data gradient: the same kernel on dy with the transposed image (Cout' = Cin)
        dx = dgrad_bf16(dy.to(DEV), w)
        assert lib().idiff_conv2d_last_algo() == BF16
        assert torch.equal(dx.cpu(), F.conv_transpose2d(dy.double(), w.double(), padding=1).float())
    dw = train_ops.conv2d_wgrad(s0.to(DEV), None if s1 is None else s1.to(DEV), mode, 3, dy.to(DEV), C0 + C1, operands="bf16")
    assert lib().idiff_conv2d_wgrad_last_algo() == BF16
    assert torch.equal(dw.cpu(), wgrad64(x, dy, w.shape).float())
    # accumulate: dw += the gradient
    dw2 = dw.clone()
    train_ops.conv2d_wgrad(s0.to(DEV), None if s1 is None else s1.to(DEV), mode, 3, dy.to(DEV), C0 + C1, dw=dw2, accumulate=True, operands="bf16")
    assert torch.equal(dw2.cpu(), 2 * wgrad64(x, dy, w.shape).float())


# ---- 2. rounding point --------------------------------------------------------------------------------------------------------------
def _contract_checks(got, xr, wr, x, w, extra, what):
    """max|got - ref_bf16| <= 5e-5 (|W~| * |X~|) (+ the fp32 epilogue's own rounding); rms(got - ref_bf16) <= 0.05 rms(ref_bf16 - ref_f64)"""
    ref_bf16 = conv64(xr, wr) + extra
    ref_f64 = conv64(x, w) + extra
    absconv = conv64(xr.abs(), wr.abs())
    err = (got.double() - ref_bf16).abs()
    assert (err <= 5e-5 * absconv + 4e-7 * ref_bf16.abs() + 1e-30).all(), (what, float((err - 5e-5 * absconv).max()))
    rms_err = float(err.pow(2).mean().sqrt())
    rms_rnd = float((ref_bf16 - ref_f64).pow(2).mean().sqrt())
    assert rms_err <= 0.05 * rms_rnd, (what, rms_err, rms_rnd)
    return rms_err, rms_rnd


@pytest.mark.parametrize("mode,C0,C1,Cout,H,W,prologue", [
    (ops.CONV_NORMAL, 64, 0, 64, 32, 64, True),
    (ops.CONV_NORMAL, 128, 0, 128, 16, 32, True),
    (ops.CONV_NORMAL, 256, 128, 128, 8, 32, False),
    (ops.CONV_UPSAMPLE2, 256, 0, 128, 8, 16, True),
])
def test_rounding_after_the_prologue(mode, C0, C1, Cout, H, W, prologue):
    g = torch.Generator().manual_seed(C0 + Cout + H + 31 * mode)
    B = 2
    s0 = torch.randn(B, C0, H, W, generator=g)
    s1 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    pro = (1.0 + 0.5 * torch.randn(B, C0, generator=g), 0.3 * torch.randn(B, C0, generator=g)) if prologue else None
    w = 0.05 * torch.randn(Cout, C0 + C1, 3, 3, generator=g)
    x = gather(s0, s1, mode, pro)
    Ho, Wo = x.shape[2:]
    bias = torch.randn(Cout, generator=g)
    vec = torch.randn(B, Cout, generator=g)
    res = torch.randn(B, Cout, Ho, Wo, generator=g)
    aux = torch.randn(B, Cout, Ho, Wo, generator=g)
    aa, ab = torch.randn(B, Cout, generator=g), torch.randn(B, Cout, generator=g)
    d = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    y, stats = fwd_bf16(d(s0), w, bias=d(bias), src1=d(s1), mode=mode, pro=None if pro is None else (d(pro[0]), d(pro[1])), res=d(res),
                        vec=d(vec), aux=(d(aux), d(aa), d(ab)), want_stats=True)
    assert lib().idiff_conv2d_last_algo() == BF16
    extra = (bias[None, :, None, None] + vec[:, :, None, None] + res + F.silu(aa[:, :, None, None] * aux + ab[:, :, None, None])).double()
    xr, wr = rne_bf16(x), rne_bf16(w)
    _contract_checks(y.cpu(), xr, wr, x, w, extra, "forward")
    # GroupNorm partials of acc + bias: against float64 sums of the stored output of a call with bias only
    y2, st2 = fwd_bf16(d(s0), w, bias=d(bias), src1=d(s1), mode=mode, pro=None if pro is None else (d(pro[0]), d(pro[1])), want_stats=True)
    assert tuple(st2.shape) == (B, lib().idiff_conv2d_num_tiles(Ho, Wo), Cout, 2)
    tot = st2.double().sum(1).cpu()
    y64 = y2.double().cpu()
    s_ref, q_ref = y64.sum((2, 3)), y64.pow(2).sum((2, 3))
    assert ((tot[..., 0] - s_ref).abs() <= 1e-5 * y64.abs().sum((2, 3)) + 1e-6).all()
    assert ((tot[..., 1] - q_ref).abs() <= 1e-5 * q_ref + 1e-6).all()
    # weight gradient: dW = sum bf16(dY) bf16(X~) in fp32
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    dw = train_ops.conv2d_wgrad(d(s0), d(s1), mode, 3, d(dy), C0 + C1, pro=None if pro is None else (d(pro[0]), d(pro[1])), operands="bf16")
    assert lib().idiff_conv2d_wgrad_last_algo() == BF16
    ref_bf16, ref_f64 = wgrad64(xr, rne_bf16(dy), w.shape), wgrad64(x, dy, w.shape)
    absg = wgrad64(xr.abs(), rne_bf16(dy).abs(), w.shape)
    err = (dw.cpu().double() - ref_bf16).abs()
    assert (err <= 5e-5 * absg).all(), float((err - 5e-5 * absg).max())
    assert float(err.pow(2).mean().sqrt()) <= 0.05 * float((ref_bf16 - ref_f64).pow(2).mean().sqrt())


# ---- 3. selection and fallback ------------------------------------------------------------------------------------------------------
def test_non_tiling_layers_fall_back_and_hard_requests_raise():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 32, 32, generator=g).to(DEV)
    w5 = (0.05 * torch.randn(5, 64, 3, 3, generator=g)).to(DEV)  # the 5-channel output conv: Cout % 64 != 0
    y_bf = fwd_bf16(x, w5)
    assert lib().idiff_conv2d_last_algo() != BF16
    y_f32 = ops.conv2d(x, ops.pack_conv_weight(w5), None, 3, 5)
    assert torch.equal(y_bf, y_f32)
    with pytest.raises(_lib.IdiffError):
        ops.conv2d(x, ops.pack_conv_weight(w5, bf16=True), None, 3, 5, algo=BF16)
    w = (0.05 * torch.randn(64, 64, 3, 3, generator=g)).to(DEV)
    x16 = torch.randn(2, 64, 16, 16, generator=g).to(DEV)  # Wout % 32 != 0
    fwd_bf16(x16, w)
    assert lib().idiff_conv2d_last_algo() != BF16
    with pytest.raises(_lib.IdiffError):
        ops.conv2d(x16, ops.pack_conv_weight(w, bf16=True), None, 3, 64, algo=BF16)
    train_ops.conv2d_wgrad(x16, None, ops.CONV_NORMAL, 3, torch.randn(2, 64, 16, 16, device=DEV), 64, operands="bf16")
    assert lib().idiff_conv2d_wgrad_last_algo() != BF16
    # an eligible layer with operands f32 (the default) and a bf16 image present stays on the fp32 kernels, same bits as without it
    x32 = torch.randn(2, 64, 32, 32, generator=g).to(DEV)
    y0 = ops.conv2d(x32, ops.pack_conv_weight(w), None, 3, 64)
    a0 = lib().idiff_conv2d_last_algo()
    y1 = ops.conv2d(x32, ops.pack_conv_weight(w, bf16=True), None, 3, 64)
    assert a0 != BF16 and lib().idiff_conv2d_last_algo() == a0 and torch.equal(y0, y1)
    # ... and by name it runs
    ops.conv2d(x32, ops.pack_conv_weight(w, bf16=True), None, 3, 64, algo=BF16)
    assert lib().idiff_conv2d_last_algo() == BF16
    train_ops.conv2d_wgrad(x32, None, ops.CONV_NORMAL, 3, torch.randn(2, 64, 32, 32, device=DEV), 64)
    assert lib().idiff_conv2d_wgrad_last_algo() != BF16
    with pytest.raises(ValueError):
        with ops.conv_operands("fp16"):
            pass


def test_default_model_never_selects_bf16():
    """operands == 0 everywhere: a whole sampling step and a training iteration of the default (f32) model trace no BF16 launch"""
    model, sde = pipeline.build(phase="train", device=torch.device(DEV), T=4, seed=0, score_map_dropout=0)
    assert model.conv_dtype == "f32"
    batch = make_batch(2, 64, seed=3)
    ops.ALGO_TRACE = collections.Counter()
    try:
        model.feed_data(batch)
        loss, _ = model.optimize_parameters_inputRes()
        model.set_eval()
        sde.hip_graph = False
        model.test()
        trace = ops.ALGO_TRACE
    finally:
        ops.ALGO_TRACE = None
    assert torch.isfinite(torch.as_tensor(float(loss)))
    assert trace and not any(k[0] == BF16 for k in trace), trace


# ---- 4. determinism and batch invariance --------------------------------------------------------------------------------------------
def test_deterministic_and_batch_invariant():
    g = torch.Generator().manual_seed(9)
    B = 4
    x = torch.randn(B, 128, 32, 64, generator=g).to(DEV)
    pa, pb = (1 + 0.3 * torch.randn(B, 128, generator=g)).to(DEV), (0.2 * torch.randn(B, 128, generator=g)).to(DEV)
    w = (0.05 * torch.randn(128, 128, 3, 3, generator=g)).to(DEV)
    dy = torch.randn(B, 128, 32, 64, generator=g).to(DEV)
    y1 = fwd_bf16(x, w, pro=(pa, pb))
    y2 = fwd_bf16(x, w, pro=(pa, pb))
    assert torch.equal(y1, y2)
    for b in range(B):
        yb = fwd_bf16(x[b:b + 1].contiguous(), w, pro=(pa[b:b + 1].contiguous(), pb[b:b + 1].contiguous()))
        assert torch.equal(yb, y1[b:b + 1])
    d1, d2 = dgrad_bf16(dy, w), dgrad_bf16(dy, w)
    assert torch.equal(d1, d2)
    assert torch.equal(dgrad_bf16(dy[1:2].contiguous(), w), d1[1:2])
    wg = lambda xx, dd, pp: train_ops.conv2d_wgrad(xx, None, ops.CONV_NORMAL, 3, dd, 128, pro=pp, operands="bf16")  # noqa: E731
    g1, g2 = wg(x, dy, (pa, pb)), wg(x, dy, (pa, pb))
    assert torch.equal(g1, g2)
    # 32x64 = 2048 pixels: one K-block per sample, so dW(B) is the fp32 sum, in sample order, of the per-sample gradients -- the
    # result does not depend on how the batch is split over workgroups
    parts = [wg(x[b:b + 1].contiguous(), dy[b:b + 1].contiguous(), (pa[b:b + 1].contiguous(), pb[b:b + 1].contiguous())) for b in range(B)]
    acc = torch.zeros_like(parts[0])
    for p in parts:
        acc = acc + p
    assert torch.equal(acc, g1)
    # a 128x128 image has four K-blocks per sample: still reproducible
    xl = torch.randn(2, 64, 128, 128, generator=g).to(DEV)
    dl = torch.randn(2, 64, 128, 128, generator=g).to(DEV)
    a1 = train_ops.conv2d_wgrad(xl, None, ops.CONV_NORMAL, 3, dl, 64, operands="bf16")
    a2 = train_ops.conv2d_wgrad(xl, None, ops.CONV_NORMAL, 3, dl, 64, operands="bf16")
    assert lib().idiff_conv2d_wgrad_last_algo() == BF16 and torch.equal(a1, a2)


# ---- 5. sampling chain --------------------------------------------------------------------------------------------------------------
def _eligible(cin, cout, hout, wout):
    return cout % 64 == 0 and cin % 32 == 0 and hout % 8 == 0 and wout % 32 == 0


# measured on the MI355X: max |x_bf16 - x_f32| of this chain = 1.47e-2 (mean 1.59e-3); the bound is twice that
SAMPLING_MEASURED = 1.4678e-2
SAMPLING_BOUND = 2 * SAMPLING_MEASURED


def test_sampling_chain_bf16():
    T, B, H = 50, 4, 64
    batch = make_batch(B, H, seed=21)
    g = torch.Generator().manual_seed(22)
    x_T = batch['input'] + 0.4 * torch.randn(batch['input'].shape, generator=g)
    noises = torch.randn((T,) + tuple(batch['input'].shape), generator=g)
    outs = {}
    trace = None
    for kind, use_graph in (("bf16", True), ("bf16", False), ("f32", True)):
        model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, conv_dtype=kind)
        model.set_eval()
        sde.hip_graph = use_graph
        model.feed_data(batch)
        if kind == "bf16" and use_graph:
            ops.ALGO_TRACE = collections.Counter()
        try:
            model.test(x_T=x_T.to(DEV), noises=noises.to(DEV))
            if ops.ALGO_TRACE is not None:
                trace = ops.ALGO_TRACE
            # the graph run must really have replayed a captured graph (a failed capture falls back to eager steps)
            assert sde.last_mode == ("graph" if use_graph else "eager"), (kind, use_graph, sde.last_mode)
        finally:
            ops.ALGO_TRACE = None
        outs[(kind, use_graph)] = torch.from_numpy(model.get_visuals()).clone()
    xb, xe, xf = outs[("bf16", True)], outs[("bf16", False)], outs[("f32", True)]
    assert torch.isfinite(xb).all()
    assert torch.equal(xb, xe), "graph replay differs from the eager steps"
    three = [k for k in trace if k[1] == 3]
    assert any(k[0] == BF16 for k in three)
    for k in three:
        if _eligible(k[2], k[3], k[4], k[5]):
            assert k[0] == BF16, k
    diff = (xb - xf).abs()
    print(f"bf16 vs f32 chain (c1 shape, {T} steps): max |dx| = {float(diff.max()):.4e}, mean |dx| = {float(diff.mean()):.4e}")
    assert float(diff.max()) > 0, "the bf16 mode computed the fp32 result"
    assert float(diff.max()) < SAMPLING_BOUND


# ---- 6. training --------------------------------------------------------------------------------------------------------------------
# measured on the MI355X: the lowest cosine similarity of a conv weight's bf16-mode gradient to its fp32-mode gradient = 0.999850;
# the bound leaves twice the measured distance from 1
GRAD_COS_MEASURED = 0.999850
GRAD_COS_BOUND = 1 - 2 * (1 - GRAD_COS_MEASURED)


def test_training_bf16():
    model, sde = pipeline.build(phase="train", device=torch.device(DEV), T=100, seed=0, score_map_dropout=0, conv_dtype="bf16")
    assert model.conv_dtype == "bf16" and model.drift_net.conv_dtype == "bf16"
    batch = make_batch(2, 64, seed=8)
    model.feed_data(batch)
    # conv weight gradients of the drift net, bf16 vs f32 mode, same inputs and output gradient
    net = model.drift_net
    convs = [m.weight for m in net.modules() if isinstance(m, nn.Conv2d)]
    g = torch.Generator().manual_seed(4)
    xa = torch.randn(2, 1, 64, 64, generator=g).to(DEV)
    xb = torch.randn(2, 1, 64, 64, generator=g).to(DEV)
    t = torch.tensor([10.0, 60.0], device=DEV)
    ctx = batch['A_emb'].to(DEV)
    grads = {}
    for kind in ("f32", "bf16"):
        net.conv_dtype = kind
        try:
            ops.ALGO_TRACE = collections.Counter()
            with torch.enable_grad():
                out = net(xa, xb, t, batch['names'], model.text_encoder, image_context=ctx)
            fwd_trace = ops.ALGO_TRACE
            # the backward (autograd may run it on another thread, outside any conv_operands scope): data-gradient convs in
            # ALGO_TRACE, weight gradients in WGRAD_TRACE
            ops.ALGO_TRACE, ops.WGRAD_TRACE = collections.Counter(), collections.Counter()
            pred = out[0] if isinstance(out, tuple) else out
            gout = torch.randn(pred.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
            gr = torch.autograd.grad(pred, convs, grad_outputs=gout, allow_unused=True)
            torch.cuda.synchronize()
            dgrad_trace, wgrad_trace = ops.ALGO_TRACE, ops.WGRAD_TRACE
        finally:
            ops.ALGO_TRACE = ops.WGRAD_TRACE = None
        for what, tr in (("forward", fwd_trace), ("data gradient", dgrad_trace), ("weight gradient", wgrad_trace)):
            assert tr, what
            assert any(k[0] == BF16 for k in tr) == (kind == "bf16"), (kind, what, tr)
        if kind == "bf16":  # every eligible 3x3 weight gradient ran in bf16
            for k in wgrad_trace:
                if k[1] == 3 and _eligible(k[2], k[3], k[4], k[5]):
                    assert k[0] == BF16, k
        grads[kind] = gr
    net.conv_dtype = "bf16"
    worst = 1.0
    for a, b in zip(grads["f32"], grads["bf16"]):
        if a is None or float(a.norm()) == 0:
            continue
        assert torch.isfinite(b).all()
        cos = float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))
        worst = min(worst, cos)
    print(f"lowest cosine similarity of a conv weight gradient, bf16 vs f32 mode: {worst:.6f}")
    assert worst >= GRAD_COS_BOUND, worst
    # the loss falls over 20 iterations on a fixed batch
    losses = []
    for _ in range(20):
        loss, _ = model.optimize_parameters_inputRes()
        losses.append(float(loss))
    print("bf16 training losses:", [f"{v:.4f}" for v in losses])
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sum(losses[-3:]) < sum(losses[:3]), losses
