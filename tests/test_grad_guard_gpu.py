"""Gradient guard on the GPU: idiff_grad_sumsq / idiff_grad_guard / idiff_adam_step_dev through the C ABI against fp64 torch on the same
data, then FusedAdam(max_grad_norm=...) against clip_grad_norm_ + torch.optim.Adam in fp64, then the model's training step.

Tolerances are test_train_kernels_gpu's: 1e-5 relative for reductions under 65 536 terms, RED = 5e-5 from there up (fp32 accumulation;
the norm halves the sum's relative error, so the bound is loose by that much).  Flags and the unclipped coefficient are exact."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, pipeline, train_ops as T  # noqa: E402
from instancediff_amd.ops import _p, _stream  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
RED = 5e-5  # reductions over >= 65 536 terms
BADARG = -1  # IDIFF_E_BADARG
HYPER = (2e-3, 0.9, 0.99, 1e-8)  # lr, beta1, beta2, eps


def _tol(n):
    return RED if n >= 65536 else 1e-5


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _parts():
    return int(_lib.load().idiff_grad_sumsq_parts())


def _guard(bufs, scale=1.0, max_norm=0.0, skip=0):
    """-> (part, info) of idiff_grad_sumsq per buffer + one idiff_grad_guard; both start from a sentinel"""
    lib, P = _lib.load(), _parts()
    part = torch.full((len(bufs) * P,), -7.0, device=DEV)
    info = torch.full((4,), -7.0, device=DEV)
    for k, b in enumerate(bufs):
        assert lib.idiff_grad_sumsq(_p(b), b.numel(), part.data_ptr() + 4 * k * P, _stream()) == 0
    assert lib.idiff_grad_guard(_p(part), len(bufs), scale, max_norm, skip, _p(info), _stream()) == 0
    return part, info


def _coef_ref(max_norm, norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _close(got, ref, tol, what):
    e = abs(got - ref) / max(abs(ref), 1e-30)
    print(f"{what}: got {got!r} ref {ref!r} rel {e:.2e} (tol {tol:.0e})")
    assert e <= tol, (what, got, ref, e)


def test_parts_is_the_documented_constant():
    assert _parts() == 1024


def _norm_sizes():
    return [1, 3, 255, 1027, 65537, 2 * (1024 * 256 * 4) + 37]


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", _norm_sizes())
def test_norm_and_coef_vs_fp64(n, scale):
    """the last size makes every thread of the fixed grid loop twice and leaves a tail of one float4 + 1 element"""
    assert _norm_sizes()[-1] == 2 * (_parts() * 256 * 4) + 37
    g = torch.randn(n, generator=_g(100 + n % 997)).to(DEV)
    ref = abs(scale) * float(g.double().norm())
    tol = _tol(n)
    part, info = _guard([g], scale)
    host = info.cpu().tolist()
    _close(host[0], ref, tol, f"n{n} norm")
    assert host[1:] == [1.0, 1.0, 0.0], host  # clipping off: coef exactly 1
    sq = (g.double() ** 2).sum()
    _close(float(part.double().sum()), float(sq), 2 * tol, f"n{n} sum of partials")
    assert float(part.min()) >= 0.0  # every partial was written (the sentinel is negative); empty workgroups wrote 0
    if n < 4 * 256:
        assert float(part[1:].abs().max()) == 0.0
    for factor in (0.5, 2.0):
        mx = factor * ref
        host = _guard([g], scale, mx)[1].cpu().tolist()
        _close(host[0], ref, tol, f"n{n} norm (max_norm {factor} |g|)")
        if factor > 1:
            assert host[1] == 1.0, host
        else:
            _close(host[1], _coef_ref(float(torch.tensor(mx, dtype=torch.float32)), ref), tol, f"n{n} coef")
        assert host[2:] == [1.0, 0.0], host
    # a negative scale (never used by the optimizer) still gives a norm
    assert _guard([g], -scale)[1].cpu().tolist()[0] == _guard([g], scale)[1].cpu().tolist()[0]


def test_norm_of_mixed_magnitudes():
    n = 65537
    g = torch.randn(n, generator=_g(5))
    g[:n // 4] *= 1e3
    g[n // 4:] *= 1e-3
    g = g.to(DEV)
    ref = float(g.double().norm())
    host = _guard([g], 1.0, 0.5 * ref)[1].cpu().tolist()
    _close(host[0], ref, _tol(n), "mixed norm")
    _close(host[1], _coef_ref(float(torch.tensor(0.5 * ref, dtype=torch.float32)), ref), _tol(n), "mixed coef")
    assert host[2:] == [1.0, 0.0]


def test_two_calls_give_identical_bits():
    g = torch.randn(2 * (1024 * 256 * 4) + 37, generator=_g(6)).to(DEV)
    p1, i1 = _guard([g], 0.125, 3.0)
    p2, i2 = _guard([g], 0.125, 3.0)
    assert torch.equal(p1, p2) and torch.equal(i1, i2)


def test_two_buffers_give_the_norm_of_the_concatenation():
    a = torch.randn(1027, generator=_g(7)).to(DEV)
    b = 3.0 * torch.randn(65537, generator=_g(8)).to(DEV)
    ref = float(torch.cat([a, b]).double().norm())
    host = _guard([a, b], 1.0, 0.25 * ref)[1].cpu().tolist()
    _close(host[0], ref, RED, "nbuf=2 norm")
    _close(host[1], _coef_ref(float(torch.tensor(0.25 * ref, dtype=torch.float32)), ref), RED, "nbuf=2 coef")
    assert host[2:] == [1.0, 0.0]
    one = _guard([b], 1.0)[1].cpu().tolist()[0]
    assert host[0] > one  # the first buffer's range was read too


def _adam(entry, p, g, m, v, wd, scale, step, info=None):
    lr, b1, b2, eps = HYPER
    lib = _lib.load()
    if info is None:
        return lib.idiff_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, wd, scale, step, _stream())
    return lib.idiff_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, wd, scale, step, _p(info), _stream())


def _state(n, seed):
    g = _g(seed)
    p = torch.randn(n, generator=g).to(DEV)
    m = (0.1 * torch.randn(n, generator=g)).to(DEV)
    v = (0.01 * torch.rand(n, generator=g)).to(DEV)
    gr = torch.randn(n, generator=g).to(DEV)
    return p, gr, m, v


N_BAD = 65539  # 16 384 float4s (the last one belongs to thread 255 of workgroup 63) + a tail of 3


@pytest.mark.parametrize("pos", [pytest.param(0, id="first"), pytest.param(N_BAD // 4 * 4 - 1, id="last-of-body"), pytest.param(N_BAD - 1, id="tail")])
@pytest.mark.parametrize("bad", [pytest.param(math.nan, id="nan"), pytest.param(math.inf, id="inf")])
def test_nonfinite_gradient(bad, pos):
    p, gr, m, v = _state(N_BAD, 11)
    gr[pos] = bad
    # skip on: the record says "not applied" and the step leaves everything as it was
    info = _guard([gr], 1.0, 1.0, skip=1)[1]
    host = info.cpu().tolist()
    assert host[2] == 0.0 and host[3] == 0.0, host
    assert math.isnan(host[0]) if math.isnan(bad) else host[0] == math.inf
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    assert _adam("dev", p, gr, m, v, 1e-2, 1.0, 2, info) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
    # skip off: applied, with clip_grad_norm_'s coefficient (0 for an inf norm, NaN for a NaN norm)
    host = _guard([gr], 1.0, 1.0, skip=0)[1].cpu().tolist()
    assert host[2] == 1.0 and host[3] == 0.0, host
    assert math.isnan(host[1]) if math.isnan(bad) else host[1] == 0.0, host
    # and skip on without clipping still skips
    assert _guard([gr], 1.0, 0.0, skip=1)[1].cpu().tolist()[1:] == [1.0, 0.0, 0.0]


def test_overflowing_sum_of_squares_counts_as_nonfinite():
    gr = torch.full((1027,), 3e19, device=DEV)  # finite elements, 9e38 per square: inf in fp32
    host = _guard([gr], 1.0, 0.0, skip=1)[1].cpu().tolist()
    assert host[0] == math.inf and host[2] == 0.0, host


@pytest.mark.parametrize("n,wd,scale", [pytest.param(255, 1e-2, 0.125, id="n255-wd"), pytest.param(255, 1e-2, 1.0 / 3.0, id="n255-wd-inexact-scale"),
                                        pytest.param(256 * 8192 + 37, 1e-2, 1.0, id="n-above-grid-cap")])
def test_unit_coef_is_adam_step_bit_for_bit(n, wd, scale):
    p, gr, m, v = _state(n, 21)
    q, mq, vq = p.clone(), m.clone(), v.clone()
    info = torch.tensor([123.0, 1.0, 1.0, 0.0], device=DEV)
    for step in (1, 2):
        assert _adam("plain", p, gr, m, v, wd, scale, step) == 0
        assert _adam("dev", q, gr, mq, vq, wd, scale, step, info) == 0
    assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq)
    assert not torch.equal(p, _state(n, 21)[0])  # and something happened


@pytest.mark.parametrize("n", [255, 1027])
def test_quarter_coef_is_adam_step_on_a_quarter_of_the_gradient(n):
    p, gr, m, v = _state(n, 22)
    q, mq, vq = p.clone(), m.clone(), v.clone()
    info = torch.tensor([0.0, 0.25, 1.0, 0.0], device=DEV)
    gq = 0.25 * gr  # exact
    for step in (1, 2):
        assert _adam("plain", p, gq, m, v, 1e-2, 1.0, step) == 0
        assert _adam("dev", q, gr, mq, vq, 1e-2, 1.0, step, info) == 0
    assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq)


def test_refusals_leave_the_outputs_untouched():
    lib, P = _lib.load(), _parts()
    buf = torch.randn(1028, generator=_g(31)).to(DEV)
    part = torch.full((P,), -7.0, device=DEV)
    launches = lib.idiff_launch_count()
    assert lib.idiff_grad_sumsq(buf.data_ptr() + 4, 1027, _p(part), _stream()) == BADARG  # misaligned
    assert lib.idiff_grad_sumsq(_p(buf), 0, _p(part), _stream()) == BADARG
    assert lib.idiff_grad_sumsq(None, 1027, _p(part), _stream()) == BADARG
    assert lib.idiff_grad_sumsq(_p(buf), 1027, None, _stream()) == BADARG
    info = torch.full((4,), -7.0, device=DEV)
    assert lib.idiff_grad_guard(None, 1, 1.0, 0.0, 0, _p(info), _stream()) == BADARG
    assert lib.idiff_grad_guard(_p(part), 0, 1.0, 0.0, 0, _p(info), _stream()) == BADARG
    assert lib.idiff_grad_guard(_p(part), 1, 1.0, 0.0, 0, None, _stream()) == BADARG
    p, gr, m, v = _state(1027, 32)
    p0, m0, v0, g0 = p.clone(), m.clone(), v.clone(), gr.clone()
    gr[100:104] = torch.tensor([0.0, 1.0, 1.0, 0.0])
    g0[100:104] = gr[100:104]
    lr, b1, b2, eps = HYPER
    for alias in (gr[100:104], gr[1023:], p[0:4], m[500:504], v[1020:1024]):  # info inside (or straddling the end of) a buffer
        assert lib.idiff_adam_step_dev(_p(p), _p(gr), _p(m), _p(v), 1027, lr, b1, b2, eps, 0.0, 1.0, 1, _p(alias), _stream()) == BADARG
    good = torch.tensor([0.0, 1.0, 1.0, 0.0], device=DEV)
    assert lib.idiff_adam_step_dev(_p(p), _p(gr), _p(m), _p(v), 0, lr, b1, b2, eps, 0.0, 1.0, 1, _p(good), _stream()) == BADARG
    assert lib.idiff_adam_step_dev(_p(p), _p(gr), _p(m), _p(v), 1027, lr, b1, b2, eps, 0.0, 1.0, 1, None, _stream()) == BADARG
    assert lib.idiff_adam_step_dev(None, _p(gr), _p(m), _p(v), 1027, lr, b1, b2, eps, 0.0, 1.0, 1, _p(good), _stream()) == BADARG
    torch.cuda.synchronize()
    assert lib.idiff_launch_count() == launches  # nothing was launched
    assert float(part.min()) == -7.0 and float(part.max()) == -7.0 and info.cpu().tolist() == [-7.0] * 4
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(gr, g0)


# =====================================================================================================
# the optimizer
# =====================================================================================================
def _check(row, name, got, ref, tol):
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    e = float((got - ref).abs().max()) / float(ref.abs().max().clamp_min(1e-12))
    print(f"{row} {name}: rel {e:.2e} (tol {tol:.1e})")
    assert e <= tol, (row, name, e, tol)


@pytest.mark.parametrize("n,wd", [pytest.param(255, 1e-2, id="n255"), pytest.param(65537, 0.0, id="n65537")])
def test_fused_adam_clips_like_clip_grad_norm(n, wd):
    """three steps, the second with a gradient a hundred times smaller: the clip is active, inactive, active.  p at test_adam_step's
    1e-6 (Adam's update does not see a common scale of g, up to eps); the moments at its 1e-5 plus the norm's own tolerance, since a
    relative error of the coefficient is a relative error of the clipped gradient (the large row runs without weight decay for the
    reason test_adam_step gives)."""
    row = f"clip-n{n}"
    g = _g(40 + n % 100)
    p0 = torch.randn(n, generator=g)
    c = 0.5 * math.sqrt(n)  # E|g| = sqrt(n) for the full-size gradients, a hundredth of it for the small one
    ref_p = p0.double().to(DEV).requires_grad_(True)
    ropt = torch.optim.Adam([ref_p], lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    pp = nn.Parameter(p0.clone().to(DEV))
    opt = T.FusedAdam([pp], lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, max_grad_norm=c)
    active = []
    for it in range(3):
        gr = (torch.randn(n, generator=g) * (0.01 if it == 1 else 1.0)).to(DEV)
        ref_p.grad = gr.double()
        total = float(torch.nn.utils.clip_grad_norm_([ref_p], c))
        ropt.step()
        opt.zero_grad()
        pp.grad = gr
        opt.step()
        info = opt.last_info.cpu().tolist()
        assert opt.settle(info) is False
        _close(info[0], total, _tol(n), f"{row} step {it} norm")
        _close(info[1], _coef_ref(c, total), _tol(n), f"{row} step {it} coef")
        assert info[2:] == [1.0, 0.0]
        active.append(info[1] < 1.0)
    assert active == [True, False, True], active
    assert opt._flat[0]["step"] == 3 and opt.skipped_steps == 0
    st, f = ropt.state[ref_p], opt._flat[0]
    _check(row, "exp_avg", f["m"], st["exp_avg"], 1e-5 + _tol(n))
    _check(row, "exp_avg_sq", f["v"], st["exp_avg_sq"], 1e-5 + _tol(n))
    _check(row, "p", pp.data, ref_p, 1e-6)


def test_unsettled_skipped_step_is_settled_by_the_next_step():
    pp = nn.Parameter(torch.randn(1027, generator=_g(50)).to(DEV))
    opt = T.FusedAdam([pp], lr=2e-3, skip_nonfinite=True)
    p0 = pp.data.clone()
    bad = torch.randn(1027, generator=_g(51)).to(DEV)
    bad[5] = math.nan
    pp.grad = bad
    opt.step()
    assert opt._flat[0]["step"] == 1  # advanced on the host, not yet settled
    assert torch.equal(pp.data, p0)
    opt.zero_grad()
    pp.grad = torch.randn(1027, generator=_g(52)).to(DEV)
    opt.step()  # settles the skipped one itself, then counts this one as step 1
    assert opt.skipped_steps == 1 and opt._flat[0]["step"] == 1
    assert opt.settle() is False and opt._flat[0]["step"] == 1
    assert bool(torch.isfinite(pp.data).all()) and not torch.equal(pp.data, p0)
    # the first applied step of Adam moves every element by lr * g / (|g| + eps): the bias corrections were those of step 1
    assert float((pp.data - p0).abs().max()) <= 2e-3 * (1 + 1e-5) + 2.0 ** -24 * float(p0.abs().max())
    assert opt.state_dict()["flat"][0]["skipped"] == 1


# =====================================================================================================
# the model's training step (32 x 32, batch 2, T = 20, injected t and eps)
# =====================================================================================================
@pytest.fixture(scope="module")
def fed():
    batch = make_batch(2, 32, seed=3)
    t = torch.tensor([[[[5]]], [[[17]]]])
    eps = torch.randn(batch['input'].shape, generator=_g(7))
    return batch, t, eps


def _model(**kw):
    model, sde = pipeline.build(phase="train", device=torch.device(DEV), T=20, seed=0, score_map_dropout=0.0, **kw)
    model.set_train()
    return model, sde


def _feed(model, sde, fed, seed_shift=0):
    batch, t, eps = fed
    model.input = batch['input'].to(DEV)
    model.target = batch['target'].to(DEV).clone()
    model.names = batch['names']
    model.A_emb = batch['A_emb'].to(DEV)
    e = eps if not seed_shift else torch.randn(eps.shape, generator=_g(7 + seed_shift))
    model.t, model.drift_noised_x, _, model.std_noise, _ = sde.forward_diffusion(model.target, model.input, t=t, eps=e.to(DEV))
    model.std_noise = model.std_noise.clone()


def _opt_state(model):
    return [x.clone() for o in (model.drift_optimizer, model.noise_optimizer) for x in (o._flat[0]["p"], o._flat[0]["m"], o._flat[0]["v"])]


def test_guard_that_never_clips_leaves_the_training_bits(fed):
    plain, sde_a = _model()
    clip, sde_b = _model(grad_clip_norm=1e30)
    assert not plain.drift_optimizer.guarded and clip.drift_optimizer.guarded and clip.noise_optimizer.guarded
    for it in range(2):
        _feed(plain, sde_a, fed, it)
        _feed(clip, sde_b, fed, it)
        la, _ = plain.optimize_parameters()
        lb, _ = clip.optimize_parameters()
        assert la == lb
    assert plain.grad_info is None and plain.get_grad_message() == ""
    for a, b in zip(_opt_state(plain), _opt_state(clip)):
        assert torch.equal(a, b)
    gi = clip.grad_info
    assert gi["skipped_steps"] == 0
    for key, o in (("drift", plain.drift_optimizer), ("noise", plain.noise_optimizer)):
        flat = o._flat[0]["g"]  # the last step's gradient, still in the flat buffer
        _close(gi[key]["norm"], float(flat.double().norm()), _tol(flat.numel()), f"{key} grad_info norm (n = {flat.numel()})")
        assert gi[key]["coef"] == 1.0 and gi[key]["skipped"] is False
    msg = clip.get_grad_message()
    assert "dgn=" in msg and "ngn=" in msg and "skipped=0" in msg
    assert clip.drift_optimizer._flat[0]["step"] == 2 and plain.drift_optimizer._flat[0]["step"] == 2


def test_tiny_clip_norm_bounds_the_update(fed):
    c = 1e-4
    model, sde = _model(grad_clip_norm=c)
    before = _opt_state(model)
    _feed(model, sde, fed)
    model.optimize_parameters()
    gi = model.grad_info
    for key, o, p0 in (("drift", model.drift_optimizer, before[0]), ("noise", model.noise_optimizer, before[3])):
        assert gi[key]["coef"] < 1.0 and gi[key]["skipped"] is False
        _close(gi[key]["coef"], _coef_ref(c, gi[key]["norm"]), 1e-6, f"{key} coef from its own norm")
        # the first Adam step: m / bc1 = gr, sqrt(v) / sqrt(bc2) = |gr|, so |dp| = lr |gr| / (|gr| + eps) <= lr for ANY gradient
        # gr = coef g + wd p; beyond that only the fp32 rounding of p itself (half an ulp) and of lr / bc1
        lr = o.param_groups[0]["lr"]
        p1 = o._flat[0]["p"]
        excess = (p1.double() - p0.double()).abs() - 2.0 ** -24 * p0.double().abs()
        assert float(excess.max()) <= lr * (1 + 1e-5), (key, float(excess.max()), lr)
        assert not torch.equal(p1, p0)
        # the clipped gradient, as the first moment saw it: |m| = (1 - beta1) |coef g + wd p| <= (1 - beta1) (c + wd |p|) per element
        b1, wd = o.param_groups[0]["betas"][0], o.param_groups[0]["weight_decay"]
        # (the computed norm, hence coef, is off by at most RED)
        bound = (1 - b1) * (c + wd * p0.double().abs()) * (1 + 2 * RED)
        assert bool((o._flat[0]["m"].double().abs() <= bound).all()), key


def test_bad_batch_is_skipped_and_training_goes_on(fed):
    model, sde = _model(skip_nonfinite_steps=True)
    _feed(model, sde, fed)
    model.target[0, 0, 3, 4] = math.nan      # the drift net's loss target is input - target ...
    model.std_noise[1, 0, 7, 1] = math.nan   # ... and the noise net's is std_noise
    before = _opt_state(model)
    model.optimize_parameters()
    for a, b in zip(before, _opt_state(model)):
        assert torch.equal(a, b)
    gi = model.grad_info
    assert gi["skipped_steps"] == 1 and gi["drift"]["skipped"] is True and gi["noise"]["skipped"] is True
    assert not math.isfinite(gi["drift"]["norm"]) and not math.isfinite(gi["noise"]["norm"])
    for o in (model.drift_optimizer, model.noise_optimizer):
        assert o._flat[0]["step"] == 0 and o.skipped_steps == 1
        assert o.state_dict()["flat"][0]["skipped"] == 1 and o.state_dict()["flat"][0]["step"] == 0
    assert "skipped=1" in model.get_grad_message()
    _feed(model, sde, fed)  # a clean batch
    loss, _ = model.optimize_parameters()
    assert math.isfinite(loss)
    after = _opt_state(model)
    for a, b in zip(before, after):
        assert bool(torch.isfinite(b).all())
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[3], after[3])
    assert model.grad_info["skipped_steps"] == 1 and model.grad_info["drift"]["skipped"] is False
    for o in (model.drift_optimizer, model.noise_optimizer):
        assert o._flat[0]["step"] == 1 and o.skipped_steps == 1


def test_bad_batch_without_the_option_poisons_the_nets(fed):
    model, sde = _model()
    _feed(model, sde, fed)
    model.target[0, 0, 3, 4] = math.nan
    model.std_noise[1, 0, 7, 1] = math.nan
    model.optimize_parameters()
    for o in (model.drift_optimizer, model.noise_optimizer):
        assert not bool(torch.isfinite(o._flat[0]["p"]).all())
        assert o._flat[0]["step"] == 1
