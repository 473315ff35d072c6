"""driftSDE second-order multistep solver (solver_order: 2) on the device: the step kernel against a fp32 restatement of its stated
operation order (bits), chains through reverse_ddpm (one-jump chain against order 1, graph replay against eager steps, a 10-jump chain
against the oracle's CPU nets), what the nets are fed, the analytic-net accuracy ordering, and the testUM option."""
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from instancediff_amd import ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs import create_sde  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import driftSDE  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402
from oracle import sde_ref, unet_ref  # noqa: E402

DEV = "cuda"
TP1 = 8


def oracle_nets(model):
    """CPU oracle copies of the model's two nets (as in tests/test_sample_steps_gpu.py)"""
    mo = pipeline.load_options()['models']['DriftNoise']
    refs = []
    for key, net in (('dnet_settings', model.drift_net), ('nnet_settings', model.noise_net)):
        s = {k: v for k, v in dict(mo[key]).items() if k not in ("module_name", "class_name")}
        smm = nn.ModuleList([unet_ref.ScoreMapModule(visual_dim=mo['score_map_ngf'] * m) for m in mo['score_map_ch_mult']])
        r = unet_ref.LearnableForwardUNet_MultiScoreMap(CLIP_ScoreMapModule=smm, use_image_context=True, **s).eval()
        r.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        refs.append(r)
    return refs


def _chain(model, batch, seed):
    model.sde.set_seed(seed)
    model.feed_data(batch)
    model.sde.set_seed(seed)
    model.test()
    return torch.from_numpy(model.get_visuals()).clone()


class Recorder:
    def __init__(self):
        self.ts = []

    def __call__(self, a, b, t, names, text_encoder, image_context=None):
        self.ts.append(t.detach().cpu().tolist())
        return torch.zeros_like(a)


# ---- 5. the kernel ------------------------------------------------------------------------------------------------------------
def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def restated_step2(x, r, e, rp, ep, z, cond, a, b, c, rho_d, rho_s):
    """include/idiff.h's operation order in fp32 torch on the host: one rounding per operation, a zero rho skips its term"""
    rt = r if float(rho_d) == 0.0 else r + rho_d * (r - rp)
    et = e if float(rho_s) == 0.0 else e + rho_s * (e - ep)
    xn = ((x - a * rt) - b * et) + c * z
    return xn, xn - cond


def table(rows, t):
    """[len(rows), TP1] with `rows` in column t and NaN elsewhere"""
    tb = torch.full((len(rows), TP1), float("nan"), dtype=torch.float32)
    tb[:, t] = torch.stack([f32(v) for v in rows])
    return tb.to(DEV)


def same_bits(got, want):
    return torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n", [3 * 4096, 4096 + 3, 5])
@pytest.mark.parametrize("rhos", [(0.37, 0.81), (0.0, 0.81), (0.37, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("noise", ["injected", "philox", "none"])
def test_step2_kernel_bits(n, rhos, noise):
    g = torch.Generator().manual_seed(n + int(100 * rhos[0]) + int(1000 * rhos[1]))
    x, r, e, rp, ep, cond = (torch.randn(n, generator=g) for _ in range(6))
    t, a, b = 5, 0.0713, 0.1291
    c = 0.0 if noise == "none" else 0.0577
    step = 1 if (noise == "injected" and n % 4 == 0) else 0  # a later row of z_base where rows stay 16-byte aligned
    state = torch.tensor([t, 3, step], dtype=torch.int32, device=DEV)
    seed, nper, off_base = 1234, (n + 3) // 4, 77
    if noise == "injected":
        zb = torch.randn(step + 1, n, generator=g)
        z, z_base = zb[step], zb.to(DEV)
    elif noise == "philox":  # the order-1 kernel with a = b = 0, c = 1 on zeros writes z itself, at the same counters
        zero = torch.zeros(n, device=DEV)
        zx = torch.zeros(n, device=DEV)
        ops.drift_reverse_step_dev(zx, zero, zero, None, zero, torch.empty(n, device=DEV), table([0.0, 0.0, 1.0], t), state, seed, nper, off_base)
        z, z_base = zx.cpu(), None
        assert float(z.std()) > 0.5 or n < 16
    else:
        z, z_base = torch.zeros(n), None
    # a clock whose rho is 0 must not read its history: poison it
    rp_in = rp if rhos[0] != 0.0 else torch.full((n,), float("nan"))
    ep_in = ep if rhos[1] != 0.0 else torch.full((n,), float("nan"))
    want_x, want_xa = restated_step2(x, r, e, rp, ep, z, cond, f32(a), f32(b), f32(c), f32(rhos[0]), f32(rhos[1]))
    xd, xad, rpd, epd = x.to(DEV), torch.empty(n, device=DEV), rp_in.to(DEV), ep_in.to(DEV)
    ops.drift_reverse_step2_dev(xd, r.to(DEV), e.to(DEV), rpd, epd, z_base, cond.to(DEV), xad, table([a, b, c, rhos[0], rhos[1]], t), state, seed,
                                nper, off_base)
    torch.cuda.synchronize()
    assert torch.isfinite(xd).all()
    assert same_bits(xd, want_x) and same_bits(xad, want_xa)
    assert same_bits(rpd, r) and same_bits(epd, e)  # the history now holds this jump's predictions
    assert state.cpu().tolist() == [t, 3, step]     # the state is read only
    if rhos == (0.0, 0.0):
        x1, xa1 = x.to(DEV), torch.empty(n, device=DEV)
        ops.drift_reverse_step_dev(x1, r.to(DEV), e.to(DEV), z_base, cond.to(DEV), xa1, table([a, b, c], t), state, seed, nper, off_base)
        assert torch.equal(xd, x1) and torch.equal(xad, xa1)


def test_step2_off_schedule_row_poisons_the_result():
    """a NaN rho counts as non-zero: a state that points at a row which starts no jump cannot pass unnoticed"""
    n = 64
    x = torch.ones(n, device=DEV)
    state = torch.tensor([4, 0, 0], dtype=torch.int32, device=DEV)  # table() fills row 5 only
    ops.drift_reverse_step2_dev(x, x.clone(), x.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), None, x.clone(),
                                torch.empty(n, device=DEV), table([0.1, 0.1, 0.0, 0.5, 0.5], 5), state, 0, n // 4, 0)
    assert torch.isnan(x).all()


def test_step2_argument_checks():
    n = 64
    x = torch.ones(n, device=DEV)
    bufs = [torch.zeros(n, device=DEV) for _ in range(5)]
    state = torch.tensor([5, 0, 0], dtype=torch.int32, device=DEV)
    coef5 = table([0.1, 0.1, 0.0, 0.5, 0.5], 5)
    with pytest.raises(Exception):  # one buffer for both histories
        ops.drift_reverse_step2_dev(x, bufs[0], bufs[1], bufs[2], bufs[2], None, bufs[3], bufs[4], coef5, state, 0, n // 4, 0)
    with pytest.raises(Exception):  # the history aliases a prediction
        ops.drift_reverse_step2_dev(x, bufs[0], bufs[1], bufs[0], bufs[2], None, bufs[3], bufs[4], coef5, state, 0, n // 4, 0)
    with pytest.raises(Exception):  # a 3-row table
        ops.drift_reverse_step2_dev(x, bufs[0], bufs[1], bufs[2], x.clone(), None, bufs[3], bufs[4], coef5[:3].contiguous(), state, 0, n // 4, 0)
    with pytest.raises(Exception):  # host tensor
        ops.drift_reverse_step2_dev(x, bufs[0], bufs[1], bufs[2].cpu(), x.clone(), None, bufs[3], bufs[4], coef5, state, 0, n // 4, 0)
    assert torch.equal(x, torch.ones(n, device=DEV))


# ---- 6. chains on the real nets -----------------------------------------------------------------------------------------------
T, B, H = 100, 4, 64


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0)
    model.set_eval()
    return model, sde


def test_one_jump_chain_equals_order_one(built):
    model, sde = built
    batch = make_batch(B, H, seed=21)
    sde.set_sample_steps(sample_T=1)
    outs = []
    for order in (1, 2):
        sde.set_solver_order(order)
        outs.append(_chain(model, batch, 31))
        assert sde.last_solver_order == order and sde.last_steps == 1
    sde.set_solver_order(1)
    sde.set_sample_steps()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_graph_replay_equals_eager_steps_at_order_two(built):
    model, sde = built
    K = 25
    batch = make_batch(B, H, seed=11)
    sde.set_sample_steps(sample_T=K)
    sde.set_solver_order(2)
    outs = {}
    for use_graph in (True, False):
        sde.hip_graph = use_graph
        outs[use_graph] = _chain(model, batch, 99)
        assert sde.last_mode == ("graph" if use_graph else "eager") and sde.last_steps == K and sde.last_solver_order == 2
    sde.hip_graph = True
    sde.set_solver_order(1)
    first_order = _chain(model, batch, 99)
    sde.set_sample_steps()
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
    assert not torch.equal(outs[True], first_order)  # the two orders are different numerical choices


def _jump_coeffs2_fp64(T, K, eta, max_sigma=0.4):
    """[(t, a, b, c, rho_d, rho_s)] of the uniform schedule restated from DESIGN.md §3: a = d_t - d_s, eta_t = eta s_s sqrt(1 - s_s^2/s_t^2),
    b = s_t - sqrt(s_s^2 - eta_t^2), c = eta_t, rho = 1/2 (l_t - l_s) / (l_p - l_t) on l = d and l = s (0 at the first jump); fp64, rounded
    once to fp32"""
    d = [float(v) for v in sde_ref.drift_level_table(T, "sigmoid").double()]
    sg = [max_sigma * math.sqrt(float(v)) for v in sde_ref.drift_level_table(T, "sigmoid").double()]
    ts = [((K - k) * T) // K for k in range(K + 1)]
    out = []
    for k, (t, s) in enumerate(zip(ts[:-1], ts[1:])):
        et = eta * sg[s] * math.sqrt(max(1.0 - (sg[s] / sg[t]) ** 2, 0.0))
        b = sg[t] - math.sqrt(max(sg[s] ** 2 - et ** 2, 0.0))
        rho = [0.0, 0.0] if k == 0 else [0.5 * (lv[t] - lv[s]) / (lv[ts[k - 1]] - lv[t]) for lv in (d, sg)]
        out.append((t,) + tuple(torch.tensor(v, dtype=torch.float64).float() for v in (d[t] - d[s], b, et, rho[0], rho[1])))
    return out


def test_ten_jump_order_two_chain_parity_with_the_oracle(built):
    """T = 100, K = 10 at 64x64 batch 4 with injected noise against a CPU restatement: oracle nets, this test's own fp64 coefficients,
    the history kept here; the bars of tests/test_sample_steps_gpu.py::test_ten_jump_chain_parity_with_the_oracle; eta = 1 and eta = 0."""
    K = 10
    model, sde0 = built
    refs = oracle_nets(model)
    batch = make_batch(B, H, seed=1234)
    g = torch.Generator().manual_seed(4321)
    x_T = batch['input'] + 0.4 * torch.randn(batch['input'].shape, generator=g)
    noises = torch.randn((K,) + tuple(batch['input'].shape), generator=g)
    enc = unet_ref.StubTextEncoder()
    try:
        for eta in (1.0, 0.0):
            sde = create_sde(model.get_nets(), dict(class_name="driftSDE", T=T, max_sigma=0.4, eta=eta, sample_T=K, solver_order=2))
            sde.set_gpu(model.device)
            model.set_sde(sde)
            model.feed_data(batch)
            model.test(x_T=x_T.to(DEV), noises=noises.to(DEV))
            assert sde.last_steps == K and sde.last_solver_order == 2 and sde.last_mode == "graph"
            out = torch.from_numpy(model.get_visuals())
            assert out.shape == (B, 1, H, H) and torch.isfinite(out).all()
            x, rp, ep = x_T.clone(), None, None
            with torch.no_grad():
                for i, (t, a, b, c, rho_d, rho_s) in enumerate(_jump_coeffs2_fp64(T, K, eta)):
                    assert (float(c) == 0.0) == (eta == 0.0 or i == K - 1)
                    assert (float(rho_d) == 0.0) == (i == 0) and (float(rho_s) == 0.0) == (i == 0)
                    tt = torch.full((B,), t, dtype=torch.long)
                    rd = refs[0](x - batch['input'], batch['input'], tt, batch['names'], enc, image_context=batch['A_emb'])
                    rn = refs[1](x - batch['input'], x, tt, batch['names'], enc, image_context=batch['A_emb'])
                    rd = rd[0] if isinstance(rd, tuple) else rd
                    rn = rn[0] if isinstance(rn, tuple) else rn
                    rt = rd if i == 0 else rd + rho_d * (rd - rp)
                    et = rn if i == 0 else rn + rho_s * (rn - ep)
                    x = sde_ref.drift_reverse_update(x, rt, et, noises[i], a, b, c)
                    rp, ep = rd, rn
            err = float((out - x).abs().max())
            worst = max(abs(sde_ref.psnr(out[k], batch['target'][k]) - sde_ref.psnr(x[k], batch['target'][k])) for k in range(B))
            print(f"order 2, K={K} eta={eta}: max|hip-oracle| {err:.3e}, worst per-image |dPSNR| {worst:.2e} dB")
            assert abs(sde_ref.psnr(out, batch['target']) - sde_ref.psnr(x, batch['target'])) < 1e-3
            assert worst < 1e-3 and err < 5e-4
    finally:
        model.set_sde(sde0)


@pytest.mark.parametrize("kw,Tn", [(dict(sample_T=7), 100), (dict(sample_timesteps=[97, 80, 41, 40, 12, 3]), 100), (dict(), 12)])
def test_nets_see_each_schedule_point_once_at_order_two(kw, Tn):
    """one evaluation per net and schedule point: the history replaces a second evaluation.  With no schedule set, order 2 runs the
    schedule path over T, T-1, ..., 0."""
    Bn = 3
    nets = {"drift_net": Recorder(), "noise_net": Recorder()}
    sde = driftSDE(nets=nets, T=Tn, solver_order=2, **kw)
    sde.set_gpu(torch.device(DEV))
    sde.hip_graph = False
    cond = torch.rand(Bn, 1, 16, 16, device=DEV)
    out = sde.reverse_ddpm(cond, ["x"] * Bn, None)
    torch.cuda.synchronize()
    K = len(sde.timesteps) - 1
    assert sde.last_steps == K and sde.last_mode == "eager" and sde.last_solver_order == 2 and torch.isfinite(out).all()
    want = [[float(t)] * Bn for t in sde.timesteps[:-1]]
    assert nets["drift_net"].ts == want and nets["noise_net"].ts == want
    nets["drift_net"].ts.clear()
    sde.reverse_ddpm(cond, ["x"] * Bn, None, T_stop=sde.timesteps[3])
    torch.cuda.synchronize()
    assert sde.last_steps == 3 and len(nets["drift_net"].ts) == 3


# ---- 7. accuracy on analytic nets ---------------------------------------------------------------------------------------------
def gaussian_device_nets(sde, cond, m, v):
    """device stand-ins: the posterior means of tests/test_solver_order_cpu.py::gaussian_nets, from the timestep vector they are fed"""
    d = sde.drift_schedule
    sg = sde.max_sigma * torch.sqrt(sde.noise_schedule)

    def u_of(y, t):
        ti = t.long()
        g = -(1 - torch.index_select(d, 0, ti).view(-1, 1, 1, 1))
        s = torch.index_select(sg, 0, ti).view(-1, 1, 1, 1)
        return g, s, (y - g * m) / (g * g * v + s * s)

    def drift_net(xa, c, t, *args, **kw):
        g, s, u = u_of(xa, t)
        return m + v * g * u

    def noise_net(xa, x, t, *args, **kw):
        g, s, u = u_of(xa, t)
        return s * u
    return drift_net, noise_net


def test_order_two_ends_closer_to_the_full_chain_on_analytic_nets():
    """T = 100, K = 10, eta = 0, graph replay: distance of the K = 10 result to the K = T result, both orders.  The K = T chain is run
    at both orders as well (at T = 100 the order-1 one still carries a first-order error of its own); the ordering holds against either."""
    Tn, K, Bn, Hn = 100, 10, 2, 32
    g = torch.Generator().manual_seed(0)
    cond = (torch.rand(Bn, 1, Hn, Hn, generator=g) * 2 - 1).to(DEV)
    m = (0.3 * torch.randn(cond.shape, generator=g)).to(DEV)
    v = (0.05 + 0.2 * torch.rand(cond.shape, generator=g)).to(DEV)
    sde = driftSDE(T=Tn, eta=0.0, drift_schedule="linear", noise_schedule="linear")
    sde.set_gpu(torch.device(DEV))
    sde.drift_net, sde.noise_net = gaussian_device_nets(sde, cond, m, v)
    x_T = cond + sde.max_sigma * torch.randn(cond.shape, generator=g).to(DEV)
    res = {}
    for k in (K, Tn):
        for order in (1, 2):
            sde.set_sample_steps(sample_T=k)
            sde.set_solver_order(order)
            res[(k, order)] = sde.reverse_ddpm(cond, ["x"] * Bn, None, x_T=x_T).clone()
            torch.cuda.synchronize()
            assert sde.last_steps == k and sde.last_mode == "graph" and sde.last_solver_order == order
    for ref_order in (1, 2):
        ref = res[(Tn, ref_order)]
        d1 = float((res[(K, 1)] - ref).abs().max())
        d2 = float((res[(K, 2)] - ref).abs().max())
        print(f"analytic nets, K={K} against the order-{ref_order} K={Tn} chain: order 1 {d1:.4e}, order 2 {d2:.4e}")
        assert math.isfinite(d1) and d2 < d1


# ---- 8. the driver ------------------------------------------------------------------------------------------------------------
def test_testum_solver_order_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_o2").replace("image_size: 64", "image_size: 32").replace("T: 100", "T: 4")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    res = testUM.main(["-opt", str(cfg), "--random-init", "--sample-T", "3", "--solver-order", "2", "--limit", "1"])
    assert sum(v['num'] for v in res.values()) == 1
    out = capsys.readouterr().out
    assert "(3 steps)" in out and "solver order 2" in out, out[-500:]
