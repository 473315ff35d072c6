"""driftSDE few-step sampling (sample_T / sample_timesteps) on the device: the table-driven state advance, the table path against the
plain T-step path, parity of a 10-jump chain with the oracle's CPU restatement, graph replay against eager steps, what the nets are fed,
the exact-prediction invariant through the real kernels, and the testUM option."""
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


def oracle_nets(model):
    """CPU oracle copies of the model's two nets (as in tests/test_sampling_gpu.py)"""
    mo = pipeline.load_options()['models']['DriftNoise']
    refs = []
    for key, net in (('dnet_settings', model.drift_net), ('nnet_settings', model.noise_net)):
        s = {k: v for k, v in dict(mo[key]).items() if k not in ("module_name", "class_name")}
        smm = nn.ModuleList([unet_ref.ScoreMapModule(visual_dim=mo['score_map_ngf'] * m) for m in mo['score_map_ch_mult']])
        r = unet_ref.LearnableForwardUNet_MultiScoreMap(CLIP_ScoreMapModule=smm, use_image_context=True, **s).eval()
        r.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        refs.append(r)
    return refs


def test_table_advance_kernel_against_a_host_model():
    T, B = 100, 5
    ts = [97, 60, 59, 31, 7, 0]
    next_t = torch.full((T + 1,), -1, dtype=torch.int32)
    for t, s in zip(ts[:-1], ts[1:]):
        next_t[t] = s
    nd = next_t.to(DEV)
    for t_stop in (0, 31):
        state = torch.tensor([ts[0], 0, 0], dtype=torch.int32, device=DEV)
        tdev = torch.full((B,), float(ts[0]), device=DEV)
        t, n = ts[0], 0
        for _ in range(len(ts) - 1 + 2):  # K + 2 calls: the wrap back to t_0 included
            ops.step_state_advance_table(state, tdev, nd, ts[0], t_stop)
            t = int(next_t[t])
            if t <= t_stop:
                t = ts[0]
            n += 1
            assert state.cpu().tolist() == [t, n, n]
            assert tdev.cpu().tolist() == [float(t)] * B
    # a state outside [0, T+1) restarts at t_0 instead of reading past next_t
    for bad in (-7, T + 1, 10 ** 6):
        state = torch.tensor([bad, 4, 4], dtype=torch.int32, device=DEV)
        tdev = torch.zeros(B, device=DEV)
        ops.step_state_advance_table(state, tdev, nd, ts[0], 0)
        assert state.cpu().tolist() == [ts[0], 5, 5] and tdev.cpu().tolist() == [float(ts[0])] * B


def test_forward_diffusion_unchanged_by_the_option():
    plain = create_sde({}, dict(class_name="driftSDE", T=100, max_sigma=0.4))
    few = create_sde({}, dict(class_name="driftSDE", T=100, max_sigma=0.4, sample_T=10))
    b = make_batch(3, 32, seed=4)
    t = torch.tensor([1, 57, 100]).reshape(3, 1, 1, 1)
    outs = []
    for sde in (plain, few):
        sde.set_gpu(torch.device(DEV))
        sde.set_seed(8)
        outs.append([o.cpu() for o in sde.forward_diffusion(b['target'].to(DEV), b['input'].to(DEV), t=t)])
    for p, q in zip(*outs):
        assert torch.equal(p, q)


def _chain(model, batch, seed):
    sde = model.sde
    sde.set_seed(seed)
    model.feed_data(batch)
    sde.set_seed(seed)
    model.test()
    return torch.from_numpy(model.get_visuals()).clone()


def test_full_length_schedule_is_bit_identical_to_the_plain_chain():
    """sample_T = T runs the table path (jump tables, table advance) and must give the plain T-step chain's bits, on-device Philox
    noise and graph replay in both."""
    T, B, H = 20, 4, 64
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0)
    model.set_eval()
    batch = make_batch(B, H, seed=21)
    sde.hip_graph = True
    outs = []
    for kw in ({}, dict(sample_T=T)):
        sde.set_sample_steps(**kw)
        outs.append(_chain(model, batch, 31))
        assert sde.last_mode == "graph" and sde.last_steps == T
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def _jump_coeffs_fp64(T, K, eta, max_sigma=0.4):
    """the jump coefficients restated from DESIGN.md §3 for the uniform schedule: a = d_t - d_s, eta_t = eta s_s sqrt(1 - s_s^2/s_t^2),
    b = s_t - sqrt(s_s^2 - eta_t^2), c = eta_t; fp64, rounded once to fp32"""
    d = sde_ref.drift_level_table(T, "sigmoid").double()
    sg = max_sigma * torch.sqrt(sde_ref.drift_level_table(T, "sigmoid").double())
    ts = [((K - k) * T) // K for k in range(K + 1)]
    out = []
    for t, s in zip(ts[:-1], ts[1:]):
        et = eta * float(sg[s]) * math.sqrt(max(1.0 - float(sg[s] / sg[t]) ** 2, 0.0))
        b = float(sg[t]) - math.sqrt(max(float(sg[s]) ** 2 - et ** 2, 0.0))
        out.append((t, torch.tensor(float(d[t] - d[s])).float(), torch.tensor(b).float(), torch.tensor(et).float()))
    return out


def test_ten_jump_chain_parity_with_the_oracle():
    """T = 100, K = 10 at 64x64 batch 4 with injected noise against a CPU restatement (oracle nets, oracle update, this test's own
    jump coefficients); the c1 chain's bar, eta = 1 and eta = 0."""
    T, K, B, H = 100, 10, 4, 64
    model, _ = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0)
    model.set_eval()
    refs = oracle_nets(model)
    batch = make_batch(B, H, seed=1234)
    g = torch.Generator().manual_seed(4321)
    x_T = batch['input'] + 0.4 * torch.randn(batch['input'].shape, generator=g)
    noises = torch.randn((K,) + tuple(batch['input'].shape), generator=g)
    enc = unet_ref.StubTextEncoder()
    for eta in (1.0, 0.0):
        sde = create_sde(model.get_nets(), dict(class_name="driftSDE", T=T, max_sigma=0.4, eta=eta, sample_T=K))
        sde.set_gpu(model.device)
        model.set_sde(sde)
        model.feed_data(batch)
        model.test(x_T=x_T.to(DEV), noises=noises.to(DEV))
        assert sde.last_steps == K
        out = torch.from_numpy(model.get_visuals())
        assert out.shape == (B, 1, H, H) and torch.isfinite(out).all()
        x = x_T.clone()
        with torch.no_grad():
            for i, (t, a, b, c) in enumerate(_jump_coeffs_fp64(T, K, eta)):
                assert (float(c) == 0.0) == (eta == 0.0 or i == K - 1)
                tt = torch.full((B,), t, dtype=torch.long)
                rd = refs[0](x - batch['input'], batch['input'], tt, batch['names'], enc, image_context=batch['A_emb'])
                rn = refs[1](x - batch['input'], x, tt, batch['names'], enc, image_context=batch['A_emb'])
                rd = rd[0] if isinstance(rd, tuple) else rd
                rn = rn[0] if isinstance(rn, tuple) else rn
                x = sde_ref.drift_reverse_update(x, rd, rn, noises[i], a, b, c)
        err = float((out - x).abs().max())
        worst = max(abs(sde_ref.psnr(out[k], batch['target'][k]) - sde_ref.psnr(x[k], batch['target'][k])) for k in range(B))
        print(f"K={K} eta={eta}: max|hip-oracle| {err:.3e}, worst per-image |dPSNR| {worst:.2e} dB")
        assert abs(sde_ref.psnr(out, batch['target']) - sde_ref.psnr(x, batch['target'])) < 1e-3
        assert worst < 1e-3 and err < 5e-4


def test_graph_replay_equals_eager_steps_on_a_schedule():
    T, K, B, H = 100, 25, 2, 32
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=3, sde_overrides=dict(sample_T=K))
    model.set_eval()
    batch = make_batch(B, H, seed=11)
    outs = []
    for use_graph in (True, False):
        sde.hip_graph = use_graph
        outs.append(_chain(model, batch, 99))
        assert sde.last_mode == ("graph" if use_graph else "eager") and sde.last_steps == K
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


class Recorder:
    def __init__(self):
        self.ts = []

    def __call__(self, a, b, t, names, text_encoder, image_context=None):
        self.ts.append(t.detach().cpu().tolist())
        return torch.zeros_like(a)


def test_nets_see_each_schedule_point_once():
    T, K, B = 100, 7, 3
    nets = {"drift_net": Recorder(), "noise_net": Recorder()}
    sde = driftSDE(nets=nets, T=T, sample_T=K)
    sde.set_gpu(torch.device(DEV))
    sde.hip_graph = False
    cond = torch.rand(B, 1, 16, 16, device=DEV)
    out = sde.reverse_ddpm(cond, ["x"] * B, None)
    torch.cuda.synchronize()
    assert sde.last_steps == K and sde.last_mode == "eager" and torch.isfinite(out).all()
    want = [[float(t)] * B for t in sde.timesteps[:-1]]
    assert nets["drift_net"].ts == want and nets["noise_net"].ts == want
    # T_stop: a schedule point ends the chain there; anything else is refused
    nets["drift_net"].ts.clear()
    sde.reverse_ddpm(cond, ["x"] * B, None, T_stop=sde.timesteps[3])
    torch.cuda.synchronize()
    assert sde.last_steps == 3 and len(nets["drift_net"].ts) == 3
    with pytest.raises(ValueError):
        sde.reverse_ddpm(cond, ["x"] * B, None, T_stop=sde.timesteps[3] + 1)


def test_exact_predictions_land_on_x0_through_the_kernels():
    """Stand-in nets that return the true R = cond - x0 and eps_hat = (x_t - x0 - d_t R) / s_t, computed on the device from the
    timestep vector they are fed: a deterministic (eta = 0) non-uniform chain through the jump tables, the table advance and the fused
    update must land on x0 (see tests/test_sample_steps_cpu.py), here to fp32 rounding, graph replay on."""
    T, B, H = 100, 2, 32
    g = torch.Generator().manual_seed(5)
    x0 = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).to(DEV)
    cond = (x0.cpu() + 0.3 * torch.randn(x0.shape, generator=g)).to(DEV)
    R = cond - x0
    sde = driftSDE(T=T, eta=0.0, sample_timesteps=[97, 80, 41, 40, 12, 3])
    sde.set_gpu(torch.device(DEV))
    d = sde.drift_schedule
    sg = sde.max_sigma * torch.sqrt(sde.noise_schedule)

    def drift_net(a, b, t, *args, **kw):
        return R.clone()

    def noise_net(a, x, t, *args, **kw):
        ti = t.long()
        return (x - x0 - torch.index_select(d, 0, ti).view(-1, 1, 1, 1) * R) / torch.index_select(sg, 0, ti).view(-1, 1, 1, 1)

    sde.drift_net, sde.noise_net = drift_net, noise_net
    x_T = x0 + d[97] * R + sg[97] * torch.randn(x0.shape, generator=g).to(DEV)
    out = sde.reverse_ddpm(cond, ["x"] * B, None, x_T=x_T)
    torch.cuda.synchronize()
    assert sde.last_steps == 6 and sde.last_mode == "graph"
    err = float((out - x0).abs().max())
    print(f"exact-prediction chain: max|x - x0| {err:.3e}")
    assert err < 2e-5


def test_testum_sample_T_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_few").replace("image_size: 64", "image_size: 32").replace("T: 100", "T: 4")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    res = testUM.main(["-opt", str(cfg), "--random-init", "--sample-T", "3", "--limit", "1"])
    assert sum(v['num'] for v in res.values()) == 1
    out = capsys.readouterr().out
    assert "(3 steps)" in out, out[-500:]
