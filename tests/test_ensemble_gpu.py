"""Posterior ensembles (driftSDE num_samples) on the device: the member noise streams against the Philox oracle, the fused x_T
construction and the member step against the launches they replace (bits), the mean / std reduction against fp64 with bounds derived
from its stated operation order, batch independence of whole chains on the pipeline nets, independence of the noise across members and
steps on zero nets, and the model / testUM surface."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import driftSDE  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402
from oracle import philox_ref  # noqa: E402

DEV = "cuda"
TP1 = 8
U = 2.0 ** -24  # unit roundoff of fp32


def member_randn_ref(n_s, seed, member, j=0):
    """include/idiff.h on the oracle: counters (lo32(q), hi32(q), lo32(m), hi32(m)), q = j*Q + v, Q = n_s/4; philox_ref.randn's mapping"""
    Q = n_s // 4
    q = np.uint64(j * Q) + np.arange(Q, dtype=np.uint64)
    c = np.zeros((Q, 4), dtype=np.uint32)
    c[:, 0] = (q & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c[:, 1] = (q >> np.uint64(32)).astype(np.uint32)
    c[:, 2] = np.uint32(member & 0xFFFFFFFF)
    c[:, 3] = np.uint32((member >> 32) & 0xFFFFFFFF)
    w = philox_ref.philox4x32_10(c, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))
    r0 = np.sqrt(np.float32(-2.0) * np.log(philox_ref.u01(w[:, 0])))
    r1 = np.sqrt(np.float32(-2.0) * np.log(philox_ref.u01(w[:, 2])))
    a0 = np.float32(6.283185307179586) * philox_ref.u01(w[:, 1])
    a1 = np.float32(6.283185307179586) * philox_ref.u01(w[:, 3])
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1).astype(np.float32).reshape(-1)


def ids(*members):
    return ops.member_ids(members, DEV)


def table(rows, t):
    tb = torch.full((len(rows), TP1), float("nan"), dtype=torch.float32)
    tb[:, t] = torch.tensor(rows, dtype=torch.float32)
    return tb.to(DEV)


# ---- 1. the streams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 3])
def test_randn_members_against_the_oracle(j):
    n_s, seed = 32 * 32, 0x1234567887654321
    members = [1, 2, 2 ** 32 + 1]
    z = ops.randn_members(ids(*members), (1, 32, 32), seed, j)
    assert z.shape == (3, 1, 32, 32)
    z = z.cpu().numpy().reshape(3, -1)
    for row, m in enumerate(members):
        err = np.abs(z[row] - member_randn_ref(n_s, seed, m, j)).max()
        print(f"member {m}, j = {j}: max |z - z_ref| = {err:.2e}")
        assert err < 1e-4  # the bar of tests/test_ops_gpu.py for idiff_randn
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.06


def test_a_members_draw_does_not_depend_on_its_row_or_neighbours():
    seed, shp = 77, (1, 64, 64)
    alone = {m: ops.randn_members(ids(m), shp, seed, 2)[0] for m in (1, 2, 2 ** 32 + 1, 9)}
    mixed = ops.randn_members(ids(9, 2 ** 32 + 1, 1, 5, 2), shp, seed, 2)
    for row, m in ((0, 9), (1, 2 ** 32 + 1), (2, 1), (4, 2)):
        assert torch.equal(mixed[row], alone[m]), m
    assert not torch.equal(alone[1], alone[2]) and not torch.equal(alone[1], alone[2 ** 32 + 1])
    assert not torch.equal(alone[1], ops.randn_members(ids(1), shp, seed, 3)[0])       # another draw index
    assert not torch.equal(alone[1], ops.randn(shp, DEV, seed, 2 * 64 * 64 // 4))     # member 0's counters at the same q


def test_member_entry_points_refuse_bad_arguments():
    with pytest.raises(ValueError):
        ops.member_ids([1, 0], DEV)
    with pytest.raises(Exception):  # a sample that is not a whole number of 4-element groups
        ops.randn_members(ids(1), (1, 5, 5), 0, 0)
    with pytest.raises(Exception):
        ops.ensemble_init(torch.zeros(1, 1, 5, 5, device=DEV), 2, ids(1, 2), 0.4, 0)
    with pytest.raises(Exception):  # one id per row
        ops.ensemble_init(torch.zeros(1, 1, 8, 8, device=DEV), 2, ids(1), 0.4, 0)
    with pytest.raises(Exception):
        ops.ensemble_stats(torch.zeros(1, 2, 1, 5, 5, device=DEV))


def test_ensemble_init_bits():
    B, S, seed, sigma = 2, 3, 5, 0.4
    g = torch.Generator().manual_seed(3)
    cond = (torch.rand(B, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    m = ids(4, 5, 6, 2 ** 32 + 1, 8, 9)
    cond_rep, x, xa = ops.ensemble_init(cond, S, m, sigma, seed)
    want_rep = cond.repeat_interleave(S, dim=0).contiguous()
    z = ops.randn_members(m, (1, 32, 32), seed, 0)
    want_x = ops.axpby(want_rep, z, 1.0, sigma)
    want_xa = ops.axpby(want_x, want_rep, 1.0, -1.0)
    assert torch.equal(cond_rep, want_rep) and torch.equal(x, want_x) and torch.equal(xa, want_xa)
    assert float((x - want_rep).std()) > 0.3


# ---- 2. the member step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("rhos", [(0.37, 0.81), (0.0, 0.81), (0.0, 0.0)])
def test_member_step_with_injected_noise_equals_the_plain_steps(rows, rhos):
    R, shp = 3, (3, 1, 32, 32)
    n = R * 32 * 32
    g = torch.Generator().manual_seed(rows + int(100 * rhos[0]))
    x, r, e, rp, ep, cond = (torch.randn(shp, generator=g).to(DEV) for _ in range(6))
    zb = torch.randn((3,) + shp, generator=g).to(DEV)
    t, a, b, c = 5, 0.0713, 0.1291, 0.0577
    state = torch.tensor([t, 4, 2], dtype=torch.int32, device=DEV)
    m = ids(3, 1, 2)
    if rows == 3:
        coef = table([a, b, c], t)
        x0, xa0 = x.clone(), torch.empty_like(x)
        ops.drift_reverse_step_dev(x0, r, e, zb, cond, xa0, coef, state, 9, n // 4, 11)
        x1, xa1 = x.clone(), torch.empty_like(x)
        ops.drift_reverse_step_members_dev(x1, r, e, None, None, zb, cond, xa1, coef, state, m, 9)
        assert torch.equal(x0, x1) and torch.equal(xa0, xa1)
        return
    coef = table([a, b, c, rhos[0], rhos[1]], t)
    nan = torch.full(shp, float("nan"), device=DEV)  # a clock whose rho is 0 does not read its history
    hist = [(rp if rhos[0] else nan), (ep if rhos[1] else nan)]
    x0, xa0, rp0, ep0 = x.clone(), torch.empty_like(x), hist[0].clone(), hist[1].clone()
    ops.drift_reverse_step2_dev(x0, r, e, rp0, ep0, zb, cond, xa0, coef, state, 9, n // 4, 11)
    x1, xa1, rp1, ep1 = x.clone(), torch.empty_like(x), hist[0].clone(), hist[1].clone()
    ops.drift_reverse_step_members_dev(x1, r, e, rp1, ep1, zb, cond, xa1, coef, state, m, 9)
    assert torch.isfinite(x1).all()
    assert torch.equal(x0, x1) and torch.equal(xa0, xa1)
    assert torch.equal(rp1, r) and torch.equal(ep1, e) and torch.equal(rp0, rp1) and torch.equal(ep0, ep1)
    assert state.cpu().tolist() == [t, 4, 2]


@pytest.mark.parametrize("rows", [3, 5])
def test_member_step_on_device_noise_equals_injected_member_noise(rows):
    shp, seed = (3, 1, 32, 32), 21
    g = torch.Generator().manual_seed(rows)
    x, r, e, rp, ep, cond = (torch.randn(shp, generator=g).to(DEV) for _ in range(6))
    t, draws = 5, 4
    coef = table([0.0713, 0.1291, 0.0577, 0.37, 0.81][:rows], t)
    m = ids(7, 2 ** 32 + 1, 2)
    z = ops.randn_members(m, shp[1:], seed, 1 + draws)  # the draw of a step is j = 1 + state[1]
    hist = lambda: (rp.clone(), ep.clone()) if rows == 5 else (None, None)  # noqa: E731
    xa0, xa1 = torch.empty_like(x), torch.empty_like(x)
    x0, h0 = x.clone(), hist()
    ops.drift_reverse_step_members_dev(x0, r, e, h0[0], h0[1], None, cond, xa0, coef, torch.tensor([t, draws, 0], dtype=torch.int32, device=DEV), m, seed)
    x1, h1 = x.clone(), hist()
    ops.drift_reverse_step_members_dev(x1, r, e, h1[0], h1[1], z[None].contiguous(), cond, xa1, coef,
                                       torch.tensor([t, draws, 0], dtype=torch.int32, device=DEV), m, seed)
    assert torch.equal(x0, x1) and torch.equal(xa0, xa1)
    assert not torch.equal(x0, x)
    # the same members in other rows get the same noise: the update of a row moves with its member
    perm = [2, 0, 1]
    x2, h2 = x[perm].contiguous(), tuple(None if h is None else h[perm].contiguous() for h in hist())
    ops.drift_reverse_step_members_dev(x2, r[perm].contiguous(), e[perm].contiguous(), h2[0], h2[1], None, cond[perm].contiguous(),
                                       torch.empty_like(x), coef, torch.tensor([t, draws, 0], dtype=torch.int32, device=DEV),
                                       m[perm].contiguous(), seed)
    assert torch.equal(x2, x0[perm])


def test_member_step_argument_checks():
    shp = (2, 1, 8, 8)
    x = torch.ones(shp, device=DEV)
    bufs = [torch.zeros(shp, device=DEV) for _ in range(6)]
    state = torch.tensor([5, 0, 0], dtype=torch.int32, device=DEV)
    c3, c5 = table([0.1, 0.1, 0.0], 5), table([0.1, 0.1, 0.0, 0.5, 0.5], 5)
    m = ids(1, 2)
    with pytest.raises(Exception):  # a 3-row table takes no history
        ops.drift_reverse_step_members_dev(x, bufs[0], bufs[1], bufs[2], bufs[3], None, bufs[4], bufs[5], c3, state, m, 0)
    with pytest.raises(Exception):  # a 5-row table needs it
        ops.drift_reverse_step_members_dev(x, bufs[0], bufs[1], None, None, None, bufs[4], bufs[5], c5, state, m, 0)
    with pytest.raises(Exception):  # one buffer for both histories
        ops.drift_reverse_step_members_dev(x, bufs[0], bufs[1], bufs[2], bufs[2], None, bufs[4], bufs[5], c5, state, m, 0)
    with pytest.raises(Exception):  # one id per row
        ops.drift_reverse_step_members_dev(x, bufs[0], bufs[1], None, None, None, bufs[4], bufs[5], c3, state, ids(1), 0)
    assert torch.equal(x, torch.ones(shp, device=DEV))


# ---- 3. the reduction -----------------------------------------------------------------------------------------------------------
def stats_input(B, S, H=32, seed=0):
    """N(0, 1)*0.5 + a per-pixel offset in [-1, 1]: the value range of the images"""
    g = torch.Generator().manual_seed(seed)
    off = torch.rand(B, 1, 1, H, H, generator=g) * 2 - 1
    return (0.5 * torch.randn(B, S, 1, H, H, generator=g) + off).contiguous()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 16, 17, 40])
def test_ensemble_stats_against_fp64(B, S):
    """Bounds from the stated operation order (include/idiff.h), u = 2^-24, X = max |x|, a factor 2 as the only margin.
    mean: a sequential fp32 sum of S terms is off by at most (S - 1) u sum|x_s| <= S u S X; the division by S scales that to S u X and
      adds one rounding (u X): assert |mean - ref| <= 2 S u X.
    sum of squared deviations ss = std^2 (S - 1): each deviation d_s = x_s - mean carries the mean's error plus the subtraction's
      rounding (|d_s| <= 2X): at most (S + 2) u X; its square is then off by at most 2 |d_s| (S + 2) u X + u d_s^2 <= 4 (S + 3) u X^2; S
      such terms contribute 4 S (S + 3) u X^2, and their sequential sum, S terms of at most 4 X^2, (S - 1) u S 4 X^2: together at
      most 8 S (S + 1) u X^2 for every S >= 1.  Assert |ss - ref| <= 2 * 8 S (S + 1) u X^2.  std is checked through ss only: a square root near
      zero amplifies any bound, so no tolerance of its own is invented for it."""
    x = stats_input(B, S, seed=S)
    X = float(x.abs().max())
    mean, std = ops.ensemble_stats(x.to(DEV))
    assert mean.shape == (B, 1, 32, 32) and std.shape == mean.shape
    xd = x.double().numpy()
    ref_mean = xd.mean(axis=1)
    ref_ss = ((xd - ref_mean[:, None]) ** 2).sum(axis=1)
    got_mean, got_std = mean.cpu().double().numpy(), std.cpu().double().numpy()
    b_mean, b_ss = 2 * S * U * X, 2 * 8 * S * (S + 1) * U * X * X
    e_mean, e_ss = np.abs(got_mean - ref_mean).max(), np.abs(got_std ** 2 * (S - 1) - ref_ss).max()
    print(f"B={B} S={S} X={X:.3f}: |mean - ref| {e_mean:.3e} (bound {b_mean:.3e}, ratio {e_mean / b_mean:.3f}); "
          f"|ss - ref| {e_ss:.3e} (bound {b_ss:.3e}, ratio {e_ss / b_ss:.3f})")
    assert e_mean <= b_mean and e_ss <= b_ss
    assert (got_std >= 0).all()
    if S == 1:
        assert torch.equal(mean.cpu(), x[:, 0]) and not std.any()


@pytest.mark.parametrize("S", [2, 16, 17])
def test_ensemble_stats_do_not_depend_on_the_batch_or_the_run(S):
    x = stats_input(3, S, seed=100 + S).to(DEV)
    mean3, std3 = ops.ensemble_stats(x)
    again = ops.ensemble_stats(x)
    assert torch.equal(mean3, again[0]) and torch.equal(std3, again[1])
    for b in range(3):
        mean1, std1 = ops.ensemble_stats(x[b:b + 1].contiguous())
        assert torch.equal(mean1[0], mean3[b]) and torch.equal(std1[0], std3[b])


@pytest.mark.parametrize("S", [1, 5, 16])
def test_ensemble_stats_register_and_second_read_forms_agree(S, monkeypatch):
    x = stats_input(2, S, H=64, seed=200 + S).to(DEV)
    monkeypatch.delenv("IDIFF_ENSEMBLE_REREAD", raising=False)
    mean_reg, std_reg = ops.ensemble_stats(x)
    monkeypatch.setenv("IDIFF_ENSEMBLE_REREAD", "1")
    mean_rr, std_rr = ops.ensemble_stats(x)
    assert torch.equal(mean_reg, mean_rr) and torch.equal(std_reg, std_rr)
    assert torch.isfinite(std_rr).all() and (S == 1 or float(std_rr.min()) > 0)


# ---- 4. whole chains ------------------------------------------------------------------------------------------------------------
T, H = 20, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=4))
    model.set_eval()
    return model, sde


@pytest.mark.parametrize("order", [1, 2])
def test_a_members_image_does_not_depend_on_its_batch(built, order):
    """B = 2, S = 3 on the random-init pipeline nets, on-device noise, graph replay: one chain of six rows, chunks of two, and six
    single-row calls with the member named explicitly give the same bits per member."""
    model, sde = built
    B, S = 2, 3
    batch = make_batch(B, H, seed=5)
    cond, ctx = batch['input'].to(DEV).contiguous(), batch['A_emb'].to(DEV).contiguous()
    sde.set_solver_order(order)
    try:
        runs = {}
        for mb in (16, 2, 6):
            sde.set_seed(41)
            sde.set_num_samples(S, max_batch=mb)
            mean, std, samples = sde.reverse_ddpm_ensemble(cond, batch['names'], model.text_encoder, image_context=ctx, return_samples=True)
            assert sde.last_mode == "graph" and sde.last_steps == 4 and sde.last_solver_order == order
            assert sde.last_members.tolist() == [[1, 2, 3], [4, 5, 6]]
            assert samples.shape == (B, S, 1, H, H) and mean.shape == (B, 1, H, H) and torch.isfinite(samples).all()
            runs[mb] = (mean.clone(), std.clone(), samples.clone())
        for mb in (2, 6):
            for k in range(3):
                assert torch.equal(runs[16][k], runs[mb][k]), (mb, k)
        samples = runs[16][2]
        assert not torch.equal(samples[0, 0], samples[0, 1]) and float(runs[16][1].mean()) > 0
        sde.set_num_samples(None)
        for b in range(B):
            for s in range(S):
                m, st, one = sde.reverse_ddpm_ensemble(cond[b:b + 1].contiguous(), batch['names'][b:b + 1], model.text_encoder,
                                                       image_context=ctx[b:b + 1].contiguous(), num_samples=1, members=[1 + b * S + s],
                                                       return_samples=True)
                assert torch.equal(one[0, 0], samples[b, s]), (b, s)
                assert torch.equal(m[0], samples[b, s]) and not st.any()
    finally:
        sde.set_solver_order(1)
        sde.set_num_samples(None, max_batch=16)


def zeros_net(a, b, t, names, text_encoder, image_context=None):
    return torch.zeros_like(a)


def test_noise_is_independent_across_members_and_steps():
    """Zero nets, eta = 1, K = 10, 64x64, S = 16: a member's output is cond + sigma z_0 + sum_k c_k z_k exactly.
    (i) each member equals that sum formed in fp32 in the kernel's order from ops.randn_members draws, bit for bit (zero predictions
        make (x - a*0) - b*0 exact, so only + c*z rounds);
    (ii) the pooled ensemble variance mean(std^2) equals sigma^2 + sum c_k^2 within five standard errors of a variance estimate from
        H*W*(S - 1) degrees of freedom, sqrt(2 / (H W (S - 1))) relative = 2.9 %: a shared or repeated stream misses by a factor."""
    K, Hn, S, seed = 10, 64, 16, 3
    sde = driftSDE(nets=dict(drift_net=zeros_net, noise_net=zeros_net), T=100, eta=1.0, sample_T=K, num_samples=S)
    sde.set_gpu(torch.device(DEV))
    sde.set_seed(seed)
    g = torch.Generator().manual_seed(1)
    cond = (torch.rand(1, 1, Hn, Hn, generator=g) * 2 - 1).to(DEV)
    mean, std, samples = sde.reverse_ddpm_ensemble(cond, ["x"], None, return_samples=True)
    torch.cuda.synchronize()
    assert sde.last_steps == K and sde.last_mode == "graph" and sde.last_members.tolist() == [list(range(1, S + 1))]
    coef = sde._schedule_tables(sde.timesteps)[0]
    cs = [coef[2, t] for t in sde.timesteps[:-1]]  # fp32 0-dim tensors, the table the kernel reads
    m = ops.member_ids(range(1, S + 1), DEV)
    sigma = torch.tensor(sde.max_sigma, dtype=torch.float32)
    want = cond.cpu() + sigma * ops.randn_members(m, (1, Hn, Hn), seed, 0).cpu()
    for k, c in enumerate(cs):
        if float(c) != 0.0:
            want = want + c * ops.randn_members(m, (1, Hn, Hn), seed, 1 + k).cpu()
    assert float(cs[-1]) == 0.0 and all(float(c) > 0 for c in cs[:-1])
    assert torch.equal(samples[0].cpu(), want)
    var_want = sde.max_sigma ** 2 + sum(float(c) ** 2 for c in cs)
    var_got = float((std.double() ** 2).mean())
    bound = 5 * math.sqrt(2.0 / (Hn * Hn * (S - 1)))
    print(f"pooled variance {var_got:.6f}, sigma^2 + sum c_k^2 = {var_want:.6f}, relative difference {abs(var_got / var_want - 1):.4f} (< {bound:.4f})")
    assert abs(var_got / var_want - 1) < bound
    assert float((mean - cond).abs().max()) < 6 * math.sqrt(var_want / S)


# ---- 5. the model and the driver ------------------------------------------------------------------------------------------------
def test_model_test_runs_the_ensemble_and_the_single_path_is_untouched(built):
    model, sde = built
    batch = make_batch(2, H, seed=9)
    nper = 2 * H * H // 4

    def single():
        sde.set_seed(17)
        model.feed_data(batch)
        model.test()
        return model.output.clone(), sde._off, sde._calls

    base = single()
    assert model.output_std is None and model.samples is None
    assert base[1:] == ((2 + 4) * nper, 2 + 4)  # the draws of feed_data, x_T and the four steps, as before
    try:
        sde.set_num_samples(4)
        sde.set_seed(17)
        model.feed_data(batch)
        off = (sde._off, sde._calls)
        model.test(return_samples=True)
        assert (sde._off, sde._calls) == off  # member streams consume none of the sde's own
        assert model.samples.shape == (2, 4, 1, H, H) and sde.last_members.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]]
        mean, std = ops.ensemble_stats(model.samples)
        assert torch.equal(model.output, mean) and torch.equal(model.output_std, std)
        ref = model.samples.double().mean(dim=1)
        assert float((model.output.double() - ref).abs().max()) < 2e-6
        assert float((model.output_std.double() ** 2 - model.samples.double().var(dim=1)).abs().max()) < 1e-5
        assert np.array_equal(model.get_visuals(), model.output.cpu().numpy())
        model.test()
        assert model.samples is None and model.output_std is not None
    finally:
        sde.set_num_samples(None)
    after = single()
    assert torch.equal(base[0], after[0]) and base[1:] == after[1:]


def test_pipeline_build_passes_num_samples_through():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=8, seed=0, sde_overrides=dict(num_samples=2, max_batch=3, sample_T=3))
    assert sde.num_samples == 2 and sde.max_batch == 3
    model.set_eval()
    model.feed_data(make_batch(2, H, seed=2))
    model.test()
    assert model.output.shape == (2, 1, H, H) and model.output_std.shape == (2, 1, H, H) and torch.isfinite(model.output).all()


def test_testum_num_samples_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_ens").replace("image_size: 64", "image_size: 32").replace("T: 100", "T: 8")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    res = testUM.main(["-opt", str(cfg), "--random-init", "--limit", "2", "--num-samples", "3", "--sample-T", "4"])
    out = capsys.readouterr().out
    assert "(4 steps)" in out and "3 samples per image" in out, out[-500:]
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2
    for name, v in done.items():
        assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD'}
        assert len(v['PSNR_member']) == v['num'] and len(v['STD']) == v['num']
        assert all(s > 0 for s in v['STD']) and all(math.isfinite(p) for p in v['PSNR_member'])
        folder = tmp_path / "results" / "drv_ens" / name
        files = sorted(os.listdir(folder))
        stds = [f for f in files if "_std_" in f]
        trips = [f for f in files if "_std_" not in f]
        assert len(stds) == v['num'] and len(trips) == v['num'], files
        for f in stds:
            assert f.endswith("_std_32x32x1.raw") and np.fromfile(folder / f, dtype=np.float32).size == 32 * 32
        psnr = []
        for f in trips:  # LQ | mean | GT side by side: the listed PSNR is image_metrics of the mean
            trip = torch.from_numpy(np.fromfile(folder / f, dtype=np.float32).reshape(32, 96))
            met = ops.image_metrics(trip[None, :, 32:64].contiguous().to(DEV), trip[None, :, 64:].contiguous().to(DEV)).cpu().tolist()[0]
            psnr.append(met[1])
        assert sorted(v['PSNR']) == sorted(psnr)
