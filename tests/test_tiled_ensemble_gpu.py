"""Posterior ensembles of tiled chains (driftSDE tiled_ensemble) on the device.  The new step, idiff_drift_reverse_step_tiled_members_dev,
is held bit for bit to the two kernels it shares its pieces with: the tiled step given each member's draw as injected noise, and the member
step on a single window.  Whole chains: grouping, chunking, injected noise, the tiling and the solver order do not change a member; the
model / testUM surface on the pipeline nets."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import TilePlan, driftSDE  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

from test_tiling_gpu import make_plan, poison_unweighted, rand, table  # noqa: E402

DEV = "cuda"
MEMBERS = [7, 1, 2 ** 40 + 3]
R = len(MEMBERS)
GEOMS = [(40, 40, 16, 8), (24, 40, 16, 4), (48, 64, (16, 32), 0)]
T_ROW, A, B_, C_ = 5, 0.0713, 0.1291, 0.0577
NAN = float("nan")


def operands(plan, C, seed, rows=R, poison=True):
    """x, cond, the history pair [rows, C, H, W] and window predictions [rows*ny*nx, C, Ph, Pw] whose zero-weight pixels hold NaN"""
    g = torch.Generator().manual_seed(seed)
    ny, nx, Ph, Pw = plan.grid
    full, tiles = (rows, C, plan.H, plan.W), (rows * ny * nx, C, Ph, Pw)
    x, cond, rp, ep = (rand(full, g) for _ in range(4))
    r_t, e_t = rand(tiles, g), rand(tiles, g)
    if poison:
        poison_unweighted(r_t, plan), poison_unweighted(e_t, plan)
    return x, cond, rp, ep, r_t, e_t


def coef_of(rhos, c=C_):
    return table([A, B_, c] if rhos is None else [A, B_, c, rhos[0], rhos[1]], T_ROW)


def history(rhos, rp, ep):
    """fresh copies of the history buffers of a step; NaN where the clock's rho is 0: that history is not read"""
    if rhos is None:
        return None, None
    nan = torch.full_like(rp, NAN)
    return (rp if rhos[0] else nan).clone(), (ep if rhos[1] else nan).clone()


def run_members(plan, ops_in, rhos, state, zb, mdev, seed, c=C_):
    x, cond, rp, ep, r_t, e_t = ops_in
    x1, (h0, h1) = x.clone(), history(rhos, rp, ep)
    x_t, xa_t = torch.full_like(r_t, NAN), torch.full_like(r_t, NAN)
    ops.drift_reverse_step_tiled_members_dev(x1, r_t, e_t, h0, h1, zb, cond, x_t, xa_t, plan, coef_of(rhos, c), state, mdev, seed)
    return x1, x_t, xa_t, h0, h1


def run_tiled(plan, ops_in, rhos, state, zb, seed, c=C_):
    x, cond, rp, ep, r_t, e_t = ops_in
    x0, (h0, h1) = x.clone(), history(rhos, rp, ep)
    x_t, xa_t = torch.full_like(r_t, NAN), torch.full_like(r_t, NAN)
    ops.drift_reverse_step_tiled_dev(x0, r_t, e_t, h0, h1, zb, cond, x_t, xa_t, plan, coef_of(rhos, c), state, seed, x.numel() // 4, 0)
    return x0, x_t, xa_t, h0, h1


def same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), k
        if a is not None:
            assert torch.equal(a, b), k


# ---- 1. against the tiled step with injected noise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [0, 5])
@pytest.mark.parametrize("rhos", [None, (0.37, 0.81), (0.0, 0.81), (0.0, 0.0)])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("H,W,P,O", GEOMS)
def test_device_noise_equals_the_tiled_step_given_the_members_draw(H, W, P, O, C, rhos, calls):
    plan = make_plan(H, W, P, O)
    seed = 9
    ops_in = operands(plan, C, H * W + C)
    mdev = ops.member_ids(MEMBERS, DEV)
    state = torch.tensor([T_ROW, calls, 0], dtype=torch.int32, device=DEV)
    got = run_members(plan, ops_in, rhos, state, None, mdev, seed)
    zb = ops.randn_members(mdev, (C, H, W), seed, j=1 + calls)[None].contiguous()  # [1, R, C, H, W], indexed by state[2] = 0
    want = run_tiled(plan, ops_in, rhos, state, zb, seed)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    assert not torch.equal(got[0], ops_in[0])
    same(got, want)
    if rhos is not None:  # the hand-over is the blend, finite where the NaN history of a zero rho stood
        assert torch.isfinite(got[3]).all() and torch.isfinite(got[4]).all()
    assert state.cpu().tolist() == [T_ROW, calls, 0]


@pytest.mark.parametrize("H,W,P,O", GEOMS)
def test_nothing_is_drawn_or_read_where_c_is_zero(H, W, P, O):
    plan = make_plan(H, W, P, O)
    ops_in = operands(plan, 1, 3)
    mdev = ops.member_ids(MEMBERS, DEV)
    state = torch.tensor([T_ROW, 2, 1], dtype=torch.int32, device=DEV)
    zb = torch.full((2, R, 1, H, W), NAN, device=DEV)
    got = run_members(plan, ops_in, None, state, zb, mdev, 0, c=0.0)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    same(got, run_tiled(plan, ops_in, None, state, zb, 0, c=0.0))
    same(got, run_members(plan, ops_in, None, state, None, mdev, 5, c=0.0))  # nor drawn: the seed does not matter


@pytest.mark.parametrize("rhos", [None, (0.37, 0.81)])
@pytest.mark.parametrize("H,W,P,O", GEOMS)
def test_injected_noise_equals_the_tiled_step(H, W, P, O, rhos):
    plan = make_plan(H, W, P, O)
    ops_in = operands(plan, 2, 11)
    g = torch.Generator().manual_seed(5)
    zb = rand((3, R, 2, H, W), g)
    state = torch.tensor([T_ROW, 4, 2], dtype=torch.int32, device=DEV)  # the third draw of z_base
    got = run_members(plan, ops_in, rhos, state, zb, ops.member_ids(MEMBERS, DEV), 9)
    same(got, run_tiled(plan, ops_in, rhos, state, zb, 9))
    other = run_members(plan, ops_in, rhos, torch.tensor([T_ROW, 4, 1], dtype=torch.int32, device=DEV), zb, ops.member_ids(MEMBERS, DEV), 9)
    assert not torch.equal(other[0], got[0])


# ---- 2. against the member step on one window ------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [0, 5])
@pytest.mark.parametrize("rhos", [None, (0.37, 0.81)])
@pytest.mark.parametrize("C", [1, 2])
def test_one_window_equals_the_member_step(C, rhos, calls):
    plan = make_plan(32, 32, 32, 0)
    assert plan.grid == (1, 1, 32, 32)
    seed = 13
    ops_in = operands(plan, C, 17 + C, poison=False)
    x, cond, rp, ep, r_t, e_t = ops_in
    mdev = ops.member_ids(MEMBERS, DEV)
    state = torch.tensor([T_ROW, calls, 0], dtype=torch.int32, device=DEV)
    x1, x_t, xa_t, h0, h1 = run_members(plan, ops_in, rhos, state, None, mdev, seed)
    x0, xa0, (g0, g1) = x.clone(), torch.full_like(x, NAN), history(rhos, rp, ep)
    ops.drift_reverse_step_members_dev(x0, r_t, e_t, g0, g1, None, cond, xa0, coef_of(rhos), state, mdev, seed)
    assert torch.equal(x1, x0) and torch.equal(xa_t, xa0) and torch.equal(x_t, x0)
    same((h0, h1), (g0, g1))
    assert torch.isfinite(x1).all() and not torch.equal(x1, x)


# ---- 3. rows are independent --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhos", [None, (0.37, 0.81)])
def test_a_row_does_not_depend_on_the_rows_beside_it(rhos):
    H, W, P, O = GEOMS[0]
    plan = make_plan(H, W, P, O)
    nwin = plan.ny * plan.nx
    ops_in = operands(plan, 2, 23)
    state = torch.tensor([T_ROW, 3, 0], dtype=torch.int32, device=DEV)
    mdev = ops.member_ids(MEMBERS, DEV)
    got = run_members(plan, ops_in, rhos, state, None, mdev, 9)
    for r in range(R):
        one = tuple(t[r * (nwin if k >= 4 else 1):(r + 1) * (nwin if k >= 4 else 1)].contiguous() for k, t in enumerate(ops_in))
        alone = run_members(plan, one, rhos, state, None, ops.member_ids(MEMBERS[r:r + 1], DEV), 9)
        same(alone, tuple(None if t is None else t[r * (nwin if k in (1, 2) else 1):(r + 1) * (nwin if k in (1, 2) else 1)]
                          for k, t in enumerate(got)))
    assert not torch.equal(run_members(plan, ops_in, rhos, state, None, mdev, 10)[0], got[0])  # the draw moves with the seed
    swapped = run_members(plan, ops_in, rhos, state, None, ops.member_ids(MEMBERS[::-1], DEV), 9)[0]
    assert not torch.equal(swapped[0], got[0][0]) and torch.equal(swapped[1], got[0][1])  # and with the member id, of that row alone


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_the_step_refuses_bad_arguments_and_touches_nothing():
    plan = make_plan(32, 32, 16, 0)
    g = torch.Generator().manual_seed(2)
    x = rand((R, 1, 32, 32), g)
    keep = x.clone()
    cond, h0, h1 = (rand((R, 1, 32, 32), g) for _ in range(3))
    bufs = [rand((R * 4, 1, 16, 16), g) for _ in range(4)]
    state = torch.tensor([T_ROW, 0, 0], dtype=torch.int32, device=DEV)
    mdev = ops.member_ids(MEMBERS, DEV)
    c3, c5 = coef_of(None), coef_of((0.5, 0.5))
    step = ops.drift_reverse_step_tiled_members_dev
    with pytest.raises(Exception):  # W = 36 on a 32-wide plan
        wide = rand((R, 1, 32, 36), g)
        step(wide, bufs[0], bufs[1], None, None, None, torch.zeros_like(wide), bufs[2], bufs[3], plan, c3, state, mdev, 0)
    with pytest.raises(Exception):  # no member ids
        step(x, bufs[0], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c3, state, None, 0)
    with pytest.raises(Exception):  # R = 0
        step(x[:0], bufs[0][:0], bufs[1][:0], None, None, None, cond[:0], bufs[2][:0], bufs[3][:0], plan, c3, state, mdev[:0], 0)
    with pytest.raises(Exception):  # a 3-row table takes no history
        step(x, bufs[0], bufs[1], h0, h1, None, cond, bufs[2], bufs[3], plan, c3, state, mdev, 0)
    with pytest.raises(Exception):  # a 5-row table needs it
        step(x, bufs[0], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c5, state, mdev, 0)
    with pytest.raises(Exception):  # one buffer for predictions and window inputs
        step(x, bufs[0], bufs[1], None, None, None, cond, bufs[0], bufs[3], plan, c3, state, mdev, 0)
    with pytest.raises(Exception):  # a window buffer one row short
        step(x, bufs[0][:-1], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c3, state, mdev, 0)
    with pytest.raises(Exception):  # one member id short
        step(x, bufs[0], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c3, state, mdev[:-1], 0)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    step(x, bufs[0], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c3, state, mdev, 0)  # and the good call is taken
    assert not torch.equal(x, keep) and torch.isfinite(x).all()


# ---- 5. whole chains on pointwise nets ---------------------------------------------------------------------------------------------
def zeros_net(a, b, t, names, text_encoder, image_context=None):
    return torch.zeros_like(a)


def mix_net(a, b, t, names, text_encoder, image_context=None):
    return 0.5 * a + 0.25 * b


S, K, SEED = 3, 5, 3
IDS = [5, 2, 9]


def chain_sde(net, **kw):
    sde = driftSDE(nets=dict(drift_net=net, noise_net=net), T=20, eta=1.0, sample_T=K, tiled_ensemble=True, **kw)
    sde.set_gpu(torch.device(DEV))
    sde.set_seed(SEED)
    return sde


@pytest.fixture(scope="module")
def cond():
    g = torch.Generator().manual_seed(1)
    return (torch.rand(1, 1, 48, 64, generator=g) * 2 - 1).to(DEV)


def ensemble(sde, cond, **kw):
    kw.setdefault("members", IDS)
    kw.setdefault("num_samples", S)
    samples = sde.reverse_ddpm_ensemble(cond, ["x"] * cond.shape[0], None, return_samples=True, **kw)[2].clone()
    assert sde.last_steps == K and torch.isfinite(samples).all()
    return samples


@pytest.fixture(scope="module")
def mix_base(cond):
    """the members of one tiled ensemble on mix_net, tile 16 / overlap 4, default grouping: the reference of the chain tests"""
    sde = chain_sde(mix_net, tile=16, tile_overlap=4)
    base = ensemble(sde, cond)
    assert sde.last_mode == "graph" and sde.last_tiles == (4, 5, 16, 16) and sde.last_members.tolist() == [IDS]
    return base


def test_grouping_and_chunking_do_not_change_a_member(cond, mix_base):
    sde = chain_sde(mix_net, tile=16, tile_overlap=4)
    nwin = 20
    assert mix_base.shape == (1, S, 1, 48, 64) and not torch.equal(mix_base[0, 0], mix_base[0, 1])
    for rows, mb in ((nwin, 16), (10 ** 6, 16), (128, 4), (nwin, 4)):
        sde.set_num_samples(S, max_batch=mb, max_chain_rows=rows)
        assert torch.equal(ensemble(sde, cond), mix_base), (rows, mb)
        assert sde.last_mode == "graph" and sde.last_tiles == (4, 5, 16, 16)
    sde.set_num_samples(S, max_batch=16, max_chain_rows=128)
    off = (sde._off, sde._calls)
    for s, m in enumerate(IDS):
        one = ensemble(sde, cond, num_samples=1, members=[m])
        assert torch.equal(one[0, 0], mix_base[0, s]), m
    assert (sde._off, sde._calls) == off == (0, 0)
    mean, std = sde.reverse_ddpm_ensemble(cond, ["x"], None, members=IDS)
    want = ops.ensemble_stats(mix_base)
    assert torch.equal(mean, want[0]) and torch.equal(std, want[1]) and float(std.mean()) > 0


def test_two_images_are_grouped_like_one(cond, mix_base):
    """B = 2: rows b*S + s; chains of one, two and all six rows give every member the bits of its own single-row call"""
    sde = chain_sde(mix_net, tile=16, tile_overlap=4)
    both = torch.cat([cond, cond.flip(-1)]).contiguous()
    ids = IDS + [11, 12, 13]
    runs = []
    for rows in (20, 45, 128):
        sde.set_num_samples(S, max_chain_rows=rows)
        runs.append(ensemble(sde, both, members=ids))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert torch.equal(runs[0][0], mix_base[0])


def test_injected_noise_equals_the_device_noise(cond, mix_base):
    sde = chain_sde(mix_net, tile=16, tile_overlap=4)
    mdev = ops.member_ids(IDS, DEV)
    noises = torch.stack([ops.randn_members(mdev, (1, 48, 64), SEED, j=j) for j in range(1, K + 1)]).contiguous()
    assert noises.shape == (K, S, 1, 48, 64)
    assert torch.equal(ensemble(sde, cond, noises=noises), mix_base)
    sde.set_num_samples(S, max_chain_rows=20)  # injected per group
    assert torch.equal(ensemble(sde, cond, noises=noises), mix_base)
    assert not torch.equal(ensemble(sde, cond, noises=noises.flip(1).contiguous()), mix_base)


def test_the_noise_does_not_depend_on_the_tiling(cond):
    sde = chain_sde(zeros_net)
    plain = ensemble(sde, cond)
    assert sde.last_tiles is None and sde.last_mode == "graph"
    assert float((plain - cond).std()) > 0.3 and not torch.equal(plain[0, 0], plain[0, 1])
    for tile, overlap, grid in ((16, 4, (4, 5, 16, 16)), (32, 8, (2, 3, 32, 32)), ([16, 32], 0, (3, 2, 16, 32))):
        sde.set_tiling(tile, overlap)
        out = ensemble(sde, cond)
        assert sde.last_tiles == grid and sde.last_mode == "graph"
        assert torch.equal(out, plain), (tile, overlap)
        assert (sde._off, sde._calls) == (0, 0)
    sde.set_seed(SEED + 1)
    assert not torch.equal(ensemble(sde, cond), plain)


@pytest.mark.parametrize("order", [1, 2])
def test_abutting_windows_equal_the_untiled_ensemble(cond, order):
    """overlap 0: every pixel has one window, the blend is 1.0f*r, and pointwise nets see the same values in a window as in the image"""
    sde = chain_sde(mix_net, solver_order=order)
    plain = ensemble(sde, cond)
    assert sde.last_tiles is None and sde.last_solver_order == order
    sde.set_tiling(16, 0)
    tiled = ensemble(sde, cond)
    assert sde.last_tiles == (3, 4, 16, 16) and sde.last_solver_order == order and sde.last_mode == "graph"
    assert torch.equal(tiled, plain)
    if order == 2:
        first = ensemble(chain_sde(mix_net, tile=16, tile_overlap=0), cond)
        assert not torch.equal(first, tiled)  # the second order is not the first


def test_an_image_inside_the_window_takes_the_untiled_path():
    g = torch.Generator().manual_seed(4)
    small = (torch.rand(1, 1, 16, 16, generator=g) * 2 - 1).to(DEV)
    sde = chain_sde(mix_net, tile=16)
    got = ensemble(sde, small)
    assert sde.last_tiles is None
    assert torch.equal(got, ensemble(chain_sde(mix_net), small))
    with pytest.raises(ValueError):  # a width that is no multiple of 4, refused at call time
        sde.reverse_ddpm_ensemble(torch.zeros(1, 1, 48, 62, device=DEV), ["x"], None, num_samples=S)
    off = chain_sde(mix_net, tile=16)
    off.set_tiled_ensemble(False)
    with pytest.raises(ValueError, match="num_samples"):  # without the switch the call is refused as before
        off.reverse_ddpm_ensemble(small, ["x"], None, num_samples=S)


# ---- 6. the pipeline nets, the model and the driver -------------------------------------------------------------------------------
T = 6


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0,
                                sde_overrides=dict(tile=32, tile_overlap=8, num_samples=2, tiled_ensemble=True, sample_T=3))
    model.set_eval()
    return model, sde


def test_model_test_runs_a_tiled_ensemble(built):
    model, sde = built
    assert sde.tiled_ensemble is True and sde.num_samples == 2 and sde.tile == (32, 32)
    batch = make_batch(1, 48, seed=13)
    sde.set_interval(0.5)
    try:
        sde.set_seed(5)
        model.feed_data(batch)
        off = (sde._off, sde._calls)
        model.test(return_samples=True)
        assert (sde._off, sde._calls) == off
        assert sde.last_mode == "graph" and sde.last_tiles == (2, 2, 32, 32) and sde.last_steps == 3
        out, std, samples = model.output, model.output_std, model.samples
        assert out.shape == (1, 1, 48, 48) and std.shape == out.shape and samples.shape == (1, 2, 1, 48, 48)
        assert torch.isfinite(out).all() and torch.isfinite(std).all() and float(std.max()) > 0
        sums, counts, _ = model.score_ensemble()
        assert sums.shape == (1, 3) and counts.shape == (1, 4) and int(counts[0, :3].sum()) == 48 * 48
        lo, med, hi = model.output_lo, model.output_median, model.output_hi
        assert bool((lo <= med).all()) and bool((med <= hi).all())
        srt = torch.sort(samples, dim=1).values
        ks = sde.last_order_stats["ks"]
        assert torch.equal(lo, srt[:, ks[0]]) and torch.equal(hi, srt[:, ks[1]])
        assert torch.equal(med, ops.axpby(srt[:, ks[2]].contiguous(), srt[:, ks[3]].contiguous(), 0.5, 0.5))
        ids = sde.last_members.tolist()[0]
        for s, m in enumerate(ids):  # a member against its own single-row run: bits, as the untiled ensemble's chunking test asserts
            one = sde.reverse_ddpm_ensemble(model.input, model.names, model.text_encoder, reverse_type=model.optimize_target,
                                            optimize_type=model.optimize_type, image_context=model.A_emb, num_samples=1, members=[m],
                                            return_samples=True)[2]
            assert sde.last_tiles == (2, 2, 32, 32)
            assert torch.equal(one[0, 0], samples[0, s]), m
        sde.set_num_samples(2, max_chain_rows=4)  # one member per chain
        sde.set_seed(5)
        model.feed_data(batch)
        model.test(return_samples=True)
        assert torch.equal(model.samples, samples) and torch.equal(model.output, out)
    finally:
        sde.set_interval(None)
        sde.set_num_samples(2, max_chain_rows=128)


def test_testum_tiled_ensemble_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_tens").replace("image_size: 64", "image_size: 32").replace("T: 100", "T: 8")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    args = ["-opt", str(cfg), "--random-init", "--limit", "1", "--tile", "16", "--num-samples", "2", "--sample-T", "3"]
    res = testUM.main(args + ["--tiled-ensemble"])
    out = capsys.readouterr().out
    assert "(3 steps)" in out and "2 samples per image" in out and "2x2 windows of 16x16" in out, out[-500:]
    done = [v for v in res.values() if v['num']]
    assert sum(v['num'] for v in done) == 1 and all(s > 0 for v in done for s in v['STD'])
    with pytest.raises(ValueError, match="num_samples"):
        testUM.main(args)
