"""Tiled sampling (driftSDE tile / tile_overlap) on the device: the window gather against torch slicing (bits), the fused tiled step
against the plain steps where every pixel has one window (bits) and against an fp64 restatement of its stated operation order where
windows blend (bounds derived from that order), and whole chains: a single window against the plain chain (bits), the noise against the
tiling (bits), a per-step restatement on pointwise nets, the pipeline nets (graph against eager, chunking), and the model / testUM
surface."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import TilePlan, driftSDE  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
TP1 = 8
U = 2.0 ** -24  # unit roundoff of fp32


def gamma(k):
    return k * U / (1 - k * U)


def make_plan(H, W, P, O):
    P = (P, P) if isinstance(P, int) else tuple(P)
    return TilePlan(H, W, P, (O, O)).to(DEV)


def torch_gather(full, plan):
    """full [B, C, H, W] (any device) -> [B*ny*nx, C, Ph, Pw] by indexing, row (b*ny + iy)*nx + ix"""
    yy, xx = plan.window_index()
    B, C = full.shape[:2]
    t = full[:, :, yy.to(full.device), xx.to(full.device)]  # [B, C, nwin, Ph, Pw]
    return t.permute(0, 2, 1, 3, 4).reshape(B * plan.ny * plan.nx, C, plan.Ph, plan.Pw).contiguous()


def table(rows, t):
    tb = torch.full((len(rows), TP1), float("nan"), dtype=torch.float32)
    tb[:, t] = torch.tensor(rows, dtype=torch.float32)
    return tb.to(DEV)


def axis_weights(ax):
    """[n, L] fp32: the blend weight of every window at every coordinate of an axis"""
    n, L = ax["n"], len(ax["first"])
    wt = np.zeros((n + 1, L), dtype=np.float32)
    c = np.arange(L)
    wt[ax["first"], c] = ax["w0"]
    wt[ax["first"] + 1, c] += ax["w1"]
    assert not wt[n].any()
    return wt[:n]


def poison_unweighted(tiles, plan):
    """NaN in every window pixel whose blend weight is exactly 0: the step must not read it.  -> number of pixels poisoned"""
    wy, wx = axis_weights(plan.y), axis_weights(plan.x)
    yy, xx = plan.window_index()
    iy = torch.arange(plan.ny).repeat_interleave(plan.nx)[:, None, None].expand_as(yy)
    ix = torch.arange(plan.nx).repeat(plan.ny)[:, None, None].expand_as(xx)
    w = torch.from_numpy(wy)[iy, yy] * torch.from_numpy(wx)[ix, xx]  # [nwin, Ph, Pw]
    dead = (w == 0)
    R = tiles.shape[0]
    mask = dead[None].expand(R // dead.shape[0], -1, -1, -1).reshape(R, 1, plan.Ph, plan.Pw).expand_as(tiles)
    tiles[mask.to(tiles.device)] = float("nan")
    return int(dead.sum())


def blend_ref(tiles, plan, B):
    """The blend of include/idiff.h in fp64 from the plan's fp32 tables: slots (iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1), weight
    wy*wx, slots of weight 0 skipped.  tiles: fp32 [B*ny*nx, C, Ph, Pw] on the host -> (blend, sum |w r|, terms), [B, C, H, W] / [H, W]"""
    ny, nx, Ph, Pw = plan.grid
    H, W, C = plan.H, plan.W, tiles.shape[1]
    t = tiles.double().numpy().reshape(B, ny, nx, C, Ph, Pw).transpose(1, 2, 4, 5, 0, 3)  # [ny, nx, Ph, Pw, B, C]
    oy, ox = np.asarray(plan.y["origins"]), np.asarray(plan.x["origins"])
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    val, mag, m = np.zeros((H, W, B, C)), np.zeros((H, W, B, C)), np.zeros((H, W), dtype=np.int64)
    for sy in (0, 1):
        for sx in (0, 1):
            wy = (plan.y["w0"], plan.y["w1"])[sy][:, None]
            wx = (plan.x["w0"], plan.x["w1"])[sx][None, :]
            live = (wy * wx) != 0  # the fp32 product the kernel tests
            w64 = wy.astype(np.float64) * wx.astype(np.float64)
            iy = np.broadcast_to(np.clip(plan.y["first"] + sy, 0, ny - 1)[:, None], (H, W))
            ix = np.broadcast_to(np.clip(plan.x["first"] + sx, 0, nx - 1)[None, :], (H, W))
            ly, lx = np.clip(y - oy[iy], 0, Ph - 1), np.clip(x - ox[ix], 0, Pw - 1)
            with np.errstate(invalid="ignore"):
                term = np.where(live[..., None, None], w64[..., None, None] * t[iy, ix, ly, lx], 0.0)
            val += term
            mag += np.abs(term)
            m += live
    assert m.min() >= 1 and m.max() <= 4
    return val.transpose(2, 3, 0, 1), mag.transpose(2, 3, 0, 1), m


def step_bound(m, mag_r, mag_e, a, b, c, x, Rt, Et, z, err_r=None, err_e=None):
    """Per pixel, from the operation order and not from measurement.  The blend of m <= 4 terms rounds wy*wx once, each product once and
    the sum m - 1 times: |R^ - ref| <= gamma_{m+1} sum |w_i r_i| (err_r / err_e hand in a larger prediction error, see the order-2
    restatement); the update ((x - a R) - b e) + c z: gamma_3 (|x| + |a R| + |b e| + |c z|).  The prediction errors enter the update
    through a and b."""
    g = gamma(m + 1)[None, None]
    err_r = g * mag_r if err_r is None else err_r
    err_e = g * mag_e if err_e is None else err_e
    return abs(a) * err_r + abs(b) * err_e + gamma(3) * (np.abs(x) + np.abs(a * Rt) + np.abs(b * Et) + np.abs(c * z))


def rand(shape, g, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(DEV)


# ---- 1. the gather --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P,O", [(24, 40, 16, 4), (40, 40, 16, 8), (36, 36, 16, 8), (32, 32, 32, 4), (48, 64, (16, 32), 0)])
def test_tile_gather_equals_slicing(H, W, P, O):
    plan = make_plan(H, W, P, O)
    g = torch.Generator().manual_seed(H + W)
    full = rand((2, 1, H, W), g)
    tiles = ops.tile_gather(full, plan)
    ny, nx, Ph, Pw = plan.grid
    assert tiles.shape == (2 * ny * nx, 1, Ph, Pw)
    for b in range(2):
        for iy, oy in enumerate(plan.y["origins"]):
            for ix, ox in enumerate(plan.x["origins"]):
                assert torch.equal(tiles[(b * ny + iy) * nx + ix], full[b, :, oy:oy + Ph, ox:ox + Pw]), (b, iy, ix)
    assert torch.equal(tiles, torch_gather(full, plan))
    full3 = rand((1, 3, H, W), g)  # more than one channel
    assert torch.equal(ops.tile_gather(full3, plan), torch_gather(full3, plan))


def test_tiled_entry_points_refuse_bad_arguments():
    plan = make_plan(32, 32, 16, 0)
    x = torch.zeros(1, 1, 32, 32, device=DEV)
    with pytest.raises(Exception):  # another image size than the plan's
        ops.tile_gather(torch.zeros(1, 1, 32, 36, device=DEV), plan)
    with pytest.raises(ValueError):
        make_plan(32, 30, 16, 0)
    bufs = [torch.zeros(4, 1, 16, 16, device=DEV) for _ in range(4)]
    state = torch.tensor([5, 0, 0], dtype=torch.int32, device=DEV)
    c3, c5 = table([0.1, 0.1, 0.0], 5), table([0.1, 0.1, 0.0, 0.5, 0.5], 5)
    cond, h0, h1 = (torch.zeros_like(x) for _ in range(3))
    with pytest.raises(Exception):  # a 3-row table takes no history
        ops.drift_reverse_step_tiled_dev(x, bufs[0], bufs[1], h0, h1, None, cond, bufs[2], bufs[3], plan, c3, state, 0, 256)
    with pytest.raises(Exception):  # a 5-row table needs it
        ops.drift_reverse_step_tiled_dev(x, bufs[0], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c5, state, 0, 256)
    with pytest.raises(Exception):  # one buffer for predictions and window inputs
        ops.drift_reverse_step_tiled_dev(x, bufs[0], bufs[1], None, None, None, cond, bufs[0], bufs[3], plan, c3, state, 0, 256)
    with pytest.raises(Exception):  # window buffers of another grid
        ops.drift_reverse_step_tiled_dev(x, bufs[0][:2], bufs[1], None, None, None, cond, bufs[2], bufs[3], plan, c3, state, 0, 256)
    assert not x.any()


# ---- 2. the step where every pixel has one window: the plain steps, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("device_noise", [False, True])
@pytest.mark.parametrize("rhos", [None, (0.37, 0.81), (0.0, 0.81), (0.0, 0.0)])
def test_tiled_step_on_abutting_windows_equals_the_plain_steps(rhos, device_noise):
    B, H = 2, 32
    plan = make_plan(H, H, 16, 0)
    assert plan.grid == (2, 2, 16, 16) and not plan.y["w1"].any() and not plan.x["w1"].any()
    shp = (B, 1, H, H)
    n = B * H * H
    g = torch.Generator().manual_seed(7 + (0 if rhos is None else int(100 * rhos[0] + 10 * rhos[1])))
    x, r, e, rp, ep, cond = (rand(shp, g) for _ in range(6))
    zb = None if device_noise else rand((3,) + shp, g)
    t, a, b, c = 5, 0.0713, 0.1291, 0.0577
    seed, nper, off = 9, n // 4, 11
    state = torch.tensor([t, 4, 2], dtype=torch.int32, device=DEV)
    r_t, e_t = ops.tile_gather(r, plan), ops.tile_gather(e, plan)
    x_t, xa_t = torch.full_like(r_t, float("nan")), torch.full_like(r_t, float("nan"))
    if rhos is None:
        coef = table([a, b, c], t)
        x0, xa0 = x.clone(), torch.empty_like(x)
        ops.drift_reverse_step_dev(x0, r, e, zb, cond, xa0, coef, state, seed, nper, off)
        x1 = x.clone()
        ops.drift_reverse_step_tiled_dev(x1, r_t, e_t, None, None, zb, cond, x_t, xa_t, plan, coef, state, seed, nper, off)
    else:
        coef = table([a, b, c, rhos[0], rhos[1]], t)
        nan = torch.full(shp, float("nan"), device=DEV)  # a clock whose rho is 0 does not read its history
        hist = [(rp if rhos[0] else nan), (ep if rhos[1] else nan)]
        x0, xa0, rp0, ep0 = x.clone(), torch.empty_like(x), hist[0].clone(), hist[1].clone()
        ops.drift_reverse_step2_dev(x0, r, e, rp0, ep0, zb, cond, xa0, coef, state, seed, nper, off)
        x1, rp1, ep1 = x.clone(), hist[0].clone(), hist[1].clone()
        ops.drift_reverse_step_tiled_dev(x1, r_t, e_t, rp1, ep1, zb, cond, x_t, xa_t, plan, coef, state, seed, nper, off)
        assert torch.equal(rp1, r) and torch.equal(ep1, e)  # the history is the blended prediction: here the prediction itself
    assert torch.isfinite(x1).all() and not torch.equal(x1, x)
    assert torch.equal(x0, x1)
    assert torch.equal(x_t, torch_gather(x1, plan)) and torch.equal(xa_t, torch_gather(xa0, plan))
    assert torch.equal(xa_t, torch_gather(x1 - cond, plan))
    assert state.cpu().tolist() == [t, 4, 2]
    if device_noise:  # the draw moves with the seed
        x2 = x.clone()
        hist2 = (None, None) if rhos is None else (hist[0].clone(), hist[1].clone())
        ops.drift_reverse_step_tiled_dev(x2, r_t, e_t, hist2[0], hist2[1], None, cond, x_t, xa_t, plan, coef, state, seed + 1, nper, off)
        assert not torch.equal(x2, x1)


# ---- 3. the blend against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P,O", [(40, 40, 16, 8), (24, 40, 16, 4), (36, 36, 16, 8)])
def test_tiled_step_blend_against_fp64(H, W, P, O):
    """Independent random window predictions, so overlapping windows disagree; NaN wherever a window pixel has weight 0 (36 x 36 has
    such pixels: three windows overlap there and the outer one carries no weight).  Bound: step_bound."""
    B = 2
    plan = make_plan(H, W, P, O)
    ny, nx, Ph, Pw = plan.grid
    g = torch.Generator().manual_seed(H * W + O)
    tshape = (B * ny * nx, 1, Ph, Pw)
    r_t, e_t = rand(tshape, g), rand(tshape, g)
    dead = poison_unweighted(r_t, plan)
    assert poison_unweighted(e_t, plan) == dead and (dead > 0) == (H == 36)
    x, cond = rand((B, 1, H, W), g), rand((B, 1, H, W), g)
    zb = rand((2, B, 1, H, W), g)
    t, a, b, c = 3, 0.2713, 0.1291, 0.0577
    coef = table([a, b, c], t)
    state = torch.tensor([t, 0, 1], dtype=torch.int32, device=DEV)
    x1 = x.clone()
    x_t, xa_t = torch.full(tshape, float("nan"), device=DEV), torch.full(tshape, float("nan"), device=DEV)
    ops.drift_reverse_step_tiled_dev(x1, r_t, e_t, None, None, zb, cond, x_t, xa_t, plan, coef, state, 0, B * H * W // 4)
    assert torch.isfinite(x1).all()
    R, mag_r, m = blend_ref(r_t.cpu(), plan, B)
    E, mag_e, _ = blend_ref(e_t.cpu(), plan, B)
    assert m.max() == 4 and m.min() == 1  # corners of four windows and plain interiors are both present
    a_, b_, c_ = (float(coef[k, t]) for k in range(3))
    xd, zd = x.cpu().double().numpy(), zb[1].cpu().double().numpy()
    want = xd - a_ * R - b_ * E + c_ * zd
    bound = step_bound(m, mag_r, mag_e, a_, b_, c_, xd, R, E, zd)
    err = np.abs(x1.cpu().double().numpy() - want)
    print(f"{H}x{W} P={P} O={O}: max |x - ref| = {err.max():.3e}, max err/bound = {(err / bound).max():.3f}, dead window pixels {dead}")
    assert (err <= bound).all()
    assert torch.equal(x_t, torch_gather(x1, plan)) and torch.equal(xa_t, torch_gather(x1 - cond, plan))
    # the blend is a convex combination of windows that disagree: it is not any single window's value
    assert not torch.equal(x1, x)


# ---- 4. whole chains ------------------------------------------------------------------------------------------------------------
T = 6


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(tile=32, tile_overlap=8))
    model.set_eval()
    return model, sde


@pytest.mark.parametrize("opts", [dict(), dict(sample_T=3, order=2)])
def test_a_single_window_chain_equals_the_plain_chain(built, opts):
    model, sde = built
    batch = make_batch(2, 32, seed=5)
    cond, ctx = batch['input'].to(DEV).contiguous(), batch['A_emb'].to(DEV).contiguous()
    sde.set_sample_steps(opts.get("sample_T"))
    sde.set_solver_order(opts.get("order"))
    try:
        sde.set_seed(23)
        plain = sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx).clone()  # 32 x 32 does not exceed the tile
        assert sde.last_mode == "graph" and sde.last_tiles is None
        state = (sde._off, sde._calls)
        sde.set_seed(23)
        tiled = sde.reverse_ddpm_tiled(cond, batch['names'], model.text_encoder, image_context=ctx)
        assert sde.last_mode == "graph" and sde.last_tiles == (1, 1, 32, 32)
        assert sde.last_steps == opts.get("sample_T", T) and sde.last_solver_order == opts.get("order", 1)
        assert (sde._off, sde._calls) == state
        assert torch.isfinite(tiled).all() and torch.equal(plain, tiled)
    finally:
        sde.set_sample_steps(None)
        sde.set_solver_order(None)


def zeros_net(a, b, t, names, text_encoder, image_context=None):
    return torch.zeros_like(a)


def test_the_noise_does_not_depend_on_the_tiling():
    """zero nets, eta = 1: the result is cond + sigma z_0 + sum_k c_k z_k, a function of the pixel's Philox counters alone"""
    sde = driftSDE(nets=dict(drift_net=zeros_net, noise_net=zeros_net), T=20, eta=1.0, sample_T=5)
    sde.set_gpu(torch.device(DEV))
    g = torch.Generator().manual_seed(1)
    cond = (torch.rand(1, 1, 48, 64, generator=g) * 2 - 1).to(DEV)

    def run(seed, tile, overlap=None):
        sde.set_tiling(tile, overlap)
        sde.set_seed(seed)
        out = sde.reverse_ddpm(cond, ["x"], None).clone()
        assert sde.last_steps == 5 and sde.last_mode == "graph"
        return out, sde.last_tiles, (sde._off, sde._calls)

    plain, tiles, acct = run(3, None)
    assert tiles is None and acct == (6 * 48 * 64 // 4, 6)
    assert float((plain - cond).std()) > 0.3
    for tile, overlap, grid in ((16, 4, (4, 5, 16, 16)), (32, 8, (2, 3, 32, 32)), ([16, 32], 0, (3, 2, 16, 32))):
        out, tiles, acct_t = run(3, tile, overlap)
        assert tiles == grid and acct_t == acct
        assert torch.equal(out, plain), (tile, overlap)
    other, _, _ = run(4, 32, 8)
    assert not torch.equal(other, plain)


def mix_net(a, b, t, names, text_encoder, image_context=None):
    return 0.5 * a + 0.25 * b


@pytest.mark.parametrize("order", [1, 2])
def test_tiled_chain_step_by_step_against_fp64(order):
    """Four eager steps on 40 x 40, P = 16, O = 8 with pointwise nets (0.5 a + 0.25 b: exact products, one rounding, the same bits from
    torch on the window inputs the step wrote).  After each step the device x is compared with the fp64 restatement applied to the
    previous DEVICE x: row t_k of the coefficient table, draw k of the injected noise, step_bound.
    Order 2 extrapolates R~ = R + rho (R - Rp) from the previous step's blend before the update, three more roundings on inputs that carry
    their own blend errors err(R), err(Rp) (the restatement keeps its history in fp64):
        err(R~) <= (1 + |rho|) err(R) + |rho| err(Rp) + gamma_3 (|R| + |rho| (|R| + |Rp|)),
    which replaces the blend error in step_bound; the update's term is evaluated on R~, e~.  The ratio to the order-1 form of the bound
    is printed beside it."""
    B, H, K, Tn = 2, 40, 4, 8
    sde = driftSDE(nets=dict(drift_net=mix_net, noise_net=mix_net), T=Tn, eta=1.0, sample_T=K, solver_order=order, tile=16, tile_overlap=8)
    sde.set_gpu(torch.device(DEV))
    sde.hip_graph = False
    g = torch.Generator().manual_seed(order)
    cond = (torch.rand(B, 1, H, H, generator=g) * 2 - 1).to(DEV)
    x = (cond + 0.4 * rand((B, 1, H, H), g)).contiguous()
    noises = rand((K, B, 1, H, H), g)
    plan = sde._tile_plan(H, H, DEV)
    nwin = plan.ny * plan.nx
    stepper = driftSDE.TiledStepper(sde, x, cond, plan, ["x"] * (B * nwin), None, None, noises=noises, timesteps=sde.timesteps,
                                    solver_order=order)
    coef = sde._schedule_tables(sde.timesteps)[0].double().numpy()
    cond_t = torch_gather(cond, plan)
    condd = cond.cpu().double().numpy()
    prev = None  # (R, mag_r, E, mag_e) of the previous step, fp64
    for k, t in enumerate(sde.timesteps[:-1]):
        x_before = x.clone()
        x_t = torch_gather(x_before, plan)
        xa_t = x_t - cond_t
        assert torch.equal(stepper.x_tiles, x_t) and torch.equal(stepper.xa_tiles, xa_t), k
        r_t, e_t = mix_net(xa_t, cond_t, None, None, None), mix_net(xa_t, x_t, None, None, None)
        stepper.run(1)
        assert stepper.mode == "eager"
        R, mag_r, m = blend_ref(r_t.cpu(), plan, B)
        E, mag_e, _ = blend_ref(e_t.cpu(), plan, B)
        a, b, c = coef[0, t], coef[1, t], coef[2, t]
        gm = gamma(m + 1)[None, None]
        err_r, err_e, Rt, Et = gm * mag_r, gm * mag_e, R, E
        if order == 2:
            rho_d, rho_s = coef[3, t], coef[4, t]
            assert (k == 0) == (rho_d == 0.0 and rho_s == 0.0)
            if k > 0:
                Rp, mag_rp, Ep, mag_ep = prev
                Rt, Et = R + rho_d * (R - Rp), E + rho_s * (E - Ep)
                err_r = (1 + abs(rho_d)) * err_r + abs(rho_d) * gm * mag_rp + gamma(3) * (np.abs(R) + abs(rho_d) * (np.abs(R) + np.abs(Rp)))
                err_e = (1 + abs(rho_s)) * err_e + abs(rho_s) * gm * mag_ep + gamma(3) * (np.abs(E) + abs(rho_s) * (np.abs(E) + np.abs(Ep)))
        xd, zd = x_before.cpu().double().numpy(), noises[k].cpu().double().numpy()
        want = xd - a * Rt - b * Et + c * zd
        bound = step_bound(m, mag_r, mag_e, a, b, c, xd, Rt, Et, zd, err_r, err_e)
        plain_form = step_bound(m, mag_r, mag_e, a, b, c, xd, Rt, Et, zd)
        err = np.abs(x.cpu().double().numpy() - want)
        print(f"order {order} step {k} (t = {t}): max |x - ref| = {err.max():.3e}, max err/bound = {(err / bound).max():.3f} "
              f"(order-1 form of the bound: {(err / plain_form).max():.3f})")
        assert (err <= bound).all(), k
        assert float(np.abs(x.cpu().double().numpy() - xd).max()) > 1e-3  # the step moved the image
        prev = (R, mag_r, E, mag_e)
    assert stepper.steps_done == K and (sde._off, sde._calls) == (K * B * H * H // 4, K)
    assert torch.equal(stepper.xa_tiles, torch_gather(x - cond, plan))
    assert float(np.abs(x.cpu().double().numpy() - condd).max()) < 10


def test_tiled_chain_on_the_pipeline_nets(built):
    """48 x 64, tile 32, overlap 8: 2 x 3 windows through the random-init pipeline nets"""
    model, sde = built
    batch = make_batch(1, 48, 64, seed=11)
    cond, ctx = batch['input'].to(DEV).contiguous(), batch['A_emb'].to(DEV).contiguous()
    nper = 48 * 64 // 4

    def run(graph, max_batch):
        sde.hip_graph = graph
        sde.set_num_samples(None, max_batch=max_batch)
        sde.set_seed(31)
        out = sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx).clone()
        assert sde.last_mode == ("graph" if graph else "eager") and sde.last_tiles == (2, 3, 32, 32) and sde.last_steps == T
        assert (sde._off, sde._calls) == ((1 + T) * nper, 1 + T)  # the x_T draw and T steps of a 48 x 64 image
        return out

    try:
        base = run(True, 16)
        assert base.shape == (1, 1, 48, 64) and torch.isfinite(base).all()
        assert float((base - cond).abs().max()) > 1e-3
        assert torch.equal(run(False, 16), base)
        assert torch.equal(run(True, 2), base)  # three chunks of two window rows
        assert torch.equal(run(True, 4), base)  # chunks of four and two
    finally:
        sde.hip_graph = True
        sde.set_num_samples(None, max_batch=16)


# ---- 5. the model and the driver ------------------------------------------------------------------------------------------------
def test_model_test_dispatches_on_the_option(built):
    model, sde = built
    big, small = make_batch(1, 48, 64, seed=13), make_batch(1, 32, seed=13)
    sde.set_seed(5)
    model.feed_data(big)
    model.test()
    assert sde.last_tiles == (2, 3, 32, 32) and model.output.shape == (1, 1, 48, 64) and torch.isfinite(model.output).all()
    out = model.output.clone()
    sde.set_seed(5)
    model.feed_data(big)
    want = sde.reverse_ddpm_tiled(model.input, model.names, model.text_encoder, reverse_type=model.optimize_target,
                                  optimize_type=model.optimize_type, image_context=model.A_emb)
    assert torch.equal(out, want)
    model.feed_data(small)  # does not exceed the tile: the plain chain
    model.test()
    assert sde.last_tiles is None and model.output.shape == (1, 1, 32, 32)
    with pytest.raises(ValueError):
        sde.set_num_samples(2)
    with pytest.raises(ValueError):  # a width that is no multiple of 4, refused at call time
        sde.reverse_ddpm(torch.zeros(1, 1, 48, 62, device=DEV), ["x"], None)


def test_testum_tile_options(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_tile").replace("T: 100", "T: 8")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    assert "image_size: 64" in txt
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    res = testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--tile", "32", "--tile-overlap", "8", "--sample-T", "4"])
    out = capsys.readouterr().out
    assert "(4 steps)" in out and "3x3 windows of 32x32" in out, out[-500:]
    assert sum(v['num'] for v in res.values()) == 1
    for v in res.values():
        assert all(np.isfinite(p) for p in v['PSNR'])
    testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--tile", "32", "64", "--sample-T", "3"])
    assert "3x1 windows of 32x64" in capsys.readouterr().out  # default overlap 4: ceil(60 / 28) windows down, one across
    with pytest.raises(ValueError, match="num_samples"):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--num-samples", "2", "--tile", "32"])
