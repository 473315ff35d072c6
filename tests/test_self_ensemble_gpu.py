"""Geometric self-ensembles (driftSDE self_ensemble) on the device.  idiff_dihedral_rows is a permutation, so every comparison is
torch.equal: the kernel against the torch expression of its contract (signed zeros, infinities and a NaN payload on the int32 view), the
row rule, the inverses and the refusals; then whole chains -- every member against its composition (a one-member call on the turned
input, turned back) on the pipeline nets, per call, through held graphs and as tiled chains on position-dependent analytic nets -- and
the model / testUM surface."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dihedral_ref import dihedral_rows_ref, dihedral_torch  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import driftSDE, inverse_code, order_stat_indices, self_ensemble_codes  # noqa: E402
from instancediff_amd.utils.synthetic import ARTIFACT_TYPES, make_batch  # noqa: E402

DEV = "cuda"
DIHEDRAL = [0, 4, 2, 6, 1, 5, 3, 7]
NAN_BITS = 0x7FC12345  # a quiet NaN with a payload


def bits(t):
    return t.contiguous().view(torch.int32)


def special(shape, seed):
    """normals with a -0.0, a +inf, a -inf and a NaN with a payload in every plane"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1, shape[-2] * shape[-1])
    n = flat.shape[1]
    flat[:, 1] = -0.0
    flat[:, n // 3] = float("inf")
    flat[:, n // 2 + 1] = float("-inf")
    flat.view(torch.int32)[:, n - 2] = NAN_BITS
    return x.to(DEV)


# ---- 1. the kernel against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,H,W", [(1, 4, 4), (3, 68, 68), (1, 128, 128), (2, 6, 8), (1, 70, 132)])
def test_kernel_equals_the_torch_expression(C_, H, W):
    """(1,4,4): one float4 per row, one partial tile; (3,68,68): a full tile and a 4-wide edge tile on both axes; (1,128,128): two
    tiles per axis, no edge; (2,6,8) and (1,70,132): H no multiple of 4, not square: the four codes without the transposition"""
    x = special((2, C_, H, W), H * W)
    assert int((bits(x) == NAN_BITS).sum()) == 2 * C_
    codes = range(8) if H == W else (0, 2, 4, 6)
    seen = []
    for k in codes:
        out = ops.dihedral_rows(x, [k])
        assert out.shape == x.shape
        assert torch.equal(bits(out), bits(dihedral_torch(x, k))), k
        seen.append(bits(out).clone())
    assert torch.equal(seen[0], bits(x))  # code 0 copies
    for i in range(len(seen)):
        for j in range(i):
            assert not torch.equal(seen[i], seen[j]), (i, j)
    if H * W <= 64:  # and the numpy mirror of the header's index rule, element by element
        for k in codes:
            want = dihedral_rows_ref(x.cpu().numpy().view(np.int32), [k], S=1, in_rep=1)
            assert np.array_equal(bits(ops.dihedral_rows(x, [k])).cpu().numpy(), want), k


def test_transposing_codes_need_a_square_image():
    x = special((1, 1, 8, 12), 0)
    for k in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="square"):
            ops.dihedral_rows(x, [0, k])


# ---- 2. the row rule ----------------------------------------------------------------------------------------------------------------
def test_rows_take_the_code_of_their_member_and_the_input_of_their_image():
    x = special((2, 2, 68, 68), 7)
    codes = [0, 5, 6, 3]
    out = ops.dihedral_rows(x, codes, S=3, in_rep=3)  # R = 6, S = 3, period = 4
    assert out.shape == (6, 2, 68, 68)
    for r in range(6):
        k = codes[(r % 3) % 4]
        assert torch.equal(bits(out[r]), bits(dihedral_torch(x[r // 3], k))), r
    want = dihedral_rows_ref(x.cpu().numpy().view(np.int32), codes, S=3, in_rep=3)
    assert np.array_equal(bits(out).cpu().numpy(), want)


def test_members_beyond_the_period_wrap():
    x = special((10, 1, 8, 8), 8)
    out = ops.dihedral_rows(x, DIHEDRAL, S=10)  # R = 10, S = 10, period = 8, in_rep = 1
    for r in range(10):
        assert torch.equal(bits(out[r]), bits(dihedral_torch(x[r], DIHEDRAL[r % 8]))), r
    assert torch.equal(bits(out[8]), bits(x[8])) and torch.equal(bits(out[9]), bits(x[9].flip(-1)))
    # S None: the rows themselves count; S = 5: member r % 5
    assert torch.equal(bits(ops.dihedral_rows(x, DIHEDRAL)), bits(out))
    five = ops.dihedral_rows(x, DIHEDRAL, S=5)
    for r in range(10):
        assert torch.equal(bits(five[r]), bits(dihedral_torch(x[r], DIHEDRAL[r % 5]))), r


def test_the_inverse_codes_restore_the_input():
    x = special((8, 2, 68, 68), 9)
    there = ops.dihedral_rows(x, list(range(8)))
    assert not torch.equal(bits(there[1:]), bits(x[1:]))
    back = ops.dihedral_rows(there, [inverse_code(k) for k in range(8)])
    assert torch.equal(bits(back), bits(x))
    into = torch.full_like(x, 3.0)
    assert ops.dihedral_rows(there, [inverse_code(k) for k in range(8)], out=into) is into and torch.equal(bits(into), bits(x))


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    lib = _lib.load()
    buf = torch.arange(8 * 64 + 8, dtype=torch.float32, device=DEV)  # in: its first 4 rows of [1, 8, 8]; the rest is room for shifted views
    src = buf[:4 * 64]
    out = torch.full((8 * 64 + 8,), -7.0, device=DEV)
    keep_src = src.clone()
    p, q = src.data_ptr(), out.data_ptr()
    many_in, many_out = torch.zeros(65536 * 4, device=DEV), torch.full((65536 * 4,), -7.0, device=DEV)  # 65536 rows of [1, 1, 4]

    def call(inp=p, outp=q, R=4, Cc=1, H=8, W=8, in_rep=1, S=4, period=4, codes=0o7531):
        return lib.idiff_dihedral_rows(C.c_void_p(inp), C.c_void_p(outp), R, Cc, H, W, in_rep, S, period, codes,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))

    n0 = ops.launch_count()
    bad = dict(
        width_6=dict(H=8, W=6, codes=0),
        transposing_nonsquare=dict(R=2, H=16, W=8, codes=0o10, period=2),
        period_0=dict(period=0),
        period_9=dict(period=9),
        rows_not_a_multiple_of_in_rep=dict(R=4, in_rep=3),
        out_is_in=dict(outp=p),
        out_overlaps_the_end_of_in=dict(outp=p + 3 * 64 * 4),
        in_overlaps_the_end_of_out=dict(inp=q + 3 * 64 * 4),
        misaligned_in=dict(inp=p + 4),
        misaligned_out=dict(outp=q + 8),
        S_0=dict(S=0),
        in_rep_0=dict(in_rep=0),
        R_0=dict(R=0),
        C_0=dict(Cc=0),
        too_many_rows=dict(inp=many_in.data_ptr(), outp=many_out.data_ptr(), R=65536, H=1, W=4, codes=0),
        null_in=dict(inp=0),
    )
    for name, kw in bad.items():
        assert call(**kw) == -1, name  # IDIFF_E_BADARG
        assert lib.idiff_last_error(), name
    torch.cuda.synchronize()
    assert ops.launch_count() == n0
    assert bool((out == -7.0).all()) and bool((many_out == -7.0).all()) and torch.equal(src, keep_src)
    # a transposing code beyond the period is not one of the call's codes
    assert call(R=2, H=16, W=8, codes=0o10, period=1, S=2) == 0
    # and the good call is taken: in_rep = 2 reads two rows and writes four
    out.fill_(-7.0)
    assert call(in_rep=2) == 0
    torch.cuda.synchronize()
    assert ops.launch_count() == n0 + 2
    got = out[:4 * 64].view(4, 1, 8, 8)
    for r, k in enumerate((1, 3, 5, 7)):
        assert torch.equal(got[r], dihedral_torch(src.view(4, 1, 8, 8)[r // 2], k)), r
    assert bool((out[4 * 64:] == -7.0).all())
    # the wrapper states the shape checks itself
    x = src.view(4, 1, 8, 8)
    with pytest.raises(ValueError):
        ops.dihedral_rows(torch.zeros(1, 1, 8, 6, device=DEV), [0])
    with pytest.raises(_lib.IdiffError):
        ops.dihedral_rows(x, [1], out=x)
    with pytest.raises(_lib.IdiffError):
        ops.dihedral_rows(x, [1], out=torch.empty(3, 1, 8, 8, device=DEV))
    assert torch.equal(src, keep_src)


# ---- 4. whole chains on the pipeline nets ---------------------------------------------------------------------------------------------
T, H, K = 20, 32, 4
B, S, SEED = 2, 5, 41


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=K))
    model.set_eval()
    return model, sde


def make_sde(built, seed=SEED, **kw):
    """an sde of its own over the model's nets"""
    model, base = built
    s = driftSDE(nets=model.get_nets(), T=T, max_sigma=base.max_sigma, eta=base.eta, drift_schedule=base.schedule_names[0],
                 noise_schedule=base.schedule_names[1], sample_T=K, **kw)
    s.set_gpu(torch.device(DEV))
    s.set_seed(seed)
    return s


def image(seed, n=1, W=None, cls=0):
    b = make_batch(n, H, W=W, seed=seed)
    names = [ARTIFACT_TYPES[(cls + i) % 5] for i in range(n)]
    return b['input'].to(DEV).contiguous(), names, b['A_emb'].to(DEV).contiguous()


def run(sde, model, img, **kw):
    cond, names, ctx = img
    mean, std, samples = sde.reverse_ddpm_ensemble(cond, names, model.text_encoder, image_context=ctx, return_samples=True, **kw)
    assert sde.last_mode == "graph" and sde.last_steps == K and torch.isfinite(samples).all()
    return mean.clone(), std.clone(), samples.clone()


def composition(plain, model, img, b, code, member, **kw):
    """member `member` on image b turned by `code`, through a one-member call of an sde without the option, turned back"""
    cond, names, ctx = img
    assert plain.self_ensemble is None
    turned = dihedral_torch(cond[b:b + 1], code)
    one = run(plain, model, (turned, names[b:b + 1], ctx[b:b + 1].contiguous()), num_samples=1, members=[member], **kw)[2]
    assert plain.last_member_ops is None
    return dihedral_torch(one[0, 0], inverse_code(code))


@pytest.fixture(scope="module")
def batch():
    return image(5, n=B)


@pytest.fixture(scope="module")
def dihedral_run(built, batch):
    """order -> (mean, std, samples) of the B x S dihedral ensemble in one chain: the reference of the chain tests, computed once"""
    model, _ = built
    out = {}
    for order in (1, 2):
        sde = make_sde(built, num_samples=S, self_ensemble="dihedral", solver_order=order)
        out[order] = run(sde, model, batch)
        assert sde.last_solver_order == order
        assert sde.last_members.tolist() == [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]]
        assert sde.last_member_ops.dtype == torch.int64 and sde.last_member_ops.tolist() == [DIHEDRAL[:S]] * B
    return out


@pytest.mark.parametrize("order", [1, 2])
def test_every_member_equals_its_composition(built, batch, dihedral_run, order):
    model, _ = built
    samples = dihedral_run[order][2]
    assert samples.shape == (B, S, 1, H, H)
    plain = make_sde(built, solver_order=order)
    for b in range(B):
        for s in range(S):
            want = composition(plain, model, batch, b, DIHEDRAL[s], 1 + b * S + s)
            assert torch.equal(samples[b, s], want), (b, s)
    assert (plain._off, plain._calls) == (0, 0)


def test_code_0_members_are_the_option_off_members_and_chunking_changes_nothing(built, batch, dihedral_run):
    model, _ = built
    mean, std, samples = dihedral_run[1]
    off = make_sde(built, num_samples=S)
    off_samples = run(off, model, batch)[2]
    assert off.last_member_ops is None and off.last_members.tolist() == [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]]
    assert torch.equal(samples[:, 0], off_samples[:, 0])
    assert not torch.equal(samples[:, 1], off_samples[:, 1])
    for mb in (2, 3):
        sde = make_sde(built, num_samples=S, self_ensemble="dihedral", max_batch=mb)
        got = run(sde, model, batch)
        for k, (a, b) in enumerate(zip(got, (mean, std, samples))):
            assert torch.equal(a, b), (mb, k)
    want = ops.ensemble_stats(samples)
    assert torch.equal(mean, want[0]) and torch.equal(std, want[1]) and float(std.mean()) > 0
    # members 0 .. 3 have the same code under both kinds
    fl = make_sde(built, num_samples=S, self_ensemble="flips")
    fl_samples = run(fl, model, batch)[2]
    assert fl.last_member_ops.tolist() == [[0, 4, 2, 6, 0]] * B
    assert torch.equal(fl_samples[:, :4], samples[:, :4]) and torch.equal(fl_samples[:, 4], off_samples[:, 4])
    assert not torch.equal(fl_samples[:, 4], samples[:, 4])


def test_option_off_or_one_member_launches_no_permutation(built, batch, monkeypatch):
    model, _ = built
    calls = []
    real = ops.dihedral_rows

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "dihedral_rows", counted)
    sde = make_sde(built, num_samples=3)
    base = run(sde, model, batch)
    assert not calls and sde.last_member_ops is None
    sde.set_self_ensemble("dihedral")
    one = run(sde, model, batch, num_samples=1, members=[1, 4])
    assert not calls and sde.last_member_ops is None  # S = 1: the option does nothing
    sde.set_self_ensemble(None)
    again = run(sde, model, batch, num_samples=1, members=[1, 4])
    assert not calls and torch.equal(one[2], again[2])
    assert torch.equal(one[2][:, 0], base[2][:, 0])
    sde.set_self_ensemble("dihedral")
    sde.set_seed(SEED)
    on = run(sde, model, batch)
    assert len(calls) == 2 and sde.last_member_ops.tolist() == [[0, 4, 2]] * B
    assert torch.equal(on[2][:, 0], base[2][:, 0]) and not torch.equal(on[2][:, 1], base[2][:, 1])
    sde.set_self_ensemble(None)
    sde.set_seed(SEED)
    off = run(sde, model, batch)
    assert len(calls) == 2 and sde.last_member_ops is None
    for a, b in zip(off, base):
        assert torch.equal(a, b)


def test_reducers_run_on_the_turned_back_samples(built, batch):
    model, _ = built
    level = 0.6
    sde = make_sde(built, num_samples=S, self_ensemble="dihedral", interval=level)
    mean, std, samples = run(sde, model, batch)
    stats = sde.last_order_stats
    idx = order_stat_indices(S, level)
    assert stats["ks"] == [idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]] and stats["level"] == level
    srt = torch.sort(samples, dim=1).values
    assert torch.equal(stats["lo"], srt[:, idx["k_lo"]]) and torch.equal(stats["hi"], srt[:, idx["k_hi"]])
    assert idx["k_m0"] == idx["k_m1"] and torch.equal(stats["median"], srt[:, idx["k_m0"]])  # S = 5: the middle member
    by_hand = driftSDE._order_stats(samples, level)
    for name in ("lo", "hi", "median"):
        assert torch.equal(stats[name], by_hand[name]), name
    target = make_batch(B, H, seed=5)['target'].to(DEV).contiguous()
    sums, counts, crps = sde.score_ensemble(samples, target, want_map=True)
    want = ops.ensemble_scores(samples, target, want_map=True)
    assert torch.equal(sums, want[0]) and torch.equal(counts, want[1]) and torch.equal(crps, want[2])
    assert int(counts[:, :S + 1].sum()) == B * H * H


# ---- 5. held graphs ---------------------------------------------------------------------------------------------------------------------
def test_reuse_graph_replays_and_keeps_the_bits(built):
    model, _ = built
    on = make_sde(built, seed=13, num_samples=3, self_ensemble="dihedral", reuse_graph=True)
    off = make_sde(built, seed=13, num_samples=3, self_ensemble="dihedral")
    outs = []
    for k, want in enumerate(("captured", "replayed")):
        img = image(40 + k, cls=k)
        a = run(on, model, img)
        assert on.last_session == want
        b = run(off, model, img)
        assert off.last_session is None
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        assert torch.equal(on.last_members, off.last_members) and torch.equal(on.last_member_ops, off.last_member_ops)
        assert on.last_member_ops.tolist() == [[0, 4, 2]]
        outs.append(a[2])
    assert len(on._sessions) == 1 and not torch.equal(outs[0], outs[1])
    on.close_sessions()


def test_flips_on_a_wide_image_through_a_held_graph(built):
    model, _ = built
    on = make_sde(built, seed=14, num_samples=3, self_ensemble="flips", reuse_graph=True)
    plain = make_sde(built, seed=14)
    for k, want in enumerate(("captured", "replayed")):
        img = image(60 + k, W=48, cls=k + 1)
        samples = run(on, model, img)[2]
        assert on.last_session == want and samples.shape == (1, 3, 1, H, 48)
        assert on.last_member_ops.tolist() == [[0, 4, 2]] and on.last_members.tolist() == [[1 + 3 * k, 2 + 3 * k, 3 + 3 * k]]
        for s in range(3):
            assert torch.equal(samples[0, s], composition(plain, model, img, 0, DIHEDRAL[s], 1 + 3 * k + s)), (k, s)
    with pytest.raises(ValueError, match="square"):
        on.set_self_ensemble("dihedral")
        run(on, model, image(62, W=48))
    on.close_sessions()


# ---- 6. tiled chains on position-dependent analytic nets ---------------------------------------------------------------------------------
_RAMPS = {}


def ramp_net(a, b, t, names, text_encoder, image_context=None):
    """pointwise, so a row's bits do not depend on the rows beside it, but not equivariant: a ramp along the window's W and a
    smaller one along its H are added, so a turned input does not give the turned output"""
    key = tuple(a.shape[-2:])
    if key not in _RAMPS:
        h, w = key
        _RAMPS[key] = (0.2 * torch.arange(w, device=a.device, dtype=torch.float32) / w
                       + 0.05 * torch.arange(h, device=a.device, dtype=torch.float32)[:, None] / h).contiguous()
    return 0.5 * a + 0.25 * b + _RAMPS[key]


def tiled_sde(**kw):
    sde = driftSDE(nets=dict(drift_net=ramp_net, noise_net=ramp_net), T=20, eta=1.0, sample_T=5, tiled_ensemble=True, tile=16, tile_overlap=4,
                   **kw)
    sde.set_gpu(torch.device(DEV))
    sde.set_seed(3)
    return sde


def test_tiled_ensemble_members_equal_their_tiled_compositions():
    g = torch.Generator().manual_seed(1)
    cond = (torch.rand(2, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    ids = [5, 2, 9, 11, 12, 13]
    codes = self_ensemble_codes("dihedral")
    assert codes == DIHEDRAL
    # two images of three members (codes 0, 4, 2), then one image of six, which reaches the transposing codes
    sde = tiled_sde(num_samples=3, self_ensemble="dihedral")
    samples = sde.reverse_ddpm_ensemble(cond, ["x", "x"], None, members=ids, return_samples=True)[2].clone()
    assert sde.last_tiles == (3, 3, 16, 16) and sde.last_mode == "graph" and sde.last_member_ops.tolist() == [[0, 4, 2]] * 2
    plain = tiled_sde()
    off = plain.reverse_ddpm_ensemble(cond, ["x", "x"], None, num_samples=3, members=ids, return_samples=True)[2]
    assert torch.equal(samples[:, 0], off[:, 0]) and not torch.equal(samples[:, 1], off[:, 1])  # the nets are not equivariant
    six = tiled_sde(num_samples=6, self_ensemble="dihedral")
    wide = six.reverse_ddpm_ensemble(cond[:1].contiguous(), ["x"], None, members=ids, return_samples=True)[2].clone()
    assert six.last_member_ops.tolist() == [DIHEDRAL[:6]] and six.last_tiles == (3, 3, 16, 16)

    def tiled_composition(b, code, member):
        turned = dihedral_torch(cond[b:b + 1], code)
        one = plain.reverse_ddpm_ensemble(turned, ["x"], None, num_samples=1, members=[member], return_samples=True)[2]
        assert plain.last_tiles == (3, 3, 16, 16)
        return dihedral_torch(one[0, 0], inverse_code(code))

    for b in range(2):
        for s in range(3):
            assert torch.equal(samples[b, s], tiled_composition(b, DIHEDRAL[s], ids[b * 3 + s])), (b, s)
    for s in range(6):
        assert torch.equal(wide[0, s], tiled_composition(0, DIHEDRAL[s], ids[s])), s
    # max_chain_rows = 27 holds three full-resolution rows of nine windows: the six rows split into two chains
    six.set_num_samples(6, max_chain_rows=27)
    again = six.reverse_ddpm_ensemble(cond[:1].contiguous(), ["x"], None, members=ids, return_samples=True)[2]
    assert torch.equal(again, wide)
    sde.set_num_samples(3, max_chain_rows=27)
    again = sde.reverse_ddpm_ensemble(cond, ["x", "x"], None, members=ids, return_samples=True)[2]
    assert torch.equal(again, samples)


# ---- 7. the model and the driver ----------------------------------------------------------------------------------------------------------
def test_pipeline_build_passes_the_option_through_and_model_test_returns_the_mean():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=8, seed=0,
                                sde_overrides=dict(num_samples=3, self_ensemble="flips", sample_T=3))
    assert sde.num_samples == 3 and sde.self_ensemble == "flips"
    model.set_eval()
    model.feed_data(make_batch(2, H, seed=2))
    model.test(return_samples=True)
    assert sde.last_member_ops.tolist() == [[0, 4, 2]] * 2
    assert model.samples.shape == (2, 3, 1, H, H) and torch.isfinite(model.samples).all()
    mean, std = ops.ensemble_stats(model.samples)
    assert torch.equal(model.output, mean) and torch.equal(model.output_std, std)
    assert float((model.output.double() - model.samples.double().mean(dim=1)).abs().max()) < 2e-6


def test_testum_self_ensemble_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_self").replace("image_size: 64", "image_size: 32").replace("T: 100", "T: 8")
    txt = txt.replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "1", "--num-samples", "2", "--sample-T", "3"]
    res = testUM.main(common + ["--self-ensemble", "dihedral"])
    out = capsys.readouterr().out.strip().splitlines()[-1]
    assert "2 samples per image" in out and "self-ensemble dihedral" in out, out
    done = [v for v in res.values() if v['num']]
    assert sum(v['num'] for v in done) == 1 and all(s > 0 for v in done for s in v['STD'])
    testUM.main(common)
    assert "self-ensemble" not in capsys.readouterr().out
