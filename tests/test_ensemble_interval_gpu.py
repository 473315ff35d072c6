"""Credible intervals of posterior ensembles on the device: the per-pixel order statistics against a sort on the host (selection rounds
nothing, so every comparison is torch.equal), the two kernel forms against each other bit for bit, the NaN and infinity rules, the
grid-stride loop, the refusals, the integer coverage counts, and the driftSDE / model / testUM surface."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import order_stat_indices  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
AUTO, NETWORK, RANK = ops.ORDER_AUTO, ops.ORDER_NETWORK, ops.ORDER_RANK
S_NET = [1, 2, 3, 4, 5, 8, 9, 16]
S_ALL = S_NET + [17, 33]
SHAPES = [(1, 12, 20), (1, 32, 32)]  # 60 float4 groups (less than a block) and 256
KINDS = ["normal", "ties"]


@functools.lru_cache(maxsize=None)
def case(S, shape, kind):
    """(x [2, S, *shape] on the host, its sort over the members): computed once and shared, never modified"""
    g = torch.Generator().manual_seed(1000 * S + shape[1] + (7 if kind == "ties" else 0))
    x = torch.randn((2, S) + shape, generator=g)
    if kind == "ties":  # 8 levels -4/2 .. 3/2: ties in every pixel from S = 9 on, and many below; + 0.0 turns the -0.0 of round() into +0.0
        x = (torch.round(x * 2).clamp(-4, 3) / 2 + 0.0).contiguous()
        assert x.unique().numel() == 8
    return x, torch.sort(x, dim=1).values


def k_lists(S):
    """every k of range(S) in chunks of 8, then one reversed list and one with duplicates"""
    ks = list(range(S))
    lists = [ks[i:i + 8] for i in range(0, S, 8)]
    lists.append(ks[::-1][:8])
    lists.append([S - 1, 0, S // 2, 0, S - 1, S // 2, S // 2][:8])
    return lists


def check_against_sort(S, algo):
    for shape in SHAPES:
        for kind in KINDS:
            x, srt = case(S, shape, kind)
            xd = x.to(DEV)
            for ks in k_lists(S):
                got = ops.ensemble_order_stats(xd, ks, algo=algo)
                assert got.shape == (2, len(ks)) + shape
                assert torch.equal(got.cpu(), srt[:, ks]), (S, algo, shape, kind, ks)


# ---- 1. selection against the host sort -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_NET)
def test_network_form_against_the_host_sort(S):
    check_against_sort(S, NETWORK)


@pytest.mark.parametrize("S", S_ALL)
def test_rank_form_against_the_host_sort(S):
    check_against_sort(S, RANK)


@pytest.mark.parametrize("S", S_ALL)
def test_auto_form_against_the_host_sort(S):
    check_against_sort(S, AUTO)


@pytest.mark.parametrize("S", S_NET)
def test_the_two_forms_agree_bit_for_bit(S):
    for shape in SHAPES:
        for kind in KINDS:
            xd = case(S, shape, kind)[0].to(DEV)
            for ks in k_lists(S):
                a = ops.ensemble_order_stats(xd, ks, algo=NETWORK)
                b = ops.ensemble_order_stats(xd, ks, algo=RANK)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (S, shape, kind, ks)


def test_the_result_of_an_image_does_not_depend_on_the_batch():
    x = case(5, SHAPES[1], "normal")[0].to(DEV)
    both = ops.ensemble_order_stats(x, [0, 2, 4])
    for b in range(2):
        assert torch.equal(ops.ensemble_order_stats(x[b:b + 1].contiguous(), [0, 2, 4])[0], both[b])


# ---- 2. NaN, infinities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [NETWORK, RANK])
@pytest.mark.parametrize("S", [1, 3, 8, 16])
def test_one_nan_poisons_its_pixel_and_no_other(S, algo):
    x, srt = case(S, SHAPES[0], "normal")
    x = x.clone()
    member, at = S // 2, (1, 0, 7, 13)  # image 1, pixel (7, 13)
    x[at[0], member, at[1], at[2], at[3]] = float("nan")
    ks = list(range(S))[:8]
    got = ops.ensemble_order_stats(x.to(DEV), ks, algo=algo).cpu()
    assert torch.isnan(got[at[0], :, at[1], at[2], at[3]]).all()  # every plane
    want = srt[:, ks].clone()
    want[at[0], :, at[1], at[2], at[3]] = 0.0
    got[at[0], :, at[1], at[2], at[3]] = 0.0
    assert torch.equal(got, want)  # every other pixel is the sort of the unpoisoned input


@pytest.mark.parametrize("algo", [NETWORK, RANK])
@pytest.mark.parametrize("S", [3, 5, 16])
def test_infinities_sort_as_values(S, algo):
    x = case(S, SHAPES[0], "normal")[0].clone()
    x[0, 0, 0, 0, :] = float("inf")
    x[0, S - 1, 0, 1, :] = float("-inf")
    x[1, :, 0, 2, :4] = float("inf")      # every member +inf: the network's padding and the values are the same number
    x[1, :2, 0, 3, :] = float("-inf")     # ties at -inf
    x[1, 2, 0, 3, :] = float("inf")
    srt = torch.sort(x, dim=1).values
    ks = list(range(S))[-8:]
    got = ops.ensemble_order_stats(x.to(DEV), ks, algo=algo).cpu()
    assert torch.equal(got, srt[:, ks])
    assert not torch.isnan(got).any()


# ---- 3. the grid-stride loop -------------------------------------------------------------------------------------------------------
def test_more_groups_than_the_grid_covers_in_one_pass():
    """Q = 2048 * 256 + 3 float4 groups per image: the grid's 2048 blocks of 256 threads cover 2048 * 256, so three groups are reached
    only by a thread's second trip through the loop"""
    Q, S = 2048 * 256 + 3, 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, S, 4 * Q), generator=g)
    want = torch.sort(x, dim=1).values
    xd = x.to(DEV)
    for algo in (NETWORK, RANK):
        got = ops.ensemble_order_stats(xd, [2, 0, 1], algo=algo).cpu()
        assert torch.equal(got, want[:, [2, 0, 1]]), algo
        assert torch.equal(got[0, :, -12:], want[0, [2, 0, 1], -12:])


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched():
    lib = _lib.load()
    x = torch.randn(2, 4, 1, 8, 8, device=DEV)
    sentinel = 7.0

    def fresh(nk):
        return torch.full((2, nk, 1, 8, 8), sentinel, device=DEV)

    def refused(call, out):
        n0 = ops.launch_count()
        with pytest.raises(_lib.IdiffError):
            call(out)
        torch.cuda.synchronize()
        assert ops.launch_count() == n0, "a kernel was launched before the argument check"
        assert bool((out == sentinel).all())

    refused(lambda o: ops.ensemble_order_stats(x, [0, 4], out=o), fresh(2))          # k = S
    refused(lambda o: ops.ensemble_order_stats(x, [-1], out=o), fresh(1))            # k < 0
    refused(lambda o: ops.ensemble_order_stats(x, [0] * 9, out=o), fresh(9))         # nk = 9
    ks0 = (ops.C.c_int32 * 1)(0)
    refused(lambda o: _lib.check(lib.idiff_ensemble_order_stats(x.data_ptr(), o.data_ptr(), 2, 4, 64, ks0, 0, 0, None)), fresh(1))  # nk = 0
    x17 = torch.randn(1, 17, 1, 8, 8, device=DEV)
    o17 = torch.full((1, 1, 1, 8, 8), sentinel, device=DEV)
    refused(lambda o: ops.ensemble_order_stats(x17, [0], algo=NETWORK, out=o), o17)  # the network form holds 16 members
    assert torch.equal(ops.ensemble_order_stats(x17, [0], algo=AUTO, out=o17), x17.min(dim=1, keepdim=True).values)  # auto takes the rank form
    x25 = torch.randn(1, 2, 1, 5, 5, device=DEV)
    refused(lambda o: ops.ensemble_order_stats(x25, [0], out=o), torch.full((1, 1, 1, 5, 5), sentinel, device=DEV))  # n_s % 4 != 0
    keep = x.clone()
    n0 = ops.launch_count()
    with pytest.raises(_lib.IdiffError):  # out aliasing x
        ops.ensemble_order_stats(x, [0, 1, 2, 3], out=x)
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_order_stats(x, [0], algo=3)
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_order_stats(x, [0.0])
    assert ops.launch_count() == n0 and torch.equal(x, keep)


# ---- 5. interval_coverage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 12, 20), (1, 64, 64)])
def test_interval_coverage_against_integer_counts(shape):
    B = 3
    g = torch.Generator().manual_seed(shape[1])
    a, b = torch.randn((B,) + shape, generator=g), torch.randn((B,) + shape, generator=g)
    lo, hi = torch.minimum(a, b) - 0.2, torch.maximum(a, b) + 0.2
    t = torch.randn((B,) + shape, generator=g)
    t[0, 0, 0, :] = lo[0, 0, 0, :]           # exactly on lo: inside
    t[0, 0, 1, :] = hi[0, 0, 1, :]           # exactly on hi: inside
    lo[1, 0, 2, :], hi[1, 0, 2, :] = hi[1, 0, 2, :].clone(), lo[1, 0, 2, :].clone()  # lo > hi: nothing inside there
    t[1, 0, 2, :5] = 0.5 * (lo[1, 0, 2, :5] + hi[1, 0, 2, :5])                      # not even a target between the two
    t[2, 0, 3, 4] = float("nan")             # a NaN target counts nowhere
    lo[2, 0, 5, 6] = float("nan")            # nor does a pixel whose bound is NaN
    hi[2, 0, 5, 7] = float("nan")
    ok = ~(torch.isnan(lo) | torch.isnan(hi) | torch.isnan(t))
    want = torch.stack([((t < lo) & ok).flatten(1).sum(1), ((t >= lo) & (t <= hi) & ok).flatten(1).sum(1), ((t > hi) & ok).flatten(1).sum(1)],
                       dim=1).to(torch.int32)
    got = ops.interval_coverage(lo.to(DEV), hi.to(DEV), t.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (B, 3)
    print(f"{shape}: counts {got.cpu().tolist()}, host {want.tolist()}")
    assert torch.equal(got.cpu(), want)
    n = shape[1] * shape[2]
    assert int(want[0].sum()) == n and int(want[2].sum()) == n - 3   # three NaN pixels of image 2 are counted nowhere
    assert int(want[1].sum()) > n                                    # where lo > hi a target may be below lo AND above hi, never inside
    swapped = ((t[1, 0, 2] >= lo[1, 0, 2]) & (t[1, 0, 2] <= hi[1, 0, 2])).sum()
    assert int(swapped) == 0
    again = ops.interval_coverage(lo.to(DEV), hi.to(DEV), t.to(DEV))
    assert torch.equal(again, got)


def test_interval_coverage_refusals():
    z = torch.zeros(1, 1, 5, 5, device=DEV)
    with pytest.raises(_lib.IdiffError):
        ops.interval_coverage(z, z, z)  # n_s % 4 != 0
    with pytest.raises(AssertionError):
        ops.interval_coverage(torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 4, device=DEV))


# ---- 6. whole chains ---------------------------------------------------------------------------------------------------------------
T, H = 6, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0)
    model.set_eval()
    return model, sde


@pytest.mark.parametrize("S", [5, 4])
def test_chain_order_stats_equal_the_host_sort_of_the_samples(built, S):
    model, sde = built
    B, L = 2, 0.8
    batch = make_batch(B, H, seed=5)
    cond, ctx = batch['input'].to(DEV).contiguous(), batch['A_emb'].to(DEV).contiguous()

    def run(level):
        sde.set_seed(41)
        sde.set_num_samples(S)
        sde.set_interval(level)
        n0 = ops.launch_count()
        mean, std, samples = sde.reverse_ddpm_ensemble(cond, batch['names'], model.text_encoder, image_context=ctx, return_samples=True)
        torch.cuda.synchronize()
        return (mean.clone(), std.clone(), samples.clone()), ops.launch_count() - n0, sde.last_order_stats

    try:
        run(None)  # fills the weight and text caches, whose launches belong to no later call
        plain, n_plain, stats = run(None)
        assert stats is None
        with_l, n_with, stats = run(L)
        again, n_again, none_again = run(None)
    finally:
        sde.set_interval(None)
        sde.set_num_samples(None)
    assert none_again is None and n_again == n_plain                      # unset: the launches of a call without the option
    # set: ONE selection launch; at B = 2 a plane is strided over the batch, so each map is copied out by one gather_channel launch
    # (lo, hi, m0 -- and m1 for an even S, whose median takes one axpby more)
    assert n_with == n_plain + (1 + 3 if S % 2 else 1 + 4 + 1)
    for a, b, c in zip(plain, with_l, again):                             # mean, std and samples do not know about the option
        assert torch.equal(a, b) and torch.equal(a, c)
    idx = order_stat_indices(S, L)
    assert stats["ks"] == [idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]] and stats["level"] == L and stats["nominal"] == idx["nominal"]
    assert (idx["k_lo"], idx["k_hi"]) == (0, S - 1)  # floor(0.1 * (S - 1)) = 0 for S = 4, 5
    for m in (stats["lo"], stats["hi"], stats["median"]):                 # contiguous maps: the library's own ops take them as they are
        assert m.is_contiguous()
    target = batch['target'].to(DEV).contiguous()
    counts = ops.interval_coverage(stats["lo"], stats["hi"], target).cpu()
    inside = ((target >= stats["lo"]) & (target <= stats["hi"])).flatten(1).sum(1).cpu()
    assert counts[:, 1].tolist() == inside.tolist() and bool((counts.sum(1) == H * H).all())
    samples = with_l[2].cpu()
    srt = torch.sort(samples, dim=1).values
    lo, hi, med = stats["lo"].cpu(), stats["hi"].cpu(), stats["median"].cpu()
    assert lo.shape == hi.shape == med.shape == (B, 1, H, H)
    assert torch.equal(lo, srt[:, idx["k_lo"]]) and torch.equal(hi, srt[:, idx["k_hi"]])
    if S % 2:
        assert torch.equal(med, srt[:, idx["k_m0"]])
    else:
        assert torch.equal(med, 0.5 * srt[:, idx["k_m0"]] + 0.5 * srt[:, idx["k_m1"]])  # fp32: exact products, one rounded add
    assert bool((lo <= med).all()) and bool((med <= hi).all())
    assert float((hi - lo).mean()) > 0


def test_model_test_sets_the_interval_maps(built):
    model, sde = built
    batch = make_batch(2, H, seed=9)
    try:
        sde.set_num_samples(3)
        sde.set_interval(0.5)
        model.feed_data(batch)
        model.test(return_samples=True)
        for t in (model.output_median, model.output_lo, model.output_hi):
            assert torch.is_tensor(t) and t.shape == model.output.shape and torch.isfinite(t).all()
        srt = torch.sort(model.samples, dim=1).values
        assert torch.equal(model.output_lo, srt[:, 0]) and torch.equal(model.output_median, srt[:, 1]) and torch.equal(model.output_hi, srt[:, 2])
        mean, _ = ops.ensemble_stats(model.samples)
        assert torch.equal(model.output, mean)  # output stays the mean
        sde.set_interval(None)
        model.test()
        assert model.output_median is None and model.output_lo is None and model.output_hi is None and model.output_std is not None
        sde.set_interval(0.5)
        sde.set_num_samples(None)  # the plain chain: the option does nothing
        model.test()
        assert model.output_median is None and model.output_lo is None and model.output_hi is None and model.output_std is None
    finally:
        sde.set_interval(None)
        sde.set_num_samples(None)


def test_pipeline_build_passes_interval_through():
    _, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(num_samples=2, interval=0.9))
    assert sde.interval == 0.9 and sde.num_samples == 2


NEW_WORDS = ("PSNR_median", "COVER", "WIDTH", "interval", "nominal", "_lo_", "_hi_", "_median_")


def test_testum_interval_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_int").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "1", "--num-samples", "4", "--sample-T", "3"]
    res = testUM.main(common + ["--interval", "0.9"])
    out = capsys.readouterr().out
    assert out.rstrip().splitlines()[-1].endswith("interval 0.9 (nominal 0.6)"), out[-500:]
    (name, v), = [(k, v) for k, v in res.items() if v['num']]
    assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD', 'PSNR_median', 'COVER', 'WIDTH'}
    assert len(v['COVER']) == len(v['WIDTH']) == len(v['PSNR_median']) == 1
    assert 0.0 <= v['COVER'][0] <= 1.0 and v['WIDTH'][0] > 0 and np.isfinite(v['PSNR_median'][0])
    for word in ("PSNR_median=", "COVER=", "WIDTH=", "AVG PSNR_median", "AVG COVER", "AVG WIDTH"):
        assert word in out, word
    folder = tmp_path / "results" / "drv_int" / name
    files = sorted(os.listdir(folder))
    maps = {}
    for tag in ("lo", "hi", "median", "std"):
        (f,) = [f for f in files if f"_{tag}_" in f]
        assert f.endswith(f"_{tag}_64x64x1.raw"), f
        maps[tag] = np.fromfile(folder / f, dtype=np.float32)
        assert maps[tag].size == 64 * 64
    assert (maps["lo"] <= maps["median"]).all() and (maps["median"] <= maps["hi"]).all()
    assert v['WIDTH'][0] == pytest.approx(float((maps["hi"].astype(np.float64) - maps["lo"]).mean()), rel=1e-5)
    # without --interval the driver prints and writes what it did before
    txt2 = txt.replace("name: drv_int", "name: drv_plain")
    cfg.write_text(txt2)
    res = testUM.main(common)
    out = capsys.readouterr().out
    printed = out.replace(str(tmp_path), "")
    for word in NEW_WORDS:
        assert word not in printed, word
    (name, v), = [(k, v) for k, v in res.items() if v['num']]
    assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD'}
    files = os.listdir(tmp_path / "results" / "drv_plain" / name)
    assert len(files) == 2 and not any(w in f for f in files for w in ("_lo_", "_hi_", "_median_"))
