"""Ensemble scores on the device (idiff_ensemble_scores through the C ABI and ops.ensemble_scores): the CRPS map bit for bit against the
float32 emulation of the contract (tests/ensemble_scores_ref.py), the rank histogram exactly, the fp64 sums within the bound of an fp64 sum,
independence of the batch and of the run, ties, NaN, the refusals, the interval path's coverage count, and the driftSDE / model / testUM
surface."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ensemble_scores_ref import draw, emulate, image_record  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import ensemble_score_summary, order_stat_indices  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
# one float4 group; one group past a 256-thread block; one group past one sweep of the 64 x 256-thread grid of an image
N_S = [4, 1028, 64 * 1024 + 4]
S_ALL = [1, 2, 3, 16, 17, 33]  # the register / second-read boundary and a chunk remainder
B_MAX = 3


@functools.lru_cache(maxsize=None)
def case(S, n_s):
    """(x [3, S, n_s], y [3, n_s] float32 on the host, the emulation of each image): computed once and shared, never modified"""
    pairs = [draw(S, n_s, seed=7919 * S + n_s + b) for b in range(B_MAX)]
    x, y = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return torch.from_numpy(x), torch.from_numpy(y), [emulate(x[b], y[b]) for b in range(B_MAX)]


def bits(t):
    return t.contiguous().view(torch.int32)


def check_image(S, n_s, em, sums, counts, crps_map, what):
    """one image's device results against its emulation"""
    ok = em["valid"]
    want_sums, want_counts = image_record(em, S)
    assert counts.tolist() == want_counts.tolist(), what
    if crps_map is not None:
        got = crps_map.numpy()
        assert np.array_equal(got[ok].view(np.int32), em["crps"][ok].view(np.int32)), what  # bit for bit
        assert np.isnan(got[~ok]).all(), what
    # an fp64 sum of n terms, whatever its order, is off by at most (n - 1) 2^-53 sum |term|; a factor 2 as the only margin
    for q, name in enumerate(("crps", "e", "v")):
        bound = 2 * n_s * 2.0 ** -53 * float(np.abs(em[name][ok].astype(np.float64)).sum())
        err = abs(float(sums[q]) - float(want_sums[q]))
        print(f"{what} sum {name}: {float(sums[q])!r}, host {float(want_sums[q])!r}, |diff| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, name)


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_scores_against_the_emulation(S, n_s):
    """B = 3 and B = 1 on the same data: map, histogram and sums of every image against the emulation, and image 0 of the batch bit for
    bit what it is alone.  At n_s = 4 one thread of one block has work: the other 63 partial blocks of the image contribute zeros."""
    x, y, ems = case(S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    sums3, counts3, map3 = ops.ensemble_scores(xd, yd, want_map=True)
    assert sums3.dtype == torch.float64 and sums3.shape == (3, 3) and sums3.is_cuda
    assert counts3.dtype == torch.int32 and counts3.shape == (3, S + 2) and counts3.is_cuda
    assert map3.dtype == torch.float32 and map3.shape == (3, n_s)
    for b in range(B_MAX):
        check_image(S, n_s, ems[b], sums3[b].cpu(), counts3[b].cpu(), map3[b].cpu(), f"B=3 S={S} n_s={n_s} image {b}")
        assert int(counts3[b, :S + 1].sum()) == n_s and int(counts3[b, S + 1]) == 0
    sums1, counts1, map1 = ops.ensemble_scores(xd[:1].contiguous(), yd[:1].contiguous(), want_map=True)
    check_image(S, n_s, ems[0], sums1[0].cpu(), counts1[0].cpu(), map1[0].cpu(), f"B=1 S={S} n_s={n_s}")
    assert torch.equal(sums1[0].view(torch.int64), sums3[0].view(torch.int64))
    assert torch.equal(counts1[0], counts3[0]) and torch.equal(bits(map1[0]), bits(map3[0]))


@pytest.mark.parametrize("S", [2, 16, 17])
def test_scores_do_not_depend_on_the_batch_the_run_or_the_map(S):
    n_s = 64 * 1024 + 4
    x, y, _ = case(S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    sums, counts, crps = ops.ensemble_scores(xd, yd, want_map=True)
    again = ops.ensemble_scores(xd, yd, want_map=True)
    assert torch.equal(sums.view(torch.int64), again[0].view(torch.int64)) and torch.equal(counts, again[1]) and torch.equal(bits(crps), bits(again[2]))
    bare = ops.ensemble_scores(xd, yd)  # want_map=False: the same sums and counts, no map
    assert bare[2] is None and torch.equal(sums.view(torch.int64), bare[0].view(torch.int64)) and torch.equal(counts, bare[1])
    for b in range(B_MAX):
        s1, c1, m1 = ops.ensemble_scores(xd[b:b + 1].contiguous(), yd[b:b + 1].contiguous(), want_map=True)
        assert torch.equal(s1[0].view(torch.int64), sums[b].view(torch.int64)) and torch.equal(c1[0], counts[b]) and torch.equal(bits(m1[0]), bits(crps[b]))


@pytest.mark.parametrize("S", [1, 5, 12, 16])
def test_register_and_second_read_forms_agree(S, monkeypatch):
    x, y, _ = case(S, 1028)
    xd, yd = x.to(DEV), y.to(DEV)
    monkeypatch.delenv("IDIFF_ENSEMBLE_REREAD", raising=False)
    reg = ops.ensemble_scores(xd, yd, want_map=True)
    monkeypatch.setenv("IDIFF_ENSEMBLE_REREAD", "1")
    rr = ops.ensemble_scores(xd, yd, want_map=True)
    assert torch.equal(reg[0].view(torch.int64), rr[0].view(torch.int64)) and torch.equal(reg[1], rr[1]) and torch.equal(bits(reg[2]), bits(rr[2]))


# ---- 2. ties, NaN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 9, 16, 17])
def test_ties(S):
    """members and truth on 8 levels: ties among the members in every pixel from S = 9 on, and members on the truth in many.  A member
    equal to the truth is not below it; equal members take consecutive ranks in index order (the emulation's rule, checked on the host)."""
    n_s = 1028
    rng = np.random.default_rng(S)
    x = (np.clip(np.round(rng.normal(0, 1, (1, S, n_s)) * 2), -4, 3) / 2 + 0.0).astype(np.float32)
    y = (np.clip(np.round(rng.normal(0, 1, (1, n_s)) * 2), -4, 3) / 2 + 0.0).astype(np.float32)
    em = emulate(x[0], y[0])
    # the data has what the test is about: with 8 levels a member sits on the truth with probability about 0.16, so in 1 - 0.84^2 = 0.29
    # of the pixels at S = 2 and in nearly all from S = 9 on
    assert (x[0] == y[0][None]).any(axis=0).mean() > 0.2 and np.array_equal(em["k"], (x[0] < y[0][None]).sum(axis=0))
    assert np.array_equal(np.sort(em["ranks"], axis=0), np.arange(S)[:, None].repeat(n_s, axis=1))
    sums, counts, crps = ops.ensemble_scores(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), want_map=True)
    check_image(S, n_s, em, sums[0].cpu(), counts[0].cpu(), crps[0].cpu(), f"ties S={S}")


@pytest.mark.parametrize("S", [3, 16, 17])
def test_nan_pixels_are_invalid_and_touch_no_other(S):
    n_s = 1028
    x, y, ems = case(S, n_s)
    x, y = x[:2].clone(), y[:2].clone()
    x[0, S // 2, 5] = float("nan")      # a NaN member
    x[0, 0, 1027] = float("nan")
    y[0, 300] = float("nan")            # a NaN target
    y[1, 7] = float("nan")
    x[1, S - 1, 7] = float("nan")       # both in one pixel: counted once
    bad = {0: [5, 300, 1027], 1: [7]}
    sums, counts, crps = ops.ensemble_scores(x.to(DEV), y.to(DEV), want_map=True)
    for b in range(2):
        em = emulate(x[b].numpy(), y[b].numpy())
        assert np.nonzero(~em["valid"])[0].tolist() == bad[b]
        assert int(counts[b, S + 1]) == len(bad[b]) and int(counts[b, :S + 1].sum()) == n_s - len(bad[b])
        check_image(S, n_s, em, sums[b].cpu(), counts[b].cpu(), crps[b].cpu(), f"nan S={S} image {b}")
        got, clean = crps[b].cpu().numpy(), ems[b]["crps"]
        keep = np.ones(n_s, dtype=bool)
        keep[bad[b]] = False
        assert np.array_equal(got[keep].view(np.int32), clean[keep].view(np.int32))  # every other pixel is the unpoisoned input's
        assert torch.isfinite(sums[b]).all()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, S, n_s = 2, 4, 64
    x = torch.randn(B, S, n_s + 4, device=DEV)[:, :, :n_s].contiguous()
    y = torch.randn(B, n_s, device=DEV)
    x0, y0 = x.clone(), y.clone()
    big = torch.randn(1, 1025, 4, device=DEV)
    canary = dict(map=torch.full((B, n_s), 7.0, device=DEV), sums=torch.full((B, 3), 7.0, device=DEV, dtype=torch.float64),
                  counts=torch.full((B, 1025 + 2), 7, device=DEV, dtype=torch.int32),
                  ws=torch.full((int(lib.idiff_ensemble_scores_ws_bytes(B, 1024)) // 8,), 7.0, device=DEV, dtype=torch.float64))

    def call(xp, yp, mp, B_, S_, n):
        return lib.idiff_ensemble_scores(xp, yp, mp, canary["sums"].data_ptr(), canary["counts"].data_ptr(), canary["ws"].data_ptr(), B_, S_, n, None)

    xp, yp, mp = x.data_ptr(), y.data_ptr(), canary["map"].data_ptr()
    refused = {
        "n_s % 4": lambda: call(xp, yp, mp, B, S, n_s - 2),
        "misaligned x": lambda: call(xp + 4, yp, mp, B, S, n_s - 4),
        "misaligned target": lambda: call(xp, yp + 8, mp, B, S, n_s - 4),
        "misaligned map": lambda: call(xp, yp, mp + 4, B, S, n_s - 4),
        "S = 0": lambda: call(xp, yp, mp, B, 0, n_s),
        "S = 1025": lambda: call(big.data_ptr(), yp, mp, 1, 1025, 4),
        "crps_map == x": lambda: call(xp, yp, xp, B, S, n_s),
        "crps_map == target": lambda: call(xp, yp, yp, B, S, n_s),
        "B = 0": lambda: call(xp, yp, mp, 0, S, n_s),
        "B = 65536": lambda: call(xp, yp, mp, 65536, S, 4),
        "no target": lambda: call(xp, None, mp, B, S, n_s),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert "ensemble_scores" in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert torch.equal(x, x0) and torch.equal(y, y0), what
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_scores(torch.zeros(1, 2, 1, 5, 5, device=DEV), torch.zeros(1, 1, 5, 5, device=DEV))  # n_s % 4 through the wrapper
    with pytest.raises(AssertionError):
        ops.ensemble_scores(torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 4, device=DEV))
    assert call(xp, yp, mp, B, S, n_s) == 0  # and the same buffers are accepted as they stand
    torch.cuda.synchronize()
    assert int(canary["counts"].view(-1)[:B * (S + 2)].view(B, S + 2)[:, :S + 1].sum()) == B * n_s


# ---- 4. the interval path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,level", [(8, 0.5), (17, 0.8)])
def test_histogram_agrees_with_the_interval_coverage(S, level):
    """tie-free data: the truth lies inside [x_(k_lo), x_(k_hi)] exactly when k_lo < k <= k_hi members are below it, so the `inside` count
    of interval_coverage over ensemble_order_stats' lo / hi planes is the histogram's sum over those bins"""
    n_s = 4096
    g = torch.Generator().manual_seed(S)
    x = torch.randn((1, S, n_s), generator=g)
    y = torch.randn((1, n_s), generator=g)
    assert not (x == y[:, None]).any() and all(x[0, :, i].unique().numel() == S for i in range(0, n_s, 97))
    idx = order_stat_indices(S, level)
    xd, yd = x.to(DEV), y.to(DEV)
    planes = ops.ensemble_order_stats(xd, [idx["k_lo"], idx["k_hi"]])
    inside = int(ops.interval_coverage(planes[:, 0].contiguous(), planes[:, 1].contiguous(), yd)[0, 1])
    _, counts, _ = ops.ensemble_scores(xd, yd)
    hist = counts[0, :S + 1].cpu().tolist()
    assert idx["k_lo"] >= 1 and inside == sum(hist[idx["k_lo"] + 1:idx["k_hi"] + 1]) and 0 < inside < n_s
    assert hist == np.bincount((x[0] < y).sum(dim=0).numpy(), minlength=S + 1).tolist()


# ---- 5. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, H = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=4, num_samples=4))
    model.set_eval()
    return model, sde


def test_model_score_ensemble(built):
    model, sde = built
    model.feed_data(make_batch(2, H, seed=3))
    model.test(return_samples=True)
    assert model.samples.shape == (2, 4, 1, H, H)
    n0 = ops.launch_count()
    sums, counts, crps = model.score_ensemble()
    assert ops.launch_count() == n0 + 2 and crps is None  # the two launches of ops.ensemble_scores and nothing else
    want = ops.ensemble_scores(model.samples, model.target, want_map=True)
    assert torch.equal(sums.view(torch.int64), want[0].view(torch.int64)) and torch.equal(counts, want[1])
    with_map = model.score_ensemble(want_map=True)
    assert torch.equal(bits(with_map[2]), bits(want[2])) and with_map[2].shape == model.target.shape
    direct = sde.score_ensemble(model.samples, model.target)
    assert torch.equal(direct[0].view(torch.int64), sums.view(torch.int64)) and torch.equal(direct[1], counts)
    em = emulate(model.samples[0].flatten(1).cpu().numpy(), model.target[0].flatten().cpu().numpy())
    check_image(4, H * H, em, sums[0].cpu(), counts[0].cpu(), with_map[2][0].flatten().cpu(), "model image 0")
    record = ensemble_score_summary(sums, counts, 4)
    assert record["N"] == 2 * H * H and record["invalid"] == 0 and record["CRPS"] > 0 and np.isfinite(record["SSR"])
    model.test()  # the members are not kept: nothing to score
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.score_ensemble()
    with pytest.raises(ValueError):
        sde.score_ensemble(model.output, model.target)


NEW_WORDS = ("CRPS", "SSR", "RANK_DEV", "OUTLIERS", "_crps_", "rank_hist", "pooled")


def test_testum_scores_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {H}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_scores").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "2", "--num-samples", "4", "--sample-T", "4"]
    res = testUM.main(common + ["--scores"])
    out = capsys.readouterr().out
    for word in ("CRPS=", "SSR=", "RANK_DEV=", "AVG CRPS", "pooled over", "SSR: ", "RANK_DEV: ", "OUTLIERS: ", "(nominal 0.4)"):
        assert word in out, word
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2
    for name, v in done.items():
        assert len(v['CRPS']) == len(v['SSR']) == len(v['RANK_DEV']) == v['num']
        assert all(c > 0 and np.isfinite(c) for c in v['CRPS']) and all(0.0 <= d <= 2.0 for d in v['RANK_DEV'])
        folder = tmp_path / "results" / "drv_scores" / name
        maps = sorted(f for f in os.listdir(folder) if "_crps_" in f)
        assert len(maps) == v['num'] and all(f.endswith(f"_crps_{H}x{H}x1.raw") for f in maps)
        for f, c in zip(maps, v['CRPS']):  # the map is on the printed scale: its mean is the image's CRPS
            m = np.fromfile(folder / f, dtype=np.float32)
            assert m.size == H * H and (m >= 0).all()
        assert sorted(float(np.fromfile(folder / f, dtype=np.float32).astype(np.float64).mean()) for f in maps) == \
            pytest.approx(sorted(v['CRPS']), rel=1e-6)
        hist = json.load(open(folder / "rank_hist.json"))
        assert hist["S"] == 4 and len(hist["hist"]) == 5 and sum(hist["hist"]) == hist["N"] == v['num'] * H * H
        assert hist["nominal"] == 0.2 and hist["hist"] == v['pooled']['hist']
    # without --scores the driver prints and writes what it did before
    cfg.write_text(txt.replace("name: drv_scores", "name: drv_plain"))
    n0 = ops.launch_count()
    res = testUM.main(common)
    n_plain = ops.launch_count() - n0
    printed = capsys.readouterr().out.replace(str(tmp_path), "")
    for word in NEW_WORDS:
        assert word not in printed, word
    for name, v in res.items():
        if v['num']:
            assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD'}
            files = os.listdir(tmp_path / "results" / "drv_plain" / name)
            assert len(files) == 2 * v['num'] and not any("_crps_" in f or "rank_hist" in f for f in files)
    cfg.write_text(txt.replace("name: drv_scores", "name: drv_scores2"))
    n0 = ops.launch_count()
    testUM.main(common + ["--scores"])
    capsys.readouterr()
    assert ops.launch_count() - n0 == n_plain + 2 * 2  # two images, the two launches of the scores each: nothing else differs


def test_testum_scores_needs_an_ensemble(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--scores"])
    assert "num_samples > 1" in capsys.readouterr().err
    assert not (tmp_path / "results").exists()  # before any image ran
