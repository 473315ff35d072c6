"""Radial power spectra on the device: idiff_radial_power_spectrum against np.fft.rfft2 under a derived and a measured tolerance
(tests/spectrum_ref.py), Parseval, a pure cosine, the spread decomposition through driftSDE.power_spectra, bit-independence of the row
count, the chunking and the run, non-finite rows, a hostile bin table, the refusals, and the model / testUM surface."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import spectrum_ref as sr
import torch

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import spectrum_summary  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
QNAN64 = 0x7ff8000000000000


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def bits64(t):
    return t.contiguous().view(torch.int64)


def run(x, sub=None, sub_rep=1, **kw):
    return ops.radial_power_spectrum(dev(x), dev(sub), sub_rep, **kw)


def sumsq(x, sub=None, sub_rep=1):
    a = sr.row_images(x, sub, sub_rep)
    return (a * a).sum(axis=(1, 2))


# ---- 1. against np.fft.rfft2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["white", "dc"])
@pytest.mark.parametrize("shape, mode", sr.all_cases())
def test_against_the_reference(shape, mode, kind):
    """the derived bound on every input; on white noise, where every bin holds comparable power, also the relative error per bin within
    64 x the emulation's own (measured on the CPU on these inputs, not taken from the kernel); Parseval per row"""
    x, sub, rep = sr.case(shape, mode, kind)
    got = run(x, sub, rep)
    H, W = shape
    counts = ops.radial_bins(H, W)[1]
    assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0], counts.numel())
    got, ref, ss = got.cpu().numpy(), sr.case_reference(shape, mode, kind), sumsq(x, sub, rep)
    err = np.abs(got - ref)
    bound = sr.derived_bound(H, W, counts.numpy(), ss)
    print(f"{shape} {mode} {kind}: {float(np.max(err / bound)):.3e} of the derived bound"
          + (f", relative error per bin {sr.max_rel(got, ref):.3e} (allowed {sr.REL_MARGIN * sr.EMULATION_MAX_REL:.3e})" if kind == "white" else ""))
    assert np.all(err <= bound)
    if kind == "white":
        assert sr.max_rel(got, ref) <= sr.REL_MARGIN * sr.EMULATION_MAX_REL
    parseval = np.abs(got.sum(axis=1) - ss)  # a check of its own: the bound is of the norm's error, far below the bins' bounds added up
    print(f"    Parseval: {float(np.max(parseval / np.maximum(sr.parseval_bound(H, W, ss), 1e-300))):.3e} of its bound")
    assert np.all(parseval <= sr.parseval_bound(H, W, ss))


@pytest.mark.parametrize("shape", [(520, 12), (12, 1000), (1024, 6), (1024, 1024)])
def test_sizes_past_the_wide_strip(shape):
    """H > 512 takes strips of 8 columns instead of 16 (the LDS planes of a strip must fit a CU); W = 1000 is the longest table and K
    loop short of the limit; 1024 x 1024 is the largest size, whose strip and tables take the whole 160 KB of LDS: the derived bound
    and Parseval, with and without sub"""
    H, W = shape
    rng = np.random.default_rng(H + W)
    x = rng.standard_normal((2, H, W)).astype(np.float32)
    sub = (0.5 + 0.3 * rng.standard_normal((1, H, W))).astype(np.float32)
    counts = ops.radial_bins(H, W)[1].numpy()
    for args in ((x,), (x, sub, 2)):
        got, ref, ss = run(*args).cpu().numpy(), sr.reference(*args), sumsq(*args)
        assert np.all(np.abs(got - ref) <= sr.derived_bound(H, W, counts, ss))
        assert np.all(np.abs(got.sum(axis=1) - ss) <= sr.parseval_bound(H, W, ss))


@pytest.mark.parametrize("shape, fy, fx", [((64, 64), 3, 5), ((17, 23), 2, 4), ((80, 48), 0, 24), ((16, 40), 8, 0)])
def test_a_pure_cosine_lands_in_its_bin(shape, fy, fx):
    H, W = shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.cos(2 * np.pi * ((fy * y) % H / H + (fx * x) % W / W)).astype(np.float32)[None]
    bins, counts, _ = ops.radial_bins(H, W)
    k = int(bins[fy, fx])
    got = run(img)[0].cpu().numpy()
    ss = sumsq(img)
    # the float32 rounding of the pixels is white noise of about 2^-48 sum a^2 in all: far inside the bound of any bin
    bound = sr.derived_bound(H, W, counts.numpy(), ss)[0] + 2.0 ** -44 * ss[0]
    others = np.delete(got, k)
    assert np.all(others <= np.delete(bound, k)) and abs(got[k] - ss[0]) <= bound[k] + others.sum()


def test_decomposition_through_power_spectra():
    """mean_s P(member_s)[k] = P(mean)[k] + mean_s P(member_s - mean)[k]: members on a grid of 1/8 and S = 4, so that the float32 mean
    of ops.ensemble_stats is the exact one; the mean as the target turns member_residuals into P(member_s - mean)"""
    rng = np.random.default_rng(11)
    B, S, H, W = 2, 4, 24, 40
    samples = dev((rng.integers(-64, 65, (B, S, 1, H, W)) / 8.0).astype(np.float32))
    mean, _ = ops.ensemble_stats(samples)
    assert torch.equal(mean.double(), samples.double().mean(dim=1))
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    n0 = ops.launch_count()
    sp = driftSDE.power_spectra(samples, mean)
    assert ops.launch_count() == n0 + 1 + 2 * 3  # ensemble_stats, then two radial_power_spectrum calls of three launches
    nb = ops.radial_bins(H, W)[1].numel()
    assert sp["output"].shape == sp["target"].shape == sp["residual"].shape == (B, 1, nb)
    assert sp["members"].shape == sp["member_residuals"].shape == (B, 1, S, nb)
    assert torch.equal(bits64(sp["output"]), bits64(sp["target"])) and not sp["residual"].any()
    lhs = sp["members"].mean(dim=2).cpu().numpy()[:, 0]
    rhs = (sp["output"] + sp["member_residuals"].mean(dim=2)).cpu().numpy()[:, 0]
    ss = (samples.double() ** 2).sum(dim=(2, 3, 4)).max(dim=1).values.cpu().numpy()
    assert np.all(np.abs(lhs - rhs) <= 3.0 * sr.derived_bound(H, W, ops.radial_bins(H, W)[1].numpy(), ss))
    own = driftSDE.power_spectra(samples)
    assert set(own) == {"output", "members"} and torch.equal(bits64(own["members"]), bits64(sp["members"]))
    one = driftSDE.power_spectra(mean, mean)
    assert set(one) == {"output", "target", "residual"} and torch.equal(bits64(one["output"]), bits64(sp["output"]))
    with pytest.raises(ValueError):
        driftSDE.power_spectra(samples[0, 0, 0])
    with pytest.raises(ValueError):
        driftSDE.power_spectra(samples, mean[:, :, :, :W // 2])


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 23), (80, 48)])
def test_bits_do_not_depend_on_the_rows_the_chunking_or_the_run(shape):
    H, W = shape
    rng = np.random.default_rng(H)
    x = rng.standard_normal((5, H, W)).astype(np.float32)
    full = run(x)
    assert torch.equal(bits64(full), bits64(run(x)))
    for r in (0, 2, 4):
        assert torch.equal(bits64(run(x[r:r + 1])[0]), bits64(full[r]))
    lib = _lib.load()
    two = int(lib.idiff_radial_power_spectrum_ws_bytes(2, H, W))
    n0 = ops.launch_count()
    chunked = run(x, max_ws_bytes=two)
    assert ops.launch_count() == n0 + 3 * 3  # rows 0-1, 2-3, 4
    assert torch.equal(bits64(chunked), bits64(full))
    assert torch.equal(bits64(run(x, max_ws_bytes=1)), bits64(full))  # one row per call at the least


def test_sub_is_one_exact_subtraction():
    """integer-valued images: the float64 difference is exact in float32, so the rows of the host-subtracted difference are the same
    numbers and give the same bits; under any chunking, also one that cuts a group of sub_rep rows"""
    rng = np.random.default_rng(5)
    H, W = 17, 23
    x = rng.integers(-1000, 1001, (6, H, W)).astype(np.float32)
    sub = rng.integers(-1000, 1001, (2, H, W)).astype(np.float32)
    diff = sr.row_images(x, sub, 3)
    assert np.array_equal(diff, diff.astype(np.float32).astype(np.float64))
    want = run(diff.astype(np.float32))
    got = run(x, sub, 3)
    assert torch.equal(bits64(got), bits64(want))
    lib = _lib.load()
    for rows in (1, 2, 3, 4):
        assert torch.equal(bits64(run(x, sub, 3, max_ws_bytes=int(lib.idiff_radial_power_spectrum_ws_bytes(rows, H, W)))), bits64(want)), rows
    assert torch.equal(bits64(run(x, x, 1)), torch.zeros(6, want.shape[1], dtype=torch.int64, device=DEV))  # +0.0 in every bin


# ---- 3. non-finite rows, hostile bins, refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 23), (64, 64)])
def test_non_finite_rows_are_nan_and_the_others_untouched(shape):
    H, W = shape
    rng = np.random.default_rng(W)
    x = rng.standard_normal((5, H, W)).astype(np.float32)
    clean = run(x)
    bad = x.copy()
    bad[1, H - 1, W - 1], bad[3, H // 2, 0] = np.nan, np.inf
    got = run(bad)
    for r in (1, 3):
        assert (bits64(got[r]) == QNAN64).all()
    for r in (0, 2, 4):
        assert torch.equal(bits64(got[r]), bits64(clean[r]))
    sub = np.zeros((5, H, W), dtype=np.float32)
    sub[2, 0, 0] = -np.inf
    got = run(x, sub, 1)
    assert (bits64(got[2]) == QNAN64).all() and torch.equal(bits64(got[[0, 1, 3, 4]]), bits64(clean[[0, 1, 3, 4]]))


def test_hostile_bins_drop_their_points():
    """entries of -1 and nb are a defined input: their points are dropped, the other bins keep their bits"""
    H, W = 17, 23
    x = sr.case((H, W), "plain")[0]
    table, counts, _ = ops.radial_bins(H, W)
    nb = counts.numel()
    clean = run(x)
    assert torch.equal(bits64(run(x, bins=table.to(DEV), nb=nb)), bits64(clean))
    hostile = table.clone()
    hit = [(0, 0), (3, 2), (16, 11), (9, 5)]
    for i, (u, v) in enumerate(hit):
        hostile[u, v] = -1 if i % 2 == 0 else nb
    hostile[5, 7], hostile[6, 1] = -2 ** 31, 2 ** 31 - 1
    touched = sorted({int(table[u, v]) for u, v in hit + [(5, 7), (6, 1)]})
    keep = [k for k in range(nb) if k not in touched]
    got = run(x, bins=hostile.to(DEV), nb=nb)
    assert torch.equal(bits64(got[:, keep]), bits64(clean[:, keep]))
    want = sr.reference(x, bins=hostile.numpy(), nb=nb)
    assert np.all(np.abs(got.cpu().numpy() - want) <= sr.derived_bound(H, W, counts.numpy(), sumsq(x)))
    assert (got[:, touched] < clean[:, touched]).all()
    fewer = run(x, bins=table.to(DEV), nb=5)  # the bins past nb are dropped as a whole
    assert fewer.shape == (x.shape[0], 5) and torch.equal(bits64(fewer), bits64(clean[:, :5]))


def test_refusals():
    x = torch.zeros(6, 8, 8, device=DEV)
    with pytest.raises(_lib.IdiffError, match="sub_rep"):
        ops.radial_power_spectrum(x, torch.zeros(2, 8, 8, device=DEV), 4)
    with pytest.raises(_lib.IdiffError):
        ops.radial_power_spectrum(torch.zeros(1, 0, 8, device=DEV))
    with pytest.raises(_lib.IdiffError):
        ops.radial_power_spectrum(torch.zeros(1, 2, 1025, device=DEV))
    with pytest.raises(_lib.IdiffError):
        ops.radial_power_spectrum(x.cpu())
    # the entry point itself: it launches nothing and leaves out as it was
    lib = _lib.load()
    table = ops.radial_bins(8, 8)[0].to(DEV)
    out = torch.full((6, 7), -1.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.idiff_radial_power_spectrum_ws_bytes(6, 8, 8)) // 8, dtype=torch.float64, device=DEV)
    sub = torch.zeros(2, 8, 8, device=DEV)

    def call(sub_t, sub_rep, nb, R, H, W):
        return lib.idiff_radial_power_spectrum(C.c_void_p(x.data_ptr()), None if sub_t is None else C.c_void_p(sub_t.data_ptr()), sub_rep,
                                               C.c_void_p(table.data_ptr()), nb, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), R, H, W,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))

    n0 = ops.launch_count()
    for args, word in [((sub, 4, 7, 6, 8, 8), "sub_rep"), ((sub, 0, 7, 6, 8, 8), "sub_rep"), ((None, 1, 0, 6, 8, 8), "nb"),
                       ((None, 1, 7, 6, 0, 8), "H = 0"), ((None, 1, 7, 1, 2, 1025), "W = 1025"), ((None, 1, 7, 0, 8, 8), "bad args")]:
        with pytest.raises(_lib.IdiffError, match=word):
            _lib.check(call(*args), "radial_power_spectrum")
    assert ops.launch_count() == n0 and (out == -1.0).all()
    _lib.check(call(sub, 3, 7, 6, 8, 8), "radial_power_spectrum")
    _lib.check(call(None, 0, 7, 6, 8, 8), "radial_power_spectrum")  # sub_rep is ignored without sub
    assert ops.launch_count() == n0 + 6 and not out.any()


# ---- 4. the model and testUM ----------------------------------------------------------------------------------------------------------
T, HM = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=2, num_samples=3))
    model.set_eval()
    return model, sde


def test_model_power_spectra(built):
    model, sde = built
    _, counts, _ = ops.radial_bins(HM, HM)
    nb = counts.numel()
    model.feed_data(make_batch(2, HM, seed=3))
    model.test(return_samples=True)
    sp = model.power_spectra()
    assert set(sp) == {"output", "target", "residual", "members", "member_residuals"}
    assert sp["output"].shape == (2, 1, nb) and sp["members"].shape == (2, 1, 3, nb) and all(torch.isfinite(v).all() for v in sp.values())

    def parseval(spec, img):
        ss = (img.double() ** 2).sum(dim=(-2, -1))
        assert torch.all((spec.sum(dim=-1) - ss).abs() <= 1e-12 * ss)

    parseval(sp["output"], model.output), parseval(sp["target"], model.target)
    parseval(sp["residual"], model.output.double() - model.target.double())
    parseval(sp["members"], model.samples.transpose(1, 2)), parseval(sp["member_residuals"], (model.samples.double() - model.target.double()[:, None]).transpose(1, 2))
    rec = spectrum_summary(sp, counts, 3, L=HM)
    assert rec["n"] == 2 and len(rec["SSR_k"]) == nb and rec["HF_RATIO_output"] > 0 and rec["HF_RATIO_member"] >= rec["HF_RATIO_output"]
    assert rec["SSR_HF"] > 0 and rec["LSD_output"] > 0
    assert set(model.power_spectra(with_target=False)) == {"output", "members"}
    # the plain chain: S = 1
    sde.set_num_samples(1)
    try:
        model.test()
        assert model.samples is None
        sp = model.power_spectra()
        assert set(sp) == {"output", "target", "residual"} and all(v.shape == (2, 1, nb) and torch.isfinite(v).all() for v in sp.values())
        parseval(sp["output"], model.output), parseval(sp["residual"], model.output.double() - model.target.double())
        rec = spectrum_summary(sp, counts, 1, L=HM)
        assert rec["HF_RATIO_output"] > 0 and math.isnan(rec["SSR_HF"])
    finally:
        sde.set_num_samples(3)


NEW_WORDS = ("HF_RATIO", "LSD", "SSR_HF", "spectra")


@pytest.mark.parametrize("S", [1, 3])
def test_testum_spectra_option(tmp_path, capsys, S):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {HM}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_spec").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "1", "--sample-T", "2"] + (["--num-samples", str(S)] if S > 1 else [])
    res = testUM.main(common + ["--spectra"])
    out = capsys.readouterr().out
    words = ("HF_RATIO=", "LSD=", "spectra pooled over 1 images: HF_RATIO:") + (("HF_RATIO_member=", "LSD_member=", "SSR_HF=") if S > 1 else ())
    for word in words:
        assert word in out, word
    if S == 1:
        assert "_member" not in out and "SSR_HF" not in out
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 1
    nb = ops.radial_bins(HM, HM)[1].numel()
    for name, v in done.items():
        folder = tmp_path / "results" / "drv_spec" / name
        with_spectra = sorted(os.listdir(folder))
        pooled = json.load(open(folder / "spectra.json"))
        assert pooled["S"] == S and len(pooled["freq"]) == len(pooled["counts"]) == len(pooled["PSD_output"]) == nb and sum(pooled["counts"]) == HM * HM
        assert pooled["HF_RATIO_output"] == v['HF_RATIO'][0] == v['pooled_spectra'][(HM, HM)]['HF_RATIO_output'] and pooled["HF_RATIO_output"] > 0
        one = json.load(open(folder / [f for f in with_spectra if f.endswith("_spectra.json")][0]))
        assert set(one) == {"S", "freq", "counts", "PSD_output", "PSD_target", "PSD_residual"} | ({"PSD_member", "PSD_member_residual"} if S > 1 else set())
        # the PSDs are on RMSE's x/2 + 0.5 scale: the mean of PSD_residual over the frequency plane is RMSE^2
        mse = sum(p * c for p, c in zip(one["PSD_residual"], one["counts"])) / (HM * HM)
        assert mse == pytest.approx(v['RMSE'][0] ** 2, rel=1e-4)
    # without the flag: the same lines without the new words, and the folder holds what it held
    cfg.write_text(txt.replace("name: drv_spec", "name: drv_plain"))
    res = testUM.main(common)
    printed = capsys.readouterr().out.replace(str(tmp_path), "")
    for word in NEW_WORDS:
        assert word not in printed, word
    for name, v in res.items():
        if v['num']:
            assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR'} | ({'PSNR_member', 'STD'} if S > 1 else set())
            plain = sorted(os.listdir(tmp_path / "results" / "drv_plain" / name))
            assert len(plain) == (2 if S > 1 else 1) * v['num']
            assert plain == [f for f in sorted(os.listdir(tmp_path / "results" / "drv_spec" / name)) if "spectra" not in f]
