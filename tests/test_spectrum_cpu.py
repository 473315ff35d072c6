"""Radial power spectra on the host: the bin rule of ops.radial_bins, the float64 emulation of the kernel's contract
(tests/spectrum_ref.py) against np.fft.rfft2, the C ABI's new symbols and workspace rule, spectrum_summary on hand-made spectra, the
spread decomposition per frequency, and testUM's parser."""
import ctypes
import json
import math

import numpy as np
import pytest
import spectrum_ref as sr
import torch

from instancediff_amd import _lib, ops
from instancediff_amd.models.SDEs.driftSDE import spectrum_summary

NEW_SYMBOLS = ["idiff_radial_power_spectrum", "idiff_radial_power_spectrum_ws_bytes"]


# ---- 1. the bin rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 7, 16, 33, 224])
def test_bins_on_squares_are_the_rounded_radius(N):
    """H = W = L: the rule reduces to (2k - 1)^2 <= 4 (u'^2 + v'^2) < (2k + 1)^2"""
    bins, counts, freq = ops.radial_bins(N, N)
    assert bins.dtype == torch.int32 and tuple(bins.shape) == (N, N // 2 + 1) and counts.dtype == torch.int64 and freq.dtype == torch.float64
    for u in range(N):
        for v in range(N // 2 + 1):
            k, q = int(bins[u, v]), 4 * (min(u, N - u) ** 2 + v * v)
            assert k >= 0 and (k == 0 or (2 * k - 1) ** 2 <= q) and q < (2 * k + 1) ** 2, (u, v, k)
    assert freq.tolist() == [k / N for k in range(counts.numel())]


@pytest.mark.parametrize("shape, nb", [((224, 224), 159), ((256, 256), 182), ((24, 40), 29), ((17, 23), 16), ((6, 10), 8)])
def test_bin_counts(shape, nb):
    H, W = shape
    bins, counts, freq = ops.radial_bins(H, W)
    assert counts.numel() == nb == int(bins.max()) + 1 == freq.numel() and int(bins.min()) == 0 and int(bins[0, 0]) == 0
    assert int(counts.sum()) == H * W and int(counts.min()) >= 1
    w = sr.weights(W)
    assert counts.tolist() == np.bincount(bins.numpy().reshape(-1), weights=np.broadcast_to(w, (H, W // 2 + 1)).reshape(-1)).astype(int).tolist()
    assert freq[-1] == (nb - 1) / max(H, W)


@pytest.mark.parametrize("shape", [(6, 10), (17, 23), (24, 40), (16, 16), (9, 4)])
def test_bins_of_the_transposed_image(shape):
    """the bin of a frequency does not depend on which axis is halved: radial_bins(H, W)[u, v] == radial_bins(W, H)[v, u] wherever both
    tables hold the point (u <= H/2, v <= W/2)"""
    H, W = shape
    a, b = ops.radial_bins(H, W)[0], ops.radial_bins(W, H)[0]
    assert torch.equal(a[:H // 2 + 1, :], b[:W // 2 + 1, :].t())
    assert ops.radial_bins(H, W)[1].numel() == ops.radial_bins(W, H)[1].numel()


def test_bins_are_exact_past_2_to_53():
    """L = 1024: the products reach 2^61, past what float64 holds exactly; the corner (512, 512) of 1024^2 is exactly 512 sqrt(2) = 724.08 -> 724"""
    bins, counts, _ = ops.radial_bins(1024, 1024)
    assert int(bins[512, 512]) == 724 and counts.numel() == 725 and int(counts.sum()) == 1024 * 1024
    assert 4 * 1024 ** 2 * (512 ** 2 * 1024 ** 2 * 2) == 2 ** 61 > 2 ** 53
    with pytest.raises(ValueError):
        ops.radial_bins(0, 4)
    with pytest.raises(ValueError):
        ops.radial_bins(4, 2.0)


# ---- 2. the emulation -----------------------------------------------------------------------------------------------------------------
def test_the_recorded_emulation_error_is_the_measured_one():
    """EMULATION_MAX_REL was measured here, on exactly the white-noise cases the GPU test runs; another BLAS may move it a little"""
    got = sr.measure_emulation()
    print(f"emulation against np.fft.rfft2, largest relative error per bin: {got:.3e} (recorded {sr.EMULATION_MAX_REL:.3e})")
    assert got <= sr.REL_MARGIN * sr.EMULATION_MAX_REL


@pytest.mark.parametrize("kind", ["white", "dc"])
def test_emulation_within_the_derived_bound_and_parseval(kind):
    worst = 0.0
    for shape, mode in sr.all_cases():
        x, sub, rep = sr.case(shape, mode, kind)
        a = sr.row_images(x, sub, rep)
        sumsq = (a * a).sum(axis=(1, 2))
        em, ref = sr.emulate(x, sub, rep), sr.case_reference(shape, mode, kind)
        bound = sr.derived_bound(shape[0], shape[1], ops.radial_bins(*shape)[1].numpy(), sumsq)
        assert np.all(np.abs(em - ref) <= bound), (shape, mode)
        worst = max(worst, float(np.max(np.abs(em - ref) / bound)))
        assert np.all(np.abs(em.sum(axis=1) - sumsq) <= 4 * 2.0 ** -52 * sumsq), (shape, mode)
    print(f"{kind}: the emulation uses at most {worst:.2e} of the derived bound")


def test_emulation_edge_rules():
    x = np.random.default_rng(2).integers(-9, 10, (2, 6, 10)).astype(np.float32)
    bins, counts, _ = ops.radial_bins(6, 10)
    nb = counts.numel()
    clean = sr.emulate(x)
    hostile = bins.numpy().copy()
    hostile[0, 0], hostile[3, 2] = -1, nb
    got = sr.emulate(x, bins=hostile, nb=nb)
    k0, k1 = 0, int(bins[3, 2])
    keep = [k for k in range(nb) if k not in (k0, k1)]
    assert np.array_equal(got[:, keep], clean[:, keep]) and np.all(got[:, k0] < clean[:, k0]) and np.all(got[:, k1] < clean[:, k1])
    bad = x.copy()
    bad[1, 2, 3] = np.inf
    out = sr.emulate(bad)
    assert np.isnan(out[1]).all() and np.array_equal(out[0], clean[0])


def test_decomposition_identity_in_the_emulation():
    """mean_s P(member_s)[k] = P(mean)[k] + mean_s P(member_s - mean)[k] when the mean is exact: members on a grid of 1/8 and S = 4 keep
    the float64 mean and the differences exact in float32"""
    rng = np.random.default_rng(3)
    S, H, W = 4, 17, 23
    members = (rng.integers(-64, 65, (S, H, W)) / 8.0).astype(np.float32)
    mean = members.astype(np.float64).mean(axis=0)
    assert np.array_equal(mean, mean.astype(np.float32).astype(np.float64))
    lhs = sr.emulate(members).mean(axis=0)
    p_mean = sr.emulate(mean.astype(np.float32)[None])[0]
    p_dev = sr.emulate(members, sub=mean.astype(np.float32)[None], sub_rep=S).mean(axis=0)
    counts = ops.radial_bins(H, W)[1].numpy()
    bound = 3.0 * sr.derived_bound(H, W, counts, [float((members.astype(np.float64) ** 2).sum(axis=(1, 2)).max())])[0]
    assert np.all(np.abs(lhs - (p_mean + p_dev)) <= bound)
    assert np.all(p_dev >= 0) and p_dev.sum() > 0


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header


def test_workspace_size():
    """the twiddle table (16 bytes per index of W and of H), a 4-byte flag per row padded to 8 bytes, and one fp64 plane [H][W/2 + 1]
    per row"""
    lib = _lib.load()
    for R, H, W in [(1, 1, 1), (3, 17, 23), (6, 80, 48), (34, 256, 256), (9, 224, 224), (65535, 8, 8), (2, 1024, 1024)]:
        assert lib.idiff_radial_power_spectrum_ws_bytes(R, H, W) == 16 * (W + H) + 8 * ((R + 1) // 2) + 8 * R * H * (W // 2 + 1)
    assert lib.idiff_radial_power_spectrum_ws_bytes(1, 256, 256) < 300 * 1024
    for R, H, W in [(0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1025, 8), (1, 8, 1025), (-1, 8, 8)]:
        assert lib.idiff_radial_power_spectrum_ws_bytes(R, H, W) == 0


# ---- 4. spectrum_summary ------------------------------------------------------------------------------------------------------------
def _hand(L=16):
    counts = ops.radial_bins(L, L)[1]
    nb = counts.numel()
    target = torch.arange(1, nb + 1, dtype=torch.float64) * counts.to(torch.float64)  # PSD_target[k] = k + 1
    return counts, nb, target


def test_summary_of_a_truth_equal_output():
    counts, nb, target = _hand()
    got = spectrum_summary(dict(output=target[None], target=target[None], residual=torch.zeros(1, nb, dtype=torch.float64)), counts, 1)
    assert got["n"] == 1 and got["PSD_target"] == [float(k + 1) for k in range(nb)] == got["PSD_output"]
    assert got["RATIO_output"] == [1.0] * nb and got["HF_RATIO_output"] == 1.0 and got["LSD_output"] == 0.0
    assert got["SKILL_PSD"] == [0.0] * nb
    assert all(math.isnan(v) for v in got["SPREAD_PSD"]) and all(math.isnan(v) for v in got["SSR_k"]) and math.isnan(got["SSR_HF"])
    assert "RATIO_member" not in got


def test_summary_of_a_halved_high_band():
    L = 16
    counts, nb, target = _hand(L)
    output = target.clone()
    hf = [k for k in range(nb) if 4 * k > L]
    assert hf[0] == 5
    output[hf] *= 0.5
    got = spectrum_summary(dict(output=[output.tolist()], target=[target.tolist()], residual=[[1.0] * nb]), counts, 1, L=L)
    assert got["HF_RATIO_output"] == 0.5 and got["RATIO_output"][:5] == [1.0] * 5 and got["RATIO_output"][5:] == [0.5] * (nb - 5)
    # LSD over 1 <= k <= L/2 = 8: bins 5 .. 8 are 10 log10(0.5) off, bins 1 .. 4 are not
    assert got["LSD_output"] == pytest.approx(math.sqrt(4 * (10 * math.log10(0.5)) ** 2 / 8), rel=1e-14)
    # pooling: sums with sums; a second image with twice the power everywhere changes no ratio
    two = spectrum_summary(dict(output=torch.stack([output, 2 * output]), target=torch.stack([target, 2 * target]),
                                residual=torch.ones(2, nb, dtype=torch.float64)), counts, 1, L=L)
    assert two["n"] == 2 and two["HF_RATIO_output"] == 0.5 and two["PSD_target"] == [1.5 * (k + 1) for k in range(nb)]


def test_summary_of_an_ensemble_and_zero_denominators():
    L, S = 16, 4
    counts, nb, target = _hand(L)
    c = counts.to(torch.float64)
    # per frequency point: the mean holds 1, every member 1 + 3/4 (variance about the mean 3/4 -> unbiased 1), the squared error 5/4:
    # a reliable ensemble, SSR_k = sqrt((S + 1)/S * 1 / (5/4)) = 1
    spectra = dict(output=c[None].clone(), target=target[None], residual=1.25 * c[None],
                   members=(1.75 * c).expand(1, S, nb).clone(), member_residuals=(2.0 * c).expand(1, S, nb).clone())
    got = spectrum_summary(spectra, counts, S, L=L)
    assert got["SPREAD_PSD"] == [1.0] * nb and got["SKILL_PSD"] == [1.25] * nb and got["SSR_HF"] == 1.0
    assert got["SSR_k"] == [1.0] * nb and got["PSD_member"] == [1.75] * nb and got["PSD_member_residual"] == [2.0] * nb
    assert got["RATIO_member"] == [1.75 / (k + 1) for k in range(nb)]
    # a zero denominator gives NaN there and only there
    spectra["residual"][0, 3] = 0.0
    spectra["target"] = target[None].clone()
    spectra["target"][0, 2] = 0.0
    got = spectrum_summary(spectra, counts, S, L=L)
    assert math.isnan(got["SSR_k"][3]) and got["SSR_k"][2] == 1.0 and math.isnan(got["RATIO_output"][2]) and math.isnan(got["RATIO_member"][2])
    assert not math.isnan(got["RATIO_output"][3]) and not math.isnan(got["LSD_output"]) and got["SKILL_PSD"][3] == 0.0
    dead = spectrum_summary(dict(output=torch.zeros(1, nb), target=torch.zeros(1, nb), residual=torch.zeros(1, nb)), counts, 1, L=L)
    assert math.isnan(dead["HF_RATIO_output"]) and math.isnan(dead["LSD_output"]) and all(math.isnan(v) for v in dead["RATIO_output"])
    with pytest.raises(ValueError):
        spectrum_summary(dict(output=torch.zeros(2, nb), target=torch.zeros(1, nb), residual=torch.zeros(1, nb)), counts, 1)
    with pytest.raises(ValueError):
        spectrum_summary(spectra, counts, 0)


def test_summary_default_scale_is_the_square_images():
    counts = ops.radial_bins(224, 224)[1]
    nb = counts.numel()
    flat = counts.to(torch.float64)[None]
    a = spectrum_summary(dict(output=flat, target=flat, residual=flat), counts, 1)
    b = spectrum_summary(dict(output=flat, target=flat, residual=flat), counts, 1, L=224)
    assert json.dumps(a) == json.dumps(b) and len(a["PSD_output"]) == nb  # as text: NaN entries compare equal
    # a non-square image's scale cannot be read off its counts: 24 x 40 (the root of 960 is no integer) and 16 x 64 (1024 = 32^2, but
    # the counts are not those of 32 x 32) are refused without L and served with it
    for H, W in [(24, 40), (16, 64)]:
        c = ops.radial_bins(H, W)[1]
        f = c.to(torch.float64)[None]
        with pytest.raises(ValueError, match="L = max"):
            spectrum_summary(dict(output=f, target=f, residual=f), c, 1)
        got = spectrum_summary(dict(output=f, target=f, residual=f), c, 1, L=max(H, W))
        assert got["HF_RATIO_output"] == 1.0 and got["LSD_output"] == 0.0


# ---- 5. testUM ------------------------------------------------------------------------------------------------------------------------
def _parser_namespace(argv):
    """testUM.main builds its parser inside: stop it at the first thing it does after parsing, opening the options file"""
    from instancediff_amd import testUM
    seen = {}
    real = testUM.argparse.ArgumentParser.parse_args

    def spy(self, args=None, namespace=None):
        seen["ns"] = real(self, args, namespace)
        return seen["ns"]

    testUM.argparse.ArgumentParser.parse_args = spy
    try:
        with pytest.raises(FileNotFoundError):
            testUM.main(argv)
    finally:
        testUM.argparse.ArgumentParser.parse_args = real
    return seen["ns"]


def test_testum_pools_spectra_per_image_size():
    from instancediff_amd.testUM import pool_spectra

    def one(H, W, scale):
        c = ops.radial_bins(H, W)[1].to(torch.float64)[None, None]
        return H, W, dict(output=scale * c, target=c.clone(), residual=c.clone())

    got = pool_spectra([one(16, 16, 1.0), one(24, 40, 0.5), one(16, 16, 3.0)], 1)
    assert sorted(got) == [(16, 16), (24, 40)] and got[(16, 16)]["n"] == 2 and got[(24, 40)]["n"] == 1
    assert got[(16, 16)]["HF_RATIO_output"] == 2.0 and got[(24, 40)]["HF_RATIO_output"] == 0.5
    assert len(got[(24, 40)]["PSD_output"]) == 29 and pool_spectra([], 1) == {}


def test_testum_parses_spectra():
    on = _parser_namespace(["-opt", "/nonexistent/options.yml", "--spectra"])
    off = _parser_namespace(["-opt", "/nonexistent/options.yml"])
    assert on.spectra is True and off.spectra is False
    rest = {k: v for k, v in vars(off).items() if k != "spectra"}
    assert rest == {k: v for k, v in vars(on).items() if k != "spectra"}
    assert rest == dict(opt="/nonexistent/options.yml", random_init=False, limit=0, sample_T=None, solver_order=None, num_samples=None,
                        max_batch=None, interval=None, scores=False, distances=False, tile=None, tile_overlap=None, tiled_ensemble=False,
                        max_chain_rows=None, reuse_graph=False, self_ensemble=None)
