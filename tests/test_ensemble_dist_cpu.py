"""Ensemble member distances (energy score, medoid, best-of-S) on the host: the C ABI's new symbols, the float64 emulation of the contract
(tests/ensemble_dist_ref.py) on exact integers and against the per-pixel scores' emulation, ensemble_distance_summary on hand-made
matrices, the tie rule, the medoid's root form, and the propriety of ES_FAIR on a seeded synthetic ensemble."""
import ctypes
import math

import numpy as np
import pytest
import torch
from ensemble_dist_ref import draw_int, emulate, exact_int, picks, summary
from ensemble_scores_ref import emulate as emulate_scores

from instancediff_amd import _lib
from instancediff_amd.models.SDEs.driftSDE import ensemble_distance_summary

NEW_SYMBOLS = ["idiff_ensemble_distances", "idiff_ensemble_distances_ws_bytes", "idiff_ensemble_pick_rows"]
SCORE_KEYS = ("ES", "ES_FAIR", "DIVERSITY", "RMS_member", "RMS_best", "RMS_medoid")


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header


def test_workspace_size():
    """64 parts per image, one 8 x 8 fp64 tile per part and tile pair ti <= tj of the M x M matrix, and 8 bytes of counts per part"""
    lib = _lib.load()
    for B, S, ht in [(1, 1, 0), (1, 1, 1), (3, 7, 1), (3, 8, 1), (16, 16, 1), (16, 33, 0), (65535, 64, 1)]:
        nt = (S + ht + 7) // 8
        assert lib.idiff_ensemble_distances_ws_bytes(B, S, ht) == B * 64 * (nt * (nt + 1) // 2 * 64 * 8 + 8)
    assert lib.idiff_ensemble_distances_ws_bytes(1, 64, 1) <= 1.5 * 2 ** 20  # near 1 MiB per image at the largest S
    for B, S in [(0, 4), (1, 0), (1, 65), (65536, 4), (-1, 4)]:
        assert lib.idiff_ensemble_distances_ws_bytes(B, S, 1) == 0


# ---- 2. the emulation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 5, 16, 17])
def test_emulation_is_exact_on_integers(S):
    """integer-valued rows with |value| <= 2^10: every difference, square and partial sum is an integer below 2^53, so float64 in any order
    equals int64 arithmetic"""
    x, y = draw_int(S, 300, seed=S)
    em = emulate(x, y)
    want = exact_int(x, y)
    assert em["counts"] == (300, 0) and np.array_equal(em["d2"], want.astype(np.float64)) and want.max() < 2 ** 53
    assert np.array_equal(em["d2"], em["d2"].T) and not em["d2"].diagonal().any()
    bare = emulate(x)
    assert np.array_equal(bare["d2"], em["d2"][:S, :S]) and bare["pick"][1] == -1 and bare["pick"][0] == em["pick"][0]
    assert em["pick"][1] == int(np.argmin(want[:S, S]))  # np.argmin returns the first minimum


def test_invalid_pixels_in_the_emulation():
    x, y = draw_int(3, 8, seed=1)
    x[1, 2], x[0, 5], y[5], y[7] = np.nan, np.inf, np.nan, -np.inf
    em = emulate(x, y)
    assert np.nonzero(~em["valid"])[0].tolist() == [2, 5, 7] and em["counts"] == (5, 3)
    keep = [0, 1, 3, 4, 6]
    assert np.array_equal(em["d2"], exact_int(x[:, keep], y[keep]).astype(np.float64))
    bare = emulate(x)  # without the target its pixels do not count: only 2 and 5 are invalid
    assert bare["counts"] == (6, 2)
    dead = emulate(np.full((3, 4), np.nan, dtype=np.float32), np.zeros(4, dtype=np.float32))
    assert dead["counts"] == (0, 4) and not dead["d2"].any() and dead["pick"] == (0, 0)


def test_identities_against_the_per_pixel_scores():
    """S = 5, members y + 5 k with small integers k and y: in the per-pixel emulation d_s = 5 k_s, m = sum k and v = ss/4 are exact
    integers or quarter-integers in float32, so with the sums over the pixels
        sum_{i<j} d2[i][j] = S (S - 1) sum v            (sum_{i<j} (d_i - d_j)^2 = S sum_s (d_s - m)^2 = S (S - 1) v per pixel)
        sum_i d2[i][S]     = S sum e + (S - 1) sum v    (sum_s d_s^2 = S m^2 + sum_s (d_s - m)^2 per pixel)
    hold as equalities"""
    S, n = 5, 200
    rng = np.random.default_rng(5)
    y = rng.integers(-20, 21, n).astype(np.float32)
    k = rng.integers(-6, 7, (S, n))
    x = (y[None] + 5 * k).astype(np.float32)
    sc = emulate_scores(x, y)
    assert np.array_equal(sc["d"], (5 * k).astype(np.float32)) and np.array_equal(sc["e"], (k.sum(axis=0) ** 2).astype(np.float32))
    sum_e, sum_v = float(sc["e"].astype(np.float64).sum()), float(sc["v"].astype(np.float64).sum())
    d2 = emulate(x, y)["d2"]
    assert sum(d2[i, j] for i in range(S) for j in range(i + 1, S)) == S * (S - 1) * sum_v
    assert sum(d2[i, S] for i in range(S)) == S * sum_e + (S - 1) * sum_v


# ---- 3. ensemble_distance_summary ------------------------------------------------------------------------------------------------------
def test_summary_by_hand():
    # S = 2 on a line, 4 pixels, members at 0 and 4 everywhere, the truth at 1: distances 8 (members), 2 and 6 (to the truth); r = 2
    d2 = [[0.0, 64.0, 4.0], [64.0, 0.0, 36.0], [4.0, 36.0, 0.0]]
    got = ensemble_distance_summary([d2], [[4, 0]], 2, True)
    assert got["RMS_member"] == [2.0] and got["RMS_best"] == [1.0] and got["RMS_medoid"] == [1.0] and got["DIVERSITY"] == [4.0]
    assert got["ES"] == [(4.0 - 16.0 / 8.0) / 2.0] == [1.0] and got["ES_FAIR"] == [(4.0 - 16.0 / 4.0) / 2.0] == [0.0]
    assert got["medoid"] == [0] and got["best"] == [0] and got["valid"] == [4] and got["invalid"] == [0]  # a two-member tie: the lower index
    # S = 1: the score is the distance, nothing pairwise exists
    one = ensemble_distance_summary([[[0.0, 9.0], [9.0, 0.0]]], [[9, 1]], 1, True)
    assert one["ES"] == [1.0] and one["RMS_member"] == one["RMS_best"] == one["RMS_medoid"] == [1.0] and one["invalid"] == [1]
    assert math.isnan(one["ES_FAIR"][0]) and math.isnan(one["DIVERSITY"][0]) and one["medoid"] == [0] and one["best"] == [0]
    # no target: the score keys are NaN, the diversity stands
    bare = ensemble_distance_summary([[[0.0, 64.0], [64.0, 0.0]]], [[4, 0]], 2, False)
    assert bare["DIVERSITY"] == [4.0] and bare["best"] == [-1] and all(math.isnan(bare[q][0]) for q in SCORE_KEYS if q != "DIVERSITY")
    # an image with no valid pixel: everything NaN; the mean over images is then NaN too, the other image is untouched
    two = ensemble_distance_summary([d2, [[0.0] * 3] * 3], [[4, 0], [0, 4]], 2, True)
    assert two["ES"][0] == 1.0 and all(math.isnan(two[q][1]) for q in SCORE_KEYS) and two["medoid"][1] == 0 and two["best"][1] == 0
    assert math.isnan(two["mean"]["ES"]) and two["mean"]["valid"] == 2.0
    both = ensemble_distance_summary([d2, [[4 * v for v in row] for row in d2]], [[4, 0], [4, 0]], 2, True)  # pooling is the mean
    assert both["ES"] == [1.0, 2.0] and both["mean"]["ES"] == 1.5 and both["mean"]["DIVERSITY"] == 6.0
    assert ensemble_distance_summary(torch.tensor([d2], dtype=torch.float64), torch.tensor([[4, 0]], dtype=torch.int32), 2, True) == got
    assert ensemble_distance_summary(np.array([d2]), np.array([[4, 0]]), 2, True) == got
    with pytest.raises(ValueError):
        ensemble_distance_summary([d2, d2], [[4, 0]], 2, True)
    with pytest.raises(ValueError):
        ensemble_distance_summary([d2], [[4, 0]], 0, True)


@pytest.mark.parametrize("S", [1, 2, 6, 17])
def test_summary_against_the_definitions(S):
    x, y = draw_int(S, 64, seed=100 + S, lim=30)
    em = emulate(x, y)
    got = ensemble_distance_summary(em["d2"][None], [em["counts"]], S, True)
    want = summary(em["d2"], em["counts"][0], S, True)
    for q in SCORE_KEYS:
        assert (math.isnan(got[q][0]) and math.isnan(want[q])) or got[q][0] == pytest.approx(want[q], rel=1e-13), q
    assert (got["medoid"][0], got["best"][0]) == em["pick"]
    if S > 1:  # the two forms differ by the bias term alone
        assert got["ES"][0] - got["ES_FAIR"][0] == pytest.approx(got["DIVERSITY"][0] / (2 * S), rel=1e-12)


# ---- 4. the picks ------------------------------------------------------------------------------------------------------------------------
def test_duplicated_members_pick_the_lower_index():
    x, y = draw_int(5, 32, seed=9, lim=50)
    x[3] = x[1]          # members 1 and 3 are one image
    x[4] = x[1]
    em = emulate(x, y)
    assert em["d2"][1, 3] == 0.0 and np.array_equal(em["d2"][1], em["d2"][3])
    medoid, best = em["pick"]
    assert medoid not in (3, 4) and best not in (3, 4)
    all_same = emulate(np.repeat(x[:1], 4, axis=0), y)
    assert all_same["pick"] == (0, 0)
    assert picks(np.zeros((4, 4)), 3, True) == (0, 0) and picks(np.zeros((1, 1)), 1, False) == (0, -1)


def test_the_medoid_is_not_the_member_nearest_to_the_mean():
    """6 members of 64 pixels, member s = scale_s * N(0, 1) with scale_s ~ U(0.2, 3): with squared distances the central member is the one
    nearest to the mean (sum_j |x_i - x_j|^2 = S |x_i - mean|^2 + const); with the roots it is another member in a few draws of a hundred"""
    rng = np.random.default_rng(0)
    differ = 0
    for _ in range(200):
        x = (rng.uniform(0.2, 3, (6, 1)) * rng.normal(0, 1, (6, 64))).astype(np.float32)
        d2 = emulate(x)["d2"]
        medoid = picks(d2, 6, False)[0]
        nearest = int(np.argmin(((x.astype(np.float64) - x.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1)))
        assert nearest == int(np.argmin(d2.sum(axis=1)))  # the squared form IS the member nearest to the mean
        differ += medoid != nearest
    print(f"the medoid differs from the member nearest to the mean in {differ} of 200 draws")
    assert differ >= 1


# ---- 5. propriety ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_es_fair_prefers_the_calibrated_ensemble(seed):
    """200 images of 256 pixels, S = 4, value = mu + scale * (0.1 g + 0.05 g_pixel) with one g per draw (spatially coherent error) and one
    g_pixel per pixel; the truth at scale 1, the members at scale 0.5 / 1 / 2.  The mean ES_FAIR is lowest for the calibrated ensemble;
    the plain ES carries the finite-ensemble bias of the empirical-CDF form and is printed beside it (at S = 4 it prefers scale 0.5)."""
    S, n, images = 4, 256, 200
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-1, 1, (images, n))

    def draws(scale, k):
        return mu[:, None, :] + scale * (0.1 * rng.normal(0, 1, (images, k, 1)) + 0.05 * rng.normal(0, 1, (images, k, n)))

    truth = draws(1.0, 1)[:, 0].astype(np.float32)
    fair, plain = {}, {}
    for scale in (0.5, 1.0, 2.0):
        members = draws(scale, S).astype(np.float32)
        ems = [emulate(members[b], truth[b]) for b in range(images)]
        got = ensemble_distance_summary(np.stack([e["d2"] for e in ems]), [e["counts"] for e in ems], S, True)
        fair[scale], plain[scale] = got["mean"]["ES_FAIR"], got["mean"]["ES"]
    print(f"seed {seed}: mean ES_FAIR at scale 0.5 / 1 / 2: {fair[0.5]:.4f} / {fair[1.0]:.4f} / {fair[2.0]:.4f}; "
          f"plain ES: {plain[0.5]:.4f} / {plain[1.0]:.4f} / {plain[2.0]:.4f}")
    assert fair[1.0] < fair[0.5] and fair[1.0] < fair[2.0]
