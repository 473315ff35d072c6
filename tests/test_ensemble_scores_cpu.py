"""Ensemble scores (CRPS, rank histogram, spread-skill) on the host: the float32 emulation of the contract in include/idiff.h against
the textbook formulas in float64, the identities, ensemble_score_summary, a calibrated synthetic ensemble, and the C ABI's new symbols."""
import ctypes
import math

import numpy as np
import pytest
import torch
from ensemble_scores_ref import U, draw, emulate, image_record, textbook

from instancediff_amd import _lib
from instancediff_amd.models.SDEs.driftSDE import ensemble_score_summary

NEW_SYMBOLS = ["idiff_ensemble_scores", "idiff_ensemble_scores_ws_bytes"]


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
    lib = _lib.load()
    for B, S in [(1, 1), (3, 16), (16, 33), (65535, 1024)]:
        assert lib.idiff_ensemble_scores_ws_bytes(B, S) == B * 64 * (3 * 8 + (S + 2) * 4)
    for B, S in [(0, 4), (1, 0), (1, 1025), (65536, 4), (-1, 4)]:
        assert lib.idiff_ensemble_scores_ws_bytes(B, S) == 0


# ---- 2. the emulation against the textbook formulas ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 17, 33])
def test_emulation_against_the_float64_reference(S):
    """300 pixels per S (2 100 draws in all).  Per pixel D = max_s |x_s - y|, u = 2^-24, a factor 2 as the only margin of the derived bounds:
    crps: |crps - ref| <= (2 S + 4) u D, the bound the contract was written against.
    m = (sum d_s)/S: each d_s carries one rounding (u D); a sequential fp32 sum of S terms of at most D adds (S - 1) u S D; the
      quotient scales both to (1 + (S - 1)) u D = S u D and rounds once more (u D): |m - ref| <= (S + 1) u D.
    e = m*m: 2 |m| (S + 1) u D + u m^2 <= (2 S + 3) u D^2.  Assert |e - ref| <= 2 (2 S + 3) u D^2.
    v: t_s = d_s - m (|t_s| <= 2 D) carries u D of d_s, (S + 1) u D of m and its own rounding 2 u D: (S + 4) u D; its square
      2 |t_s| (S + 4) u D + u t_s^2 <= 4 (S + 5) u D^2; S such terms 4 S (S + 5) u D^2, and their sequential sum, S terms of at
      most 4 D^2, (S - 1) u S 4 D^2: together 8 S (S + 2) u D^2; the quotient by S - 1 scales that and rounds v <= 4 S D^2/(S - 1)
      once more: |v - ref| <= 4 S (2 S + 5) u D^2/(S - 1).  Assert twice that."""
    x, y = draw(S, 300, seed=S)
    em, ref = emulate(x, y), textbook(x, y)
    assert em["valid"].all()
    assert np.array_equal(em["ranks"], ref["ranks"])
    assert np.array_equal(np.sort(em["ranks"], axis=0), np.arange(S)[:, None].repeat(300, axis=1))  # a permutation in every pixel
    assert np.array_equal(em["k"], ref["k"])
    D = np.abs(x.astype(np.float64) - y.astype(np.float64)[None]).max(axis=0)
    def within(name, err, bound):  # err <= bound in every pixel (D = 0, every member on the truth: both are 0); the worst ratio is printed
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        print(f"S={S}: {name} error / bound {worst:.3f}")
        assert (err <= bound).all(), (name, worst)

    within("crps", np.abs(em["crps"] - ref["crps"]), (2 * S + 4) * U * D)
    within("e", np.abs(em["e"] - ref["e"]), 2 * (2 * S + 3) * U * D * D)
    if S > 1:
        within("v", np.abs(em["v"] - ref["v"]), 2 * 4 * S * (2 * S + 5) * U * D * D / (S - 1))
    else:
        assert not em["v"].any() and np.array_equal(em["crps"], np.abs(x[0] - y))


def test_identities():
    rng = np.random.default_rng(3)
    y = rng.uniform(-1, 1, 64).astype(np.float32)
    one = (y + rng.normal(0, 0.3, 64)).astype(np.float32)
    em = emulate(one[None], y)  # S = 1: crps = |x - y|, v = 0
    assert np.array_equal(em["crps"], np.abs(one - y)) and not em["v"].any() and np.array_equal(em["e"], (one - y) * (one - y))
    em = emulate(np.repeat(one[None], 4, axis=0), y)  # all members equal: the pairwise term vanishes (S = 4: every quotient exact)
    assert np.array_equal(em["crps"], np.abs(one - y)) and not em["v"].any()
    assert np.array_equal(em["ranks"], np.arange(4)[:, None].repeat(64, axis=1))  # ties in index order
    # by hand: members (0, 1), truth 0.25: (0.25 + 0.75)/2 - (|0 - 1| + |1 - 0|)/(2*4) = 0.5 - 0.25
    em = emulate(np.array([[0.0], [1.0]], dtype=np.float32), np.array([0.25], dtype=np.float32))
    assert em["crps"][0] == 0.25 and em["k"][0] == 1 and em["e"][0] == 0.0625 and em["v"][0] == 0.5
    # a member equal to the truth is not below it
    em = emulate(np.array([[0.5], [0.25], [0.25]], dtype=np.float32), np.array([0.25], dtype=np.float32))
    assert em["k"][0] == 0 and em["ranks"][:, 0].tolist() == [2, 0, 1]
    # NaN in a member or in the target: invalid
    em = emulate(np.array([[0.5, np.nan, 0.1], [0.25, 0.0, 0.2]], dtype=np.float32), np.array([0.25, 0.0, np.nan], dtype=np.float32))
    assert em["valid"].tolist() == [True, False, False]
    sums, counts = image_record(em, 2)
    assert counts.tolist() == [1, 0, 0, 2] and sums[0] == float(em["crps"][0])


# ---- 3. ensemble_score_summary ------------------------------------------------------------------------------------------------------
def test_summary_pools_rows():
    S = 3
    sums = [[2.0, 8.0, 6.0], [1.0, 1.0, 3.0]]
    counts = [[1, 2, 3, 4, 1], [3, 2, 1, 0, 0]]  # hist[0..3], invalid
    got = ensemble_score_summary(sums, counts, S)
    # pooled: sums (3, 9, 9), hist (4, 4, 4, 4), N = 16, invalid 1
    assert got["N"] == 16 and got["invalid"] == 1 and got["hist"] == [4, 4, 4, 4]
    assert got["CRPS"] == 3.0 / 16
    assert got["SKILL"] == math.sqrt(9.0 / 16) and got["SPREAD"] == math.sqrt(4.0 / 3.0 * 9.0 / 16)
    assert got["SSR"] == got["SPREAD"] / got["SKILL"] == pytest.approx(math.sqrt(4.0 / 3.0))
    assert got["RANK_DEV"] == 0.0  # flat once pooled, though neither image's histogram is
    assert got["OUTLIERS"] == 0.5 and got["OUTLIERS_nominal"] == 0.5
    one = ensemble_score_summary(sums[0], counts[0], S)
    assert one["N"] == 10 and one["CRPS"] == 0.2 and one["RANK_DEV"] == pytest.approx(0.15 + 0.05 + 0.05 + 0.15)
    two = ensemble_score_summary(sums[1], counts[1], S)
    assert got["CRPS"] != pytest.approx(0.5 * (one["CRPS"] + two["CRPS"]))  # pooling is not the mean of the per-image ratios
    assert ensemble_score_summary(torch.tensor(sums, dtype=torch.float64), torch.tensor(counts, dtype=torch.int32), S) == got
    assert ensemble_score_summary(np.array(sums), np.array(counts), S) == got


def test_summary_ssr_nan_rules_and_extremes():
    assert math.isnan(ensemble_score_summary([1.0, 4.0, 0.0], [3, 5, 0], 1)["SSR"])       # S = 1: no spread to compare
    assert math.isnan(ensemble_score_summary([1.0, 0.0, 2.0], [1, 1, 1, 0], 2)["SSR"])    # SKILL = 0
    assert ensemble_score_summary([1.0, 2.0, 2.0], [1, 1, 1, 0], 2)["SSR"] == pytest.approx(math.sqrt(1.5))
    empty = ensemble_score_summary([0.0, 0.0, 0.0], [0, 0, 0, 7], 2)                     # nothing valid
    assert empty["N"] == 0 and empty["invalid"] == 7 and all(math.isnan(empty[q]) for q in ("CRPS", "SKILL", "SPREAD", "SSR", "RANK_DEV", "OUTLIERS"))
    for S in (1, 4, 9):
        flat = ensemble_score_summary([1.0, 1.0, 1.0], [5] * (S + 1) + [0], S)
        assert flat["RANK_DEV"] == pytest.approx(0.0, abs=1e-15) and flat["OUTLIERS"] == pytest.approx(2.0 / (S + 1))
        assert flat["OUTLIERS_nominal"] == 2.0 / (S + 1)
        below = ensemble_score_summary([1.0, 1.0, 1.0], [40] + [0] * S + [0], S)         # every truth below all members
        assert below["RANK_DEV"] == pytest.approx(2.0 * S / (S + 1)) and below["OUTLIERS"] == 1.0
    with pytest.raises(ValueError):
        ensemble_score_summary([[1.0, 1.0, 1.0]] * 2, [[1, 1, 1, 0]], 2)
    with pytest.raises(ValueError):
        ensemble_score_summary([1.0, 1.0, 1.0], [1, 1, 1, 0], 0)


# ---- 4. a calibrated ensemble --------------------------------------------------------------------------------------------------------
def test_a_calibrated_ensemble_scores_as_one():
    """members and truth i.i.d. N(0, 1), S = 8, 20 000 pixels: the truth is one more member, so SSR -> 1 and the histogram is flat up to
    sampling noise (expected RANK_DEV: S + 1 bins of sqrt(2/pi) sqrt(p (1 - p)/N) each, p = 1/9: about 0.016)"""
    S, n = 8, 20000
    rng = np.random.default_rng(11)
    x = rng.normal(0, 1, (S, n)).astype(np.float32)
    y = rng.normal(0, 1, n).astype(np.float32)
    sums, counts = image_record(emulate(x, y), S)
    got = ensemble_score_summary(sums, counts, S)
    print({k: got[k] for k in ("CRPS", "SKILL", "SPREAD", "SSR", "RANK_DEV", "OUTLIERS")})
    assert got["N"] == n and got["invalid"] == 0
    assert abs(got["SSR"] - 1.0) < 0.05 and got["RANK_DEV"] < 0.05
    assert abs(got["OUTLIERS"] - got["OUTLIERS_nominal"]) < 0.02
    halved = ensemble_score_summary(*image_record(emulate(0.5 * x, y), S), S)  # an under-dispersed ensemble reads as one
    assert halved["SSR"] < 0.6 and halved["RANK_DEV"] > 0.2 and halved["OUTLIERS"] > 2 * halved["OUTLIERS_nominal"]
