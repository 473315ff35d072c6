"""Credible intervals of posterior ensembles (driftSDE interval) on the host: the order-statistic index rule on a table worked out by
hand, the option's validation, and the C ABI's new symbols."""
import ctypes
from fractions import Fraction

import pytest

from instancediff_amd import _lib
from instancediff_amd.models.SDEs import create_sde
from instancediff_amd.models.SDEs.driftSDE import driftSDE, order_stat_indices

NEW_SYMBOLS = ["idiff_ensemble_order_stats", "idiff_interval_coverage", "idiff_interval_coverage_ws_ints"]


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header


# ---- 2. the index rule ----------------------------------------------------------------------------------------------------------
# (S, L) -> (k_lo, k_hi, k_m0, k_m1, nominal), by hand: k_lo = floor((1 - L)/2 * (S - 1))
#   (2, .9):    .05 * 1   = .05  -> 0;  k_hi = 1;   median 0, 1;   nominal 1/3
#   (4, .9):    .05 * 3   = .15  -> 0;  k_hi = 3;   median 1, 2;   nominal 3/5       (min / max)
#   (5, .5):    .25 * 4   = 1    -> 1;  k_hi = 3;   median 2, 2;   nominal 2/6
#   (16, .9):   .05 * 15  = .75  -> 0;  k_hi = 15;  median 7, 8;   nominal 15/17
#   (21, .9):   .05 * 20  = 1    -> 1;  k_hi = 19;  median 10, 10; nominal 18/22     (in doubles (1 - 0.9)/2 * 20 = 0.99999999999999978 -> 0)
#   (41, .95):  .025 * 40 = 1    -> 1;  k_hi = 39;  median 20, 20; nominal 38/42
#   (101, .9):  .05 * 100 = 5    -> 5;  k_hi = 95;  median 50, 50; nominal 90/102
TABLE = [
    (2, 0.9, 0, 1, 0, 1, Fraction(1, 3)),
    (4, 0.9, 0, 3, 1, 2, Fraction(3, 5)),
    (5, 0.5, 1, 3, 2, 2, Fraction(2, 6)),
    (16, 0.9, 0, 15, 7, 8, Fraction(15, 17)),
    (21, 0.9, 1, 19, 10, 10, Fraction(18, 22)),
    (41, 0.95, 1, 39, 20, 20, Fraction(38, 42)),
    (101, 0.9, 5, 95, 50, 50, Fraction(90, 102)),
]


@pytest.mark.parametrize("S,L,k_lo,k_hi,k_m0,k_m1,nominal", TABLE)
def test_order_stat_indices_table(S, L, k_lo, k_hi, k_m0, k_m1, nominal):
    idx = order_stat_indices(S, L)
    assert set(idx) == {"k_lo", "k_hi", "k_m0", "k_m1", "nominal"}
    assert (idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]) == (k_lo, k_hi, k_m0, k_m1)
    assert all(isinstance(idx[k], int) and not isinstance(idx[k], bool) for k in ("k_lo", "k_hi", "k_m0", "k_m1"))
    assert idx["nominal"] == pytest.approx(float(nominal), rel=0, abs=1e-15)


def test_the_float_trap():
    assert (1 - 0.9) / 2 * 20 < 1.0  # what double arithmetic would floor to 0
    assert order_stat_indices(21, 0.9)["k_lo"] == 1


LEVELS = [0.01, 0.1, 0.25, 0.5, 0.683, 0.8, 0.9, 0.95, 0.99, 0.999]


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 8, 16, 17, 21, 41, 100, 101])
def test_order_stat_indices_invariants(S):
    prev = None
    for L in LEVELS:
        idx = order_stat_indices(S, L)
        assert idx["k_lo"] + idx["k_hi"] == S - 1
        assert 0 <= idx["k_lo"] <= idx["k_m0"] <= idx["k_m1"] <= idx["k_hi"] < S
        assert (idx["k_m0"], idx["k_m1"]) == ((S - 1) // 2, S // 2)
        assert idx["nominal"] == (idx["k_hi"] - idx["k_lo"]) / (S + 1)
        assert 0.0 <= idx["nominal"] < 1.0
        assert prev is None or idx["nominal"] >= prev, (S, L)  # non-decreasing in L
        prev = idx["nominal"]


@pytest.mark.parametrize("bad", [True, 1, 0, "0.9", 0.0, 1.0, -0.5, 1.5, float("nan")])
def test_order_stat_indices_refuses_bad_levels(bad):
    with pytest.raises(ValueError):
        order_stat_indices(8, bad)


# ---- 3. the option --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [True, False, 1, 0, -1, "0.9", 0.0, 1.0, -0.9, 2.5, float("nan"), [0.9]])
def test_interval_refuses(value):
    with pytest.raises(ValueError):
        driftSDE(T=10, interval=value)
    sde = driftSDE(T=10, interval=0.8)
    with pytest.raises(ValueError):
        sde.set_interval(value)
    assert sde.interval == 0.8


def test_interval_on_and_off():
    sde = driftSDE(T=10)
    assert sde.interval is None and sde.last_order_stats is None
    sde.set_interval(0.9)
    assert sde.interval == 0.9 and isinstance(sde.interval, float)
    sde.set_interval(None)
    assert sde.interval is None
    sde.set_interval(0.5)
    sde.set_interval()
    assert sde.interval is None


def test_interval_is_legal_without_an_ensemble_and_beside_tiling():
    sde = driftSDE(T=10, interval=0.9, tile=32)  # num_samples = 1: the plain (tiled) chain runs and the option does nothing
    assert sde.num_samples == 1 and sde.interval == 0.9 and sde.tile == (32, 32)
    sde.set_tiling(None)
    sde.set_num_samples(4)
    assert sde.interval == 0.9
    with pytest.raises(ValueError):  # the refusal of an ensemble of a tiled chain is untouched
        sde.set_tiling(32)


def test_interval_reaches_the_sde_through_create_sde():
    sde = create_sde({}, dict(class_name="driftSDE", T=20, sample_T=5, num_samples=8, interval=0.95))
    assert (sde.num_samples, sde.interval) == (8, 0.95)
    assert create_sde({}, dict(class_name="driftSDE", T=20)).interval is None
