"""Posterior ensembles of tiled chains (driftSDE tiled_ensemble) on the host: the switch and max_chain_rows options, the grouping of the
ensemble's rows into chains, and the new step's symbol in the header, the bindings and the library."""
import ctypes
import re

import pytest

from instancediff_amd import _lib
from instancediff_amd.models.SDEs import create_sde
from instancediff_amd.models.SDEs.driftSDE import chain_groups, driftSDE

NEW = "idiff_drift_reverse_step_tiled_members_dev"


# ---- 1. the switch --------------------------------------------------------------------------------------------------------------
def test_tiled_ensemble_is_off_by_default_and_takes_bools_only():
    sde = driftSDE(T=8)
    assert sde.tiled_ensemble is False and sde.max_chain_rows == 128
    assert driftSDE(T=8, tiled_ensemble=None).tiled_ensemble is False
    assert driftSDE(T=8, tiled_ensemble=True).tiled_ensemble is True
    assert driftSDE(T=8, tiled_ensemble=False).tiled_ensemble is False
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError, match="tiled_ensemble"):
            driftSDE(T=8, tiled_ensemble=bad)
        with pytest.raises(ValueError, match="tiled_ensemble"):
            sde.set_tiled_ensemble(bad)
    assert sde.tiled_ensemble is False  # a refused value changes nothing
    sde.set_tiled_ensemble(True)
    assert sde.tiled_ensemble is True
    sde.set_tiled_ensemble(None)
    assert sde.tiled_ensemble is False


def test_the_switch_lets_num_samples_and_tiling_meet_in_any_order():
    sde = driftSDE(T=8, num_samples=2, tile=16, tiled_ensemble=True)
    assert sde.num_samples == 2 and sde.tile == (16, 16) and sde.tiled_ensemble is True
    sde = driftSDE(T=8, tiled_ensemble=True)
    sde.set_num_samples(2)
    sde.set_tiling(16)
    assert sde.num_samples == 2 and sde.tile == (16, 16)
    sde = driftSDE(T=8, tiled_ensemble=True)
    sde.set_tiling(16, 4)
    sde.set_num_samples(3)
    assert sde.num_samples == 3 and sde.tile_overlap == (4, 4)
    sde = driftSDE(T=8, tile=16)
    sde.set_tiled_ensemble(True)
    sde.set_num_samples(2)
    assert sde.num_samples == 2
    sde = create_sde({}, dict(class_name="driftSDE", T=8, num_samples=2, tile=[16, 32], tiled_ensemble=True, max_chain_rows=9))
    assert sde.tiled_ensemble is True and sde.num_samples == 2 and sde.tile == (16, 32) and sde.max_chain_rows == 9


def test_turning_the_switch_off_while_both_are_set_is_refused():
    sde = driftSDE(T=8, num_samples=2, tile=16, tiled_ensemble=True)
    for off in (False, None):
        with pytest.raises(ValueError, match="tiled_ensemble"):
            sde.set_tiled_ensemble(off)
        assert sde.tiled_ensemble is True
    sde.set_num_samples(None)
    sde.set_tiled_ensemble(False)
    assert sde.tiled_ensemble is False
    with pytest.raises(ValueError, match="num_samples"):  # and the refusal is back, naming the switch
        sde.set_num_samples(2)
    with pytest.raises(ValueError, match="tiled_ensemble"):
        sde.set_num_samples(2)
    sde = driftSDE(T=8, num_samples=2, tile=16, tiled_ensemble=True)
    sde.set_tiling(None)
    sde.set_tiled_ensemble(False)
    with pytest.raises(ValueError, match="num_samples"):
        sde.set_tiling(16)


def test_without_the_switch_every_refusal_stays():
    for kw in (dict(), dict(tiled_ensemble=False), dict(tiled_ensemble=None)):
        with pytest.raises(ValueError, match="num_samples"):
            driftSDE(num_samples=2, tile=16, **kw)


@pytest.mark.parametrize("bad", [True, False, 2.0, "8", 0, -1, None])
def test_max_chain_rows_is_validated(bad):
    with pytest.raises(ValueError, match="max_chain_rows"):
        driftSDE(T=8, max_chain_rows=bad)
    sde = driftSDE(T=8)
    if bad is not None:  # None leaves the setter's value alone, as max_batch's
        with pytest.raises(ValueError, match="max_chain_rows"):
            sde.set_num_samples(None, max_chain_rows=bad)
    assert sde.max_chain_rows == 128


def test_max_chain_rows_is_set_where_max_batch_is():
    sde = driftSDE(T=8, max_chain_rows=9, max_batch=4)
    assert sde.max_chain_rows == 9 and sde.max_batch == 4
    sde.set_num_samples(None, max_batch=2, max_chain_rows=20)
    assert sde.max_chain_rows == 20 and sde.max_batch == 2
    sde.set_num_samples(None)
    assert sde.max_chain_rows == 20 and sde.max_batch == 2


# ---- 2. the grouping ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,nwin,rows,sizes", [(6, 9, 128, [6]), (6, 9, 9, [1] * 6), (6, 9, 20, [2, 2, 2]), (5, 4, 9, [2, 2, 1]),
                                               (3, 25, 16, [1, 1, 1])])
def test_chain_groups(R, nwin, rows, sizes):
    groups = chain_groups(R, nwin, rows)
    assert [r1 - r0 for r0, r1 in groups] == sizes
    assert [r for r0, r1 in groups for r in range(r0, r1)] == list(range(R))  # 0..R once, in order
    assert all((r1 - r0) * nwin <= max(rows, nwin) for r0, r1 in groups)


def test_chain_groups_cover_every_row_once():
    for R in range(1, 12):
        for nwin in (1, 2, 4, 9, 20):
            for rows in (1, 3, 8, 9, 128, 10 ** 6):
                groups = chain_groups(R, nwin, rows)
                assert [r for r0, r1 in groups for r in range(r0, r1)] == list(range(R)), (R, nwin, rows)
                G = max(1, rows // nwin)
                assert all(r1 - r0 == G for r0, r1 in groups[:-1]) and 1 <= groups[-1][1] - groups[-1][0] <= G
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError):
            chain_groups(4, 4, bad)
    with pytest.raises(ValueError):
        chain_groups(0, 4, 8)


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NEW in header and NEW in _lib.SIGNATURES and hasattr(lib, NEW)
    assert sorted(_lib.SIGNATURES) == header


def test_the_binding_has_the_headers_argument_count():
    with open(_lib.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in (NEW, "idiff_drift_reverse_step_tiled_dev", "idiff_drift_reverse_step_members_dev"):
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the tiled step's arguments with (members_dev, seed) in place of (seed, nper, offset_base)
    assert len(_lib.SIGNATURES[NEW][1]) == len(_lib.SIGNATURES["idiff_drift_reverse_step_tiled_dev"][1]) - 1
