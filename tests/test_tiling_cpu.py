"""Tiled sampling on the host: the per-axis window plan of driftSDE (origins, blend zones, weight and coverage tables) over a sweep of
sizes, its spot values, and the option validators."""
import numpy as np
import pytest

from instancediff_amd.models.SDEs.driftSDE import TilePlan, driftSDE, tile_axis_plan

SWEEP = [(P, O, L, align) for P in (8, 16, 32) for O in range(0, P // 2 + 1, 4) for L in range(4, 5 * P + 1, 4) for align in (1, 4)]


def test_axis_plan_sweep():
    for P, O, L, align in SWEEP:
        pl = tile_axis_plan(L, P, O, align=align)
        o, n, ext = pl["origins"], pl["n"], pl["P"]
        tag = (P, O, L, align)
        if L <= P:
            assert n == 1 and o == [0] and ext == L and pl["zones"] == [], tag
        else:
            assert n == -(-(L - O) // (P - O)) and ext == P, tag
        assert len(o) == n and o[0] == 0 and o[-1] == L - ext, tag
        assert all(0 < b - a <= P - O for a, b in zip(o, o[1:])), (tag, o)
        assert all(v % align == 0 for v in o), (tag, o)
        first, w0, w1 = pl["first"], pl["w0"], pl["w1"]
        assert first.dtype == np.int32 and w0.dtype == np.float32 and w1.dtype == np.float32
        assert first.shape == w0.shape == w1.shape == (L,)
        # the weight of every window at every coordinate, from the tables
        wt = np.zeros((n + 1, L))
        c = np.arange(L)
        wt[first, c] += w0
        wt[first + 1, c] += w1
        assert not wt[n].any(), tag  # no weight on a window that does not exist
        wt = wt[:n]
        assert (w0 > 0).all(), tag  # the lower slot is the owner or the zone's lower window
        for i in range(n):
            inside = (c >= o[i]) & (c < o[i] + ext)
            assert not wt[i][~inside].any(), (tag, i)  # weight only inside the window's extent
        assert ((wt != 0).sum(axis=0) <= 2).all(), tag  # at most two, adjacent by construction (first, first + 1)
        assert (np.abs(w0.astype(np.float64) + w1.astype(np.float64) - 1.0) <= 2.0 ** -23).all(), tag
        assert (((w0 == 1.0) & (w1 == 0.0)) | ((w0 < 1.0) & (w1 > 0.0))).all(), tag
        # zones: one per consecutive pair, disjoint and ordered, two weights inside and one outside
        zones = pl["zones"]
        assert len(zones) == n - 1, tag
        in_zone = np.zeros(L, dtype=bool)
        for i, (a, b) in enumerate(zones):
            assert a == o[i + 1] and b == min(o[i] + ext, o[i + 2] if i + 2 < n else L) and a <= b, (tag, i)
            assert not in_zone[a:b].any(), (tag, i)
            in_zone[a:b] = True
            z = b - a
            for k in range(z):
                beta = (k + 0.5) / z
                assert first[a + k] == i and w1[a + k] == np.float32(beta) and w0[a + k] == np.float32(1.0 - beta), (tag, i, k)
        assert all(za[1] <= zb[0] for za, zb in zip(zones, zones[1:])), tag
        assert ((w1 != 0) == in_zone).all(), tag
        # coverage: exactly the windows whose extent holds the coordinate
        for cc in range(L):
            want = [i for i in range(n) if o[i] <= cc < o[i] + ext]
            assert list(range(pl["cov_lo"][cc], pl["cov_hi"][cc])) == want, (tag, cc)
        assert (wt.sum(axis=0) > 0).all(), tag


def test_axis_plan_spot_values():
    a = tile_axis_plan(40, 16, 4)
    assert a["origins"] == [0, 12, 24] and a["zones"] == [(12, 16), (24, 28)]
    assert a["first"].tolist() == [0] * 16 + [1] * 12 + [2] * 12
    assert a["w1"][12:16].tolist() == [0.125, 0.375, 0.625, 0.875] and a["w0"][12:16].tolist() == [0.875, 0.625, 0.375, 0.125]
    assert a["w0"][:12].tolist() == [1.0] * 12 and not a["w1"][16:24].any()
    b = tile_axis_plan(20, 16, 8)
    assert b["origins"] == [0, 4] and b["zones"] == [(4, 16)]
    assert tile_axis_plan(40, 16, 4, align=4)["origins"] == [0, 12, 24]
    # three windows overlap physically at 13..15, two of them carry weight
    c = tile_axis_plan(36, 16, 8)
    assert c["origins"] == [0, 6, 13, 20] and c["zones"] == [(6, 13), (13, 20), (20, 29)]
    assert (c["cov_hi"] - c["cov_lo"])[13:16].tolist() == [3, 3, 3] and c["first"][13:16].tolist() == [1, 1, 1]
    assert tile_axis_plan(36, 16, 8, align=4)["origins"] == [0, 4, 12, 20]
    one = tile_axis_plan(12, 16, 4)
    assert one["n"] == 1 and one["P"] == 12 and one["w0"].tolist() == [1.0] * 12


def test_tile_plan_grid_and_rows():
    plan = TilePlan(24, 40, (16, 16), (4, 4))
    assert plan.grid == (2, 3, 16, 16)
    yy, xx = plan.window_index()
    assert yy.shape == (6, 16, 16)
    assert yy[4, 0, 0] == 8 and xx[4, 0, 0] == 12 and xx[5, 0, 15] == 39  # row iy * nx + ix
    assert TilePlan(32, 32, (32, 32), (4, 4)).grid == (1, 1, 32, 32)
    assert TilePlan(48, 64, (16, 32), (0, 0)).grid == (3, 2, 16, 32)
    with pytest.raises(ValueError):
        TilePlan(32, 30, (16, 16), (4, 4))


@pytest.mark.parametrize("bad", [True, 16.0, "16", 18, 0, -16, [16], [16, 16, 16], [16, 18], [16, True], [16.0, 16]])
def test_tile_option_is_validated(bad):
    with pytest.raises(ValueError):
        driftSDE(tile=bad)
    sde = driftSDE()
    with pytest.raises(ValueError):
        sde.set_tiling(bad)
    assert sde.tile is None


@pytest.mark.parametrize("bad", [True, 4.0, "4", 2, 6, -4, 12, [4, 4]])
def test_tile_overlap_option_is_validated(bad):
    with pytest.raises(ValueError):
        driftSDE(tile=16, tile_overlap=bad)
    sde = driftSDE(tile=16)
    with pytest.raises(ValueError):
        sde.set_tiling(16, bad)
    assert sde.tile == (16, 16) and sde.tile_overlap == (0, 0)


def test_tile_options_defaults_and_off():
    sde = driftSDE()
    assert sde.tile is None and sde.tile_overlap is None and sde.last_tiles is None
    assert driftSDE(tile=None, tile_overlap=None).tile is None
    for P, O in ((16, 0), (32, 4), (64, 8), (224, 28), (256, 32), (36, 4)):
        assert driftSDE(tile=P).tile_overlap == (O, O), P
    sde = driftSDE(tile=[16, 64])
    assert sde.tile == (16, 64) and sde.tile_overlap == (0, 8)
    sde.set_tiling((32, 16), 8)
    assert sde.tile == (32, 16) and sde.tile_overlap == (8, 8)
    with pytest.raises(ValueError):  # 16 exceeds half of the smaller window
        sde.set_tiling([64, 16], 16)
    sde.set_tiling(None)
    assert sde.tile is None and sde.tile_overlap is None
    with pytest.raises(ValueError):
        sde.set_tiling(None, 4)
    assert driftSDE(tile=16, tile_overlap=8).tile_overlap == (8, 8)


def test_num_samples_with_tiling_is_refused():
    with pytest.raises(ValueError, match="num_samples"):
        driftSDE(num_samples=2, tile=16)
    sde = driftSDE(tile=16)
    with pytest.raises(ValueError, match="num_samples"):
        sde.set_num_samples(2)
    assert sde.num_samples == 1
    sde = driftSDE(num_samples=2)
    with pytest.raises(ValueError, match="num_samples"):
        sde.set_tiling(16)
    assert sde.tile is None
    driftSDE(num_samples=1, tile=16)  # one sample is no ensemble
