"""tests/image_metrics_ref.py against the scipy oracle, and the witness that its row table can fail: on the rows marked with a dagger
(locally flat, bright or saturated images) the fp32 emulation of the raw-moment kernel (sum w a^2 - (sum w a)^2) misses the row's SSIM
bound by at least 10x, while the centred form the kernel now has defines that bound."""
import numpy as np
import pytest

from image_metrics_ref import GRID, SSIM_FLOOR, _reduce32, cases, emulate32, make, reference, ssim_bound
from oracle import metrics_ref

ROWS = cases()
IDS = [r["id"] for r in ROWS]


def test_the_table_holds_what_it_names():
    assert len(set(IDS)) == len(IDS) and all(isinstance(r["seed"], int) for r in ROWS)
    shapes = {(r["B"], r["H"], r["W"]) for r in ROWS}
    for s in [(1, 11, 11), (1, 11, 40), (1, 40, 11), (2, 12, 31), (3, 48, 48), (1, 129, 128), (1, 128, 129), (2, 256, 256), (65, 16, 16), (64, 16, 16)]:
        assert s in shapes
    assert 129 * 128 - GRID == 128  # 128 threads make a second trip
    assert sum(r["chan1"] for r in ROWS) == 1
    assert sorted(r["id"] for r in ROWS if r["dagger"]) == sorted(f"{k}-{h}x{w}" for k in ("flat95", "flat98", "sat", "flat0")
                                                                   for h, w in ((11, 11), (12, 31), (48, 48)))
    p, t = make(next(r for r in ROWS if r["chan1"]))
    assert not p.flags["C_CONTIGUOUS"] and not t.flags["C_CONTIGUOUS"]
    p, t = make(next(r for r in ROWS if r["kind"] == "same"))
    assert p is t
    p, t = make(next(r for r in ROWS if r["id"] == "sat-11x11"))
    assert (t == 1.0).all() and (p <= 1.0).all() and (p >= 1.0 - 2e-3).all()
    for r in ROWS:
        p, t = make(r)
        assert p.dtype == np.float32 and p.shape == (r["B"], r["H"], r["W"]) and np.abs(p).max() <= 1 and np.abs(t).max() <= 1


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_reference_equals_the_scipy_oracle(row):
    p, t = make(row)
    for b in sorted({0, row["B"] - 1}):
        with np.errstate(divide="ignore"):  # the oracle's PSNR of an exact match
            got, want = reference(p[b], t[b]), metrics_ref.metrics(p[b], t[b])
        if row["kind"] in ("const", "same"):
            assert got[0] == 0.0 and got[1] == np.inf and want[0] == 0.0
            assert abs(got[2] - want[2]) <= 1e-12
        else:
            assert np.allclose(got, want, rtol=0, atol=1e-12), (got, want)


def test_reference_small_images():
    rng = np.random.default_rng(5)
    for H, W in ((10, 40), (40, 10), (1, 1)):
        p, t = rng.uniform(-1, 1, (H, W)), rng.uniform(-1, 1, (H, W))
        for got in (reference(p, t), emulate32(p, t, True), emulate32(p, t, False)):
            mse = np.mean((p / 2 - t / 2) ** 2)
            assert abs(got[0] - np.sqrt(mse)) < 1e-6 and abs(got[1] - 10 * np.log10(1 / mse)) < 1e-3 and np.isnan(got[2])


def test_reduction_order_of_the_emulation():
    """_reduce32 against a literal restatement: thread i owns pixels i, i + 16384, ...; butterfly; (w0 + w1) + (w2 + w3); fp64 over 64"""
    rng = np.random.default_rng(6)
    v = rng.uniform(0, 1, 129 * 128).astype(np.float32)
    acc = np.zeros(GRID, dtype=np.float32)
    for i in range(v.size):
        acc[i % GRID] = np.float32(acc[i % GRID] + v[i])
    tot = 0.0
    for wg in range(64):
        waves = []
        for w in range(4):
            lanes = acc[wg * 256 + w * 64: wg * 256 + w * 64 + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                lanes = np.array([np.float32(lanes[k] + lanes[k ^ o]) for k in range(64)], dtype=np.float32)
            assert (lanes == lanes[0]).all()
            waves.append(lanes[0])
        tot += float(np.float32(np.float32(waves[0] + waves[1]) + np.float32(waves[2] + waves[3])))
    assert _reduce32(v) == tot
    assert abs(tot - v.astype(np.float64).sum()) < 1e-2


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_centred_emulation_and_the_witness(row):
    p, t = make(row)
    for b in sorted({0, row["B"] - 1}):
        ref = reference(p[b], t[b])
        cen, raw = emulate32(p[b], t[b], True), emulate32(p[b], t[b], False)
        bound, e_row = ssim_bound(p[b], t[b])
        assert bound >= SSIM_FLOOR and e_row <= 1e-6, (bound, e_row)  # the centred form itself stays at fp32 rounding level
        for em in (cen, raw):
            if row["kind"] in ("const", "same"):
                assert em[0] == 0.0 and em[1] == np.inf
            else:
                assert abs(em[0] - ref[0]) < 1e-6 and abs(em[1] - ref[1]) < 1e-3, (em, ref)
        if row["kind"] in ("const", "same"):
            assert abs(cen[2] - 1.0) <= 2.0 ** -23
        if row["kind"] == "neg":
            assert ref[2] < 0 and cen[2] < 0
        if row["dagger"]:
            miss = abs(raw[2] - ref[2])
            assert miss >= 10 * bound, (row["id"], miss, bound, e_row)
