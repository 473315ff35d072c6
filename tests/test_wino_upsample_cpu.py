"""The rule behind the upsample form of conv_wino4_kernel (csrc/conv_wino4.hip, MODE 1): of the 36 positions of B^T d B of an
F(4x4,3x3) input tile, the 11 with u == 2 or v == 2 are exactly +0 when the source is a nearest x2 upsample, in every tile, border tiles
included -- and none of the other 25 is (pos_live / quad_live of csrc/wino_common.h, mirrored in wino_upsample_ref.py).  Checked by brute
force with a float32 restatement of the kernel's row fold and bt6 over every tile of padded x2 images.  No GPU, no library."""
import re
from pathlib import Path

import numpy as np
import pytest

from wino_upsample_ref import PF, PH, QUAD_TABLE, bt6, input_transform, pos, pos_live, quad_live, row_fold, upsampled_tiles

HEADER = Path(__file__).resolve().parents[1] / "instancediff_amd" / "csrc" / "wino_common.h"
SIZES = [(h, w) for h in (8, 10, 18) for w in (12, 16, 34)]  # Hin x Win: x2 images of whole and partial 16x32 patches
DEAD = {(u, v) for u in range(6) for v in range(6) if u == 2 or v == 2}


def _transforms():
    """V [tiles of every image, 6, 6] and the tiles themselves"""
    vs, ds = [], []
    for i, (h, w) in enumerate(SIZES):
        g = np.random.default_rng(100 + i)
        src = (g.standard_normal((h, w)) * 0.5 + (3.0 if i % 2 else 0.0)).astype(np.float32)
        d = upsampled_tiles(src)
        assert d.shape[:2] == (-(-2 * h // 16) * 4, -(-2 * w // 32) * 8)
        ds.append(d.reshape(-1, 6, 6))
        vs.append(input_transform(d).reshape(-1, 6, 6))
    return np.concatenate(vs), np.concatenate(ds)


@pytest.fixture(scope="module")
def transformed():
    return _transforms()


def test_tiles_of_an_upsampled_source_repeat_rows_and_columns(transformed):
    _, d = transformed
    assert np.array_equal(d[:, 1, :], d[:, 2, :]) and np.array_equal(d[:, 3, :], d[:, 4, :])
    assert np.array_equal(d[:, :, 1], d[:, :, 2]) and np.array_equal(d[:, :, 3], d[:, :, 4])
    assert not np.array_equal(d[:, 0, :], d[:, 1, :]) and not np.array_equal(d[:, 2, :], d[:, 3, :]) and not np.array_equal(d[:, 4, :], d[:, 5, :])


def test_always_zero_positions_are_exactly_the_dead_set(transformed):
    v, _ = transformed
    zero = {(u, w) for u in range(6) for w in range(6) if not v[:, u, w].any()}
    assert zero == DEAD and len(zero) == 11
    assert zero == {(u, w) for u in range(6) for w in range(6) if not pos_live(u, w)}
    for u, w in DEAD:  # +0, never -0: what an accumulator that starts from C = 0 holds
        assert not np.signbit(v[:, u, w]).any()


def test_every_live_position_is_nonzero_somewhere(transformed):
    v, _ = transformed
    live = [(u, w) for u in range(6) for w in range(6) if pos_live(u, w)]
    assert len(live) == 25
    for u, w in live:
        assert v[:, u, w].any(), (u, w)
        assert np.count_nonzero(v[:, u, w]) > v.shape[0] // 4, (u, w)  # and not by accident (the grid holds tiles outside the image)


def test_a_plain_source_has_no_dead_position():
    g = np.random.default_rng(7)
    v = input_transform(g.standard_normal((64, 6, 6)).astype(np.float32))
    assert all(v[:, u, w].any() for u in range(6) for w in range(6))
    assert all(pos_live(u, w, upsampled=False) for u in range(6) for w in range(6))
    assert all(quad_live(q, upsampled=False) == 0xf for q in range(9))


def test_restated_transforms_are_the_winograd_matrices():
    """row_fold and bt6 are B^T of F(4x4,3x3) with points 0, +-1, +-2, inf"""
    BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], np.float64)
    g = np.random.default_rng(3)
    d = g.integers(-8, 9, size=(5, 6, 6)).astype(np.float32)  # small integers: every step is exact
    assert np.array_equal(row_fold(d).astype(np.float64), np.einsum("ur,nrc->nuc", BT, d.astype(np.float64)))
    assert np.array_equal(bt6(d).astype(np.float64), np.einsum("vc,nrc->nrv", BT, d.astype(np.float64)))


def test_quad_masks_follow_pos():
    seen = set()
    for u in range(6):
        assert PF(u) == (0, 2, 3, 5, 6, 8)[u] and PH(u) == (1, 1, 4, 4, 7, 7)[u]
        for v in range(6):
            seen.add(pos(u, v))
    assert seen == set(range(36))  # pos() is a bijection onto 9 quads of 4
    for q in range(9):
        want = {pos(u, v) & 3 for u in range(6) for v in range(6) if pos(u, v) // 4 == q and (u, v) not in DEAD}
        assert {c for c in range(4) if quad_live(q) >> c & 1} == want == QUAD_TABLE[q], q
    assert sum(bin(quad_live(q)).count("1") for q in range(9)) == 25
    assert [q for q in range(9) if quad_live(q) == 0] == [3]  # the one quad whose operand reads go too


def test_mirror_matches_the_header():
    """the Python mirrors restate what csrc/wino_common.h defines"""
    text = HEADER.read_text()
    flat = re.sub(r"\s+", " ", text)
    assert "constexpr int PF(int u) { return (3 * u + 1) / 2; }" in flat
    assert "constexpr int PH(int u) { return 1 + 3 * (u / 2); }" in flat
    assert "constexpr int pos(int u, int v) { return v < 4 ? 4 * PF(u) + v : 4 * PH(u) + 2 * (u & 1) + (v - 4); }" in flat
    assert "constexpr bool pos_live(int u, int v) { return !UPSAMPLED || (u != 2 && v != 2); }" in flat
    assert "if (pos_live<UPSAMPLED>(u, v) && pos(u, v) / 4 == quad) m |= 1u << (pos(u, v) & 3);" in flat
