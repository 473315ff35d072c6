"""The 16-byte gather table of conv_wino4_kernel (wino_gather16_ref.py, a restatement of gather_decode16 of csrc/wino_common.h) against
brute force: for every patch of every geometry, every (channel, row, column) of the 4 x 18 x 34 patch with halo must sit at row float
3 + column of the R image the requests fill, holding that pixel of the image -- or 0.0 where the pixel lies outside it; every piece is
16-byte aligned, wholly inside one image row or refused whole; every slot is requested exactly once; the mask has one bit per slot."""
import pytest

from wino_gather16_ref import CK, ES, HEAVY_THREADS, NT, PSP, RCOLS, RS, SLOTS, TRH, lds_image, requests, table

TH, TW = 16, 32
# the issue's geometries (every patch of each: all four borders, corners, ragged right / bottom edges) and one with an interior patch
GEOMETRIES = [(H, W) for W in (24, 32, 40, 64) for H in (16, 20, 32)] + [(48, 96)]


def _patches(H, W):
    return [(y0, x0) for y0 in range(0, H, TH) for x0 in range(0, W, TW)]


def test_every_slot_is_requested_once():
    seen = sorted(tid + i * ES for tid in range(NT) for i in requests(tid))
    assert seen == list(range(SLOTS))
    assert sum(len(requests(t)) for t in range(NT)) == 3 * HEAVY_THREADS == SLOTS  # 12 wave-instructions of 64 slots


@pytest.mark.parametrize("H,W", GEOMETRIES, ids=[f"{h}x{w}" for h, w in GEOMETRIES])
def test_table_against_brute_force(H, W):
    assert W % 4 == 0 and H % 4 == 0 and W >= 24  # conv_wino4_items
    if (H, W) == (48, 96):
        assert (16, 32) in _patches(H, W)  # the interior patch: no halo element outside the image
    for y0, x0 in _patches(H, W):
        offs, masks = table(y0, x0, H, W)
        for (tid, i), off in offs.items():
            assert off == -1 or (off >= 0 and off % 16 == 0), (y0, x0, tid, i, off)
            if off >= 0:  # the piece lies inside ONE row of ONE channel plane
                f = off // 4
                assert f % W + 3 < W and f // (H * W) < CK
            assert (masks[tid] >> i) & 1 == (1 if off < 0 else 0)
        for tid in range(NT):
            assert masks[tid] >> len(requests(tid)) == 0
        R = lds_image(offs)
        assert sorted(R) == list(range(CK * PSP))
        outside = 0
        for ci in range(CK):
            for r in range(TRH):
                for c in range(RCOLS):
                    oy, ox = y0 - 1 + r, x0 - 1 + c
                    want = ci * H * W + oy * W + ox if (0 <= oy < H and 0 <= ox < W) else None
                    outside += want is None
                    assert R[ci * PSP + r * RS + 3 + c] == want, (H, W, y0, x0, ci, r, c)
        if (H, W, y0, x0) == (48, 96, 16, 32):
            assert outside == 0
        else:
            assert outside > 0  # every other patch of these geometries touches a border
