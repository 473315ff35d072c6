"""No-reference despeckling statistics on the device (idiff_despeckle_stats through the C ABI and through ops): counts and the outside
count exactly against the numpy emulation of the contract (tests/despeckle_stats_ref.py), the fp64 sums within the bound of two fp64 sums
and bit for bit where every partial sum is exact; the image geometry (line, plane and sweep borders of the stencil), invalid pixels and
their neighbours, labels of the centre against labels of the neighbours, the ratio floor, independence of the batch, the members and the
run, the refusals, and the driftSDE / model / testUM surface."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import despeckle_stats_ref as ref  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import despeckle_summary, homogeneous_cells  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
# one float4; two lines of two; the smallest with a stencil pixel ... none (W = 4: no interior column); one interior line of two float4;
# three float4 per line; odd line count, five float4 per line; the surface's image; 65 float4 per line, more than one block; 224^2; and
# 66 560 pixels = 16 640 float4 against 16 384 per sweep: a second sweep whose first line has its N neighbour in the first sweep
SIZES = [(1, 4), (2, 8), (3, 4), (3, 8), (5, 12), (17, 20), (48, 48), (64, 260), (224, 224), (260, 256)]
UNIT = dict(scale=1.0, shift=0.0)


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run(x, y, labels, L, **kw):
    """x [B, S, P, H, W], y [B, P, H, W], labels [B, P, H, W] or [P, H, W] on the host -> (sums [B, S, L, 12], counts [B, S, L, 4],
    outside [B]) as numpy"""
    sums, counts, outside = ops.despeckle_stats(*dev(x, y, labels), L, **kw)
    B, S = x.shape[:2]
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (B, S, L, 12)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, S, L, 4)
    assert outside.dtype == torch.int32 and tuple(outside.shape) == (B,)
    return sums.cpu().numpy(), counts.cpu().numpy(), outside.cpu().numpy()


def bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(got, want):
    return all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))


def check_row(em, n_pix, sums, counts, outside, what, exact=False):
    """one row's device results against its emulation (ref.group's dict) -> the worst |sum - host| / bound"""
    assert counts.tolist() == em["counts"].tolist(), what
    assert int(outside) == em["outside"], what
    assert int(counts[:, [0, 3]].sum()) + int(outside) == n_pix, what  # sum_l (valid + invalid) + outside = P H W
    worst = 0.0
    for l in range(sums.shape[0]):
        for q in range(12):
            g, w, n = float(sums[l, q]), float(em["sums"][l, q]), int(em["n"][l, ref.NEED[q]])
            if n == 0:
                assert g == 0.0 and not np.signbit(g), (what, l, q, g)  # nothing counted: the sum is the +0.0 it started from
            elif exact:
                assert np.float64(g).view(np.int64) == np.float64(w).view(np.int64), (what, l, q, g, w)
            elif not np.isfinite(w):
                assert ref.same(g, w), (what, l, q, g, w)
            else:
                bound = ref.sum_bound(n, float(em["abs"][l, q]))
                assert abs(g - w) <= bound, (what, l, q, g, w, bound)
                worst = max(worst, abs(g - w) / bound if bound else 0.0)
    return worst


@functools.lru_cache(maxsize=None)
def rows(P, H, W, B=2, S=3):
    """(x [B, S, P, H, W], y [B, P, H, W], the per-pixel terms of every row) on the host, shared and never modified: speckled scenes and
    their restorations, with a NaN in member 0 of image 0 and an inf in the reference of image 1 where the plane has room for them"""
    xs, ys = [], []
    for b in range(B):
        drawn = [ref.draw(P, H, W, seed=1000 * b + 10 * s + H + W) for s in range(S)]
        xs.append(np.stack([d[0] for d in drawn]))
        ys.append(drawn[0][1])
    x, y = np.stack(xs), np.stack(ys)
    if H * W >= 16:
        x[0, 0, 0, H // 2, W // 2] = NAN
        y[1, P - 1, H - 1, W - 2] = INF
    terms = [[ref.pixel_terms(x[b, s], y[b]) for s in range(S)] for b in range(B)]
    return x, y, terms


# ---- 1. sizes, members, regions, maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_against_the_emulation(H, W):
    """B = 2, S in {1, 3}, L in {1, 3, 64}, a map per image and a shared one; P = 2 at 5 x 12 (no stencil may reach into the next
    plane); H <= 2 leaves no stencil pixel and untouched stencil sums"""
    P = 2 if (H, W) == (5, 12) else 1
    x, y, terms = rows(P, H, W)
    worst = 0.0
    for L in (1, 3, 64):
        maps = np.stack([ref.labels_blocks(P, H, W, L, seed=L), ref.labels_outside(P, H, W, L, seed=L + 1)])
        em = {(b, s, m): ref.group(terms[b][s], maps[m], L) for b in range(2) for s in range(3) for m in {b, 0}}
        for S in (1, 3):
            for shared in (False, True):
                sums, counts, outside = run(x[:, :S], y, maps[0] if shared else maps, L)
                for b in range(2):
                    for s in range(S):
                        what = f"{H}x{W} P={P} L={L} S={S} shared={shared} row ({b}, {s})"
                        worst = max(worst, check_row(em[(b, s, 0 if shared else b)], P * H * W, sums[b, s], counts[b, s], outside[b], what))
                        if H <= 2:
                            assert not counts[b, s, :, 2].any() and not bits(sums[b, s, :, 7:]).any(), what
    print(f"{H}x{W}: worst |sum - host| / bound {worst:.3f}")


def test_the_stencil_stays_inside_its_plane_and_crosses_sweeps():
    """by hand, without the emulation's masks: P = 2 at 5 x 12, every stencil pixel is an interior pixel of its own plane and La is the
    float64 Laplacian of that plane within the fp32 rounding; at 260 x 256 line 256 (float4 16 384: the second sweep's first) has its N
    neighbour in the first sweep and keeps its 254 stencil pixels"""
    x, y, _ = rows(2, 5, 12)
    labels = np.zeros((2, 5, 12), dtype=np.uint8)
    labels[1] = 1
    sums, counts, _ = run(x[:1, 1:2], y[:1], labels, 2)  # member 1 of image 0: no spoiled pixel
    a = x[0, 1].astype(np.float64) * 0.5 + 0.5
    for p in range(2):
        lap = a[p, :-2, 1:-1] + a[p, 2:, 1:-1] + a[p, 1:-1, :-2] + a[p, 1:-1, 2:] - 4 * a[p, 1:-1, 1:-1]
        assert counts[0, 0, p, 2] == 3 * 10
        assert abs(sums[0, 0, p, 7] - lap.sum()) <= 30 * 2.0 ** -19 and abs(sums[0, 0, p, 9] - (lap * lap).sum()) <= 30 * 2.0 ** -16
    H, W = 260, 256
    x, y, _ = rows(1, H, W)
    labels = np.full((1, H, W), 255, dtype=np.uint8)
    labels[0, 256] = 0  # the second sweep's first line
    labels[0, 255] = 1  # the first sweep's last line: its S neighbour is in the second sweep
    sums, counts, outside = run(x[1:, 1:2], y[1:], labels, 2)
    a = x[1, 1, 0].astype(np.float64) * 0.5 + 0.5
    assert outside.tolist() == [(H - 2) * W]
    for l, r in ((0, 256), (1, 255)):
        lap = a[r - 1, 1:-1] + a[r + 1, 1:-1] + a[r, :-2] + a[r, 2:] - 4 * a[r, 1:-1]
        assert counts[0, 0, l].tolist() == [W, W, W - 2, 0]
        assert abs(sums[0, 0, l, 7] - lap.sum()) <= (W - 2) * 2.0 ** -19


# ---- 2. invalid pixels ---------------------------------------------------------------------------------------------------------------
def test_an_invalid_pixel_removes_itself_and_its_four_neighbours_stencils():
    """5 x 8, a NaN in x at (2, 2) and an inf in ref at (2, 5): each removes its own pixel and the stencil terms of exactly its four
    neighbours; the eight diagonal neighbours are the stencil pixels left, with the Laplacians of the unspoiled image"""
    rng = np.random.default_rng(3)
    x = rng.uniform(0.1, 1.0, (1, 5, 8)).astype(np.float32)
    y = rng.uniform(0.1, 1.0, (1, 5, 8)).astype(np.float32)
    clean = ref.pixel_terms(x, y, **UNIT)
    xb, yb = x.copy(), y.copy()
    xb[0, 2, 2] = NAN
    yb[0, 2, 5] = INF
    labels = np.zeros((1, 5, 8), dtype=np.uint8)
    sums, counts, outside = run(xb[None, None], yb[None], labels, 1, **UNIT)
    assert counts[0, 0, 0].tolist() == [38, 38, 8, 2] and outside.tolist() == [0]
    left = np.zeros((1, 5, 8), dtype=bool)
    for r, c in [(1, 1), (1, 3), (3, 1), (3, 3), (1, 4), (1, 6), (3, 4), (3, 6)]:
        left[0, r, c] = True
    la, ly = clean["la"].astype(np.float64)[left], clean["ly"].astype(np.float64)[left]
    for q, t in ((7, la), (8, ly), (9, la * la), (10, ly * ly), (11, la * ly)):
        assert abs(sums[0, 0, 0, q] - t.sum()) <= ref.sum_bound(8, float(np.abs(t).sum())), q
    ok = np.ones((1, 5, 8), dtype=bool)
    ok[0, 2, 2] = ok[0, 2, 5] = False
    assert abs(sums[0, 0, 0, 0] - x.astype(np.float64)[ok].sum()) <= ref.sum_bound(38, 38.0)
    check_row(ref.emulate(xb, yb, labels, 1, **UNIT), 40, sums[0, 0], counts[0, 0], outside[0], "spoiled 5x8")
    # -inf and a NaN in the reference, an overflow of the affine map itself (x scale = inf), and every pixel invalid
    xb[0, 0, 0], yb[0, 4, 7], xb[0, 4, 0] = -INF, NAN, 3e38
    kw = dict(scale=4.0, shift=0.0)
    sums, counts, outside = run(xb[None, None], yb[None], labels, 1, **kw)
    em = ref.emulate(xb, yb, labels, 1, **kw)
    assert em["counts"][0, 3] == 5
    check_row(em, 40, sums[0, 0], counts[0, 0], outside[0], "spoiled 5x8, five kinds")
    sums, counts, outside = run(np.full((1, 1, 1, 5, 8), NAN, dtype=np.float32), yb[None], labels, 1)
    assert counts[0, 0, 0].tolist() == [0, 0, 0, 40] and not bits(sums).any()


# ---- 3. labels of the centre, not of the neighbours ----------------------------------------------------------------------------------
def test_a_stencil_term_goes_to_the_centres_region():
    """6 x 8 checkerboard: every neighbour of a pixel has the other label, and one interior pixel is 255: it lends its value to its four
    neighbours' stencils, adds to `outside` and nowhere else"""
    rng = np.random.default_rng(4)
    x = rng.uniform(0.1, 1.0, (1, 6, 8)).astype(np.float32)
    y = rng.uniform(0.1, 1.0, (1, 6, 8)).astype(np.float32)
    labels = ref.labels_checker(1, 6, 8)
    labels[0, 2, 3] = 255
    sums, counts, outside = run(x[None, None], y[None], labels, 2, **UNIT)
    check_row(ref.emulate(x, y, labels, 2, **UNIT), 48, sums[0, 0], counts[0, 0], outside[0], "checkerboard")
    assert outside.tolist() == [1] and int(counts[0, 0, :, 0].sum()) == 47 and int(counts[0, 0, :, 2].sum()) == 4 * 6 - 1
    a = x[0].astype(np.float64)
    lap = np.zeros((6, 8))
    lap[1:-1, 1:-1] = a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] - 4 * a[1:-1, 1:-1]  # of the whole image, labels unseen
    inner = np.zeros((6, 8), dtype=bool)
    inner[1:-1, 1:-1] = True
    for l in (0, 1):
        sel = inner & (labels[0] == l)
        assert counts[0, 0, l, 2] == int(sel.sum())
        assert abs(sums[0, 0, l, 7] - lap[sel].sum()) <= sel.sum() * 2.0 ** -19
    # the same image with the 255 pixel's value changed: its own sums are nowhere, its neighbours' Laplacians move
    x2 = x.copy()
    x2[0, 2, 3] += 0.25
    sums2, counts2, _ = run(x2[None, None], y[None], labels, 2, **UNIT)
    assert np.array_equal(counts2, counts) and np.array_equal(bits(sums2[..., :7]), bits(sums[..., :7]))
    moved = sums2[0, 0, :, 7] - sums[0, 0, :, 7]  # (2, 3) would carry label 1: its neighbours carry 0 and each gains 0.25
    assert abs(moved[0] - 4 * 0.25) <= 2.0 ** -19 * 4 and moved[1] == 0.0


# ---- 4. the ratio floor --------------------------------------------------------------------------------------------------------------
def test_pixels_below_the_floor_are_valid_but_not_in_the_ratio():
    x = np.full((1, 3, 8), 0.75, dtype=np.float32)
    low = [0.0, -0.0, -0.5, 2.0 ** -9, np.nextafter(np.float32(2.0 ** -8), np.float32(0)), 1e-30, 1e-45, -1e-45]
    x[0, 1, :] = low
    x[0, 0, 0] = 2.0 ** -8  # at the floor: counted
    y = np.full((1, 3, 8), 0.5, dtype=np.float32)
    labels = np.zeros((1, 3, 8), dtype=np.uint8)
    sums, counts, outside = run(x[None, None], y[None], labels, 1, **UNIT)
    assert counts[0, 0, 0].tolist() == [24, 16, 6, 0]
    # 128 and 15 quotients of one fp32 value: every partial sum is exact in fp64
    assert np.isfinite(sums).all() and sums[0, 0, 0, 5] == 128.0 + 15 * float(np.float32(0.5) / np.float32(0.75))
    check_row(ref.emulate(x, y, labels, 1, **UNIT), 24, sums[0, 0], counts[0, 0], outside[0], "floor")
    # a lower floor lets 2^-9, the value under 2^-8 and 1e-30 in (rho = 5e29, rho^2 = 2.5e59: finite in fp64); 0, the negatives and the
    # denormal stay out
    sums, counts, outside = run(x[None, None], y[None], labels, 1, ratio_floor=1e-37, **UNIT)
    assert counts[0, 0, 0].tolist() == [24, 19, 6, 0] and np.isfinite(sums).all()
    check_row(ref.emulate(x, y, labels, 1, floor=1e-37, **UNIT), 24, sums[0, 0], counts[0, 0], outside[0], "low floor")


# ---- 5. exact populations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,H,W,L", [(1, 12, 12, 1), (2, 5, 12, 3), (1, 64, 260, 3), (1, 260, 256, 64)])
def test_sums_are_bit_equal_where_every_partial_sum_is_exact(P, H, W, L):
    """scale = 1, shift = 0, x integers in 1 .. 8 and ref = x * {1, 2, 4}: a, y, rho, La, Ly are small integers, every term an integer and
    every partial sum exact in any order; ref.every_partial_sum_is_exact states the sufficient condition per region and quantity"""
    x, y = ref.draw_integers(P, H, W, seed=H)
    for name in ("blocks", "random"):
        labels = (ref.labels_blocks if name == "blocks" else ref.labels_random)(P, H, W, L, seed=W)
        em = ref.emulate(x, y, labels, L, **UNIT)
        for q in range(12):
            for l in range(L):
                assert ref.every_partial_sum_is_exact(em["terms"][q][(labels == l) & em["masks"][ref.NEED[q]]]), (name, l, q)
        assert np.array_equal(em["sums"], np.round(em["sums"])) and em["counts"][:, 1].sum() == P * H * W
        sums, counts, outside = run(x[None, None], y[None], labels[None], L, **UNIT)
        check_row(em, P * H * W, sums[0, 0], counts[0, 0], outside[0], f"exact {P}x{H}x{W} L={L} {name}", exact=True)


# ---- 6. independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(17, 20), (260, 256)])
def test_a_row_depends_on_neither_the_batch_the_members_nor_the_run(H, W):
    L = 5
    x, y, _ = rows(1, H, W)
    labels = np.stack([ref.labels_outside(1, H, W, L, seed=b) for b in range(2)])
    first, again = run(x, y, labels, L), run(x, y, labels, L)
    assert same_bits(first, again)
    for b in range(2):
        for s in range(3):
            alone = run(x[b:b + 1, s:s + 1], y[b:b + 1], labels[b:b + 1], L)  # the member alone: B = S = 1
            assert np.array_equal(bits(alone[0][0, 0]), bits(first[0][b, s])) and np.array_equal(alone[1][0, 0], first[1][b, s]), (b, s)
            assert alone[2][0] == first[2][b]
    swapped = run(x[::-1], y[::-1], labels[::-1], L)  # another place in the batch
    assert same_bits([t[::-1] for t in swapped], first)
    pair = run(x[:, 1:], y, labels, L)  # another place among the members
    assert np.array_equal(bits(pair[0]), bits(first[0][:, 1:])) and np.array_equal(pair[1], first[1][:, 1:])


def test_a_shared_map_is_the_map_repeated():
    H, W, L = 48, 48, 7
    x, y, _ = rows(1, H, W)
    labels = ref.labels_outside(1, H, W, L, seed=9)
    assert same_bits(run(x, y, labels, L), run(x, y, np.stack([labels] * 2), L))
    xd, yd, ld = dev(x, y, labels)
    one = ops.despeckle_stats(xd[:, 0].contiguous(), yd, ld, L)  # [B, C, H, W] against [B, C, H, W]: S = 1
    assert tuple(one[0].shape) == (2, 1, L, 12) and torch.equal(one[1][:, 0], ops.despeckle_stats(xd, yd, ld, L)[1][:, 0])


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, S, L, P, H, W = 2, 3, 8, 1, 4, 8
    n = P * H * W
    x = torch.randn(B * S * n + 8, device=DEV)
    y = torch.randn(B * n + 8, device=DEV)
    lab = torch.zeros(B * n + 16, device=DEV, dtype=torch.uint8)
    held = [t.clone() for t in (x, y, lab)]
    canary = dict(sums=torch.full((B * S * 64 * 12 + 2,), 7.0, device=DEV, dtype=torch.float64),
                  counts=torch.full((B * S * 64 * 4 + 2,), 7, device=DEV, dtype=torch.int32),
                  outside=torch.full((B + 2,), 7, device=DEV, dtype=torch.int32),
                  ws=torch.full((int(lib.idiff_despeckle_stats_ws_bytes(B, S, 64)) // 8 + 1,), 7.0, device=DEV, dtype=torch.float64))
    xp, yp, lp = x.data_ptr(), y.data_ptr(), lab.data_ptr()
    ptr = {k: t.data_ptr() for k, t in canary.items()}

    def call(xp=xp, yp=yp, lp=lp, bstride=n, L=L, scale=0.5, shift=0.5, floor=2.0 ** -8, sums=ptr["sums"], counts=ptr["counts"],
             outside=ptr["outside"], ws=ptr["ws"], B=B, S=S, P=P, H=H, W=W):
        return lib.idiff_despeckle_stats(xp, yp, lp, bstride, L, scale, shift, floor, sums, counts, outside, ws, B, S, P, H, W, None)

    refused = {
        "no x": dict(xp=None), "no ref": dict(yp=None), "no labels": dict(lp=None), "no sums": dict(sums=None), "no counts": dict(counts=None),
        "no outside": dict(outside=None), "no ws": dict(ws=None),
        "W = 6": dict(W=6, bstride=24), "W = 2": dict(W=2, bstride=8), "W = 0": dict(W=0, bstride=0), "H = 0": dict(H=0, bstride=0),
        "P = 0": dict(P=0, bstride=0), "P H W = 2^31": dict(P=32768, H=16384, W=4, B=1, S=1, bstride=0),
        "L = 0": dict(L=0), "L = 65": dict(L=65), "S = 0": dict(S=0), "S = 65": dict(S=65, B=1, H=1, W=4, bstride=4),
        "B = 0": dict(B=0), "B S = 65536": dict(B=16384, S=4, H=1, W=4, bstride=0),
        "floor = 0": dict(floor=0.0), "floor < 0": dict(floor=-1.0), "floor NaN": dict(floor=NAN), "floor inf": dict(floor=INF),
        "scale NaN": dict(scale=NAN), "scale inf": dict(scale=INF), "shift NaN": dict(shift=NAN), "shift -inf": dict(shift=-INF),
        "misaligned x": dict(xp=xp + 4), "misaligned ref": dict(yp=yp + 8), "misaligned labels": dict(lp=lp + 2),
        "misaligned ws": dict(ws=ptr["ws"] + 4), "misaligned sums": dict(sums=ptr["sums"] + 4), "misaligned counts": dict(counts=ptr["counts"] + 2),
        "labels_bstride = 16": dict(bstride=16), "labels_bstride = -32": dict(bstride=-32),
        "sums inside ws": dict(sums=ptr["ws"] + 64), "outside inside counts": dict(outside=ptr["counts"] + 8),
        "counts on ref": dict(counts=yp), "outside on labels": dict(outside=lp), "sums on x": dict(sums=xp + 16),
    }
    for what, kw in refused.items():
        n0 = ops.launch_count()
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert "despeckle_stats" in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert all(torch.equal(a, b) for a, b in zip((x, y, lab), held)), what
    xi, yi = torch.zeros(1, 2, 1, 4, 8, device=DEV), torch.zeros(1, 1, 4, 8, device=DEV)
    li = torch.zeros(1, 1, 4, 8, device=DEV, dtype=torch.uint8)
    for bad in (lambda: ops.despeckle_stats(torch.zeros(1, 1, 4, 6, device=DEV), torch.zeros(1, 1, 4, 6, device=DEV),
                                            torch.zeros(1, 4, 6, device=DEV, dtype=torch.uint8), 2),  # W % 4
                lambda: ops.despeckle_stats(xi, yi, li, 65), lambda: ops.despeckle_stats(xi, yi, li, 0),
                lambda: ops.despeckle_stats(xi, yi, li.to(torch.int32), 2), lambda: ops.despeckle_stats(xi.cpu(), yi.cpu(), li.cpu(), 2),
                lambda: ops.despeckle_stats(torch.zeros(1, 65, 1, 4, 8, device=DEV), yi, li, 2),
                lambda: ops.despeckle_stats(xi, yi, li, 2, ratio_floor=0.0), lambda: ops.despeckle_stats(xi, yi, li, 2, scale=NAN)):
        with pytest.raises(_lib.IdiffError):
            bad()
    with pytest.raises(AssertionError):
        ops.despeckle_stats(xi, yi, torch.zeros(4, 8, device=DEV, dtype=torch.uint8), 2)
    n0 = ops.launch_count()
    assert call() == 0  # the same buffers are accepted as they stand
    torch.cuda.synchronize()
    assert ops.launch_count() == n0 + 2
    got = canary["counts"][:B * S * L * 4].view(B, S, L, 4)
    assert got[:, :, 0, 0].sum().item() + got[:, :, 0, 3].sum().item() == B * S * n and canary["outside"][:B].tolist() == [0, 0]
    assert bool((canary["counts"][B * S * L * 4:] == 7).all()) and bool((canary["sums"][B * S * L * 12:] == 7).all())
    assert canary["outside"][B:].tolist() == [7, 7]


# ---- 8. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, HW = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=2, num_samples=4, interval=0.5))
    model.set_eval()
    return model, sde


def test_model_despeckle_stats(built):
    model, sde = built
    model.feed_data(make_batch(2, HW, seed=3))
    model.test(return_samples=True)
    assert model.samples.shape == (2, 4, 1, HW, HW) and model.output_median is not None
    grid = ops.grid_labels(HW, HW, 4, 4, DEV)
    host_grid = grid.cpu().numpy()[None]
    refs = dict(input=model.input.cpu().numpy(), target=model.target.cpu().numpy())
    held = dict(ensemble=model.samples.cpu().numpy(), output=model.output.cpu().numpy()[:, None], median=model.output_median.cpu().numpy()[:, None])
    for what, S in (("ensemble", 4), ("output", 1), ("median", 1)):
        for against in ("input", "target"):
            n0 = ops.launch_count()
            sums, counts, outside = model.despeckle_stats(grid, 16, what=what, against=against)
            assert ops.launch_count() == n0 + 2  # the two launches of ops.despeckle_stats and nothing else
            assert tuple(sums.shape) == (2, S, 16, 12) and tuple(counts.shape) == (2, S, 16, 4)
            for b in range(2):
                for s in range(S):
                    em = ref.emulate(held[what][b, s], refs[against][b], host_grid, 16)
                    check_row(em, HW * HW, sums[b, s].cpu().numpy(), counts[b, s].cpu().numpy(), outside[b].cpu().numpy(), f"model {what} {against}")
            record = despeckle_summary(sums, counts, outside)
            assert record["shape"] == [2, S] and record["outside"] == 0 and sum(r["N_PIX"] for r in record["regions"]) == 2 * S * HW * HW
            assert all(r["defined"]["ENL"] == 2 * S and r["defined"]["EPI"] == 2 * S for r in record["regions"])
            cells = homogeneous_cells(sums, counts)
            assert [len(c) for c in cells["cells"]] == [4] * (2 * S) and all(e is not None for e in cells["ENL_AUTO"])
    # the mean of four draws is smoother than a draw: its Laplacian energy against the input is lower than the members' mean
    members = despeckle_summary(*model.despeckle_stats(grid, 16, what="ensemble"))
    mean = despeckle_summary(*model.despeckle_stats(grid, 16, what="output"))
    lap = lambda rec: np.mean([q["LAP_RATIO"] for row in rec["rows"] for q in row])  # noqa: E731
    assert lap(mean) < lap(members)
    direct = sde.despeckle_stats(model.samples, model.input, grid[None].contiguous(), 16)
    via = model.despeckle_stats(grid, 16)
    assert torch.equal(direct[0].view(torch.int64), via[0].view(torch.int64)) and torch.equal(direct[1], via[1])
    with pytest.raises(ValueError, match="what must be"):
        model.despeckle_stats(grid, 16, what="mean")
    with pytest.raises(ValueError, match="against must be"):
        model.despeckle_stats(grid, 16, against="truth")
    with pytest.raises(ValueError, match="uint8"):
        model.despeckle_stats(grid.to(torch.int32), 16)
    with pytest.raises(ValueError):
        sde.despeckle_stats(model.samples, model.input, grid[:, :16].contiguous(), 16)
    model.test()  # the members are not kept
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.despeckle_stats(grid, 16)
    assert model.despeckle_stats(grid, 16, what="output")[1].shape == (2, 1, 16, 4)


NEW_WORDS = ("ENL=", "SSI=", "MEAN_RATIO", "VAR_RATIO", "EPI_in", "EPI_gt", "LAP_RATIO", "speckle (")  # "speckle in OCT" is an artifact type


def run_testum(tmp_path, capsys, name, extra, common):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {HW}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", f"name: {name}").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / f"{name}.yml"
    cfg.write_text(txt)
    torch.manual_seed(0)  # --random-init draws the weights from the global generator: the same nets in every run of this test
    res = testUM.main(["-opt", str(cfg), "--random-init", "--limit", "2", "--sample-T", "2"] + common + extra)
    return res, capsys.readouterr().out.replace(str(tmp_path), "")


@pytest.mark.parametrize("common", [[], ["--num-samples", "4"]], ids=["plain", "ensemble"])
def test_testum_speckle_option(tmp_path, capsys, common):
    S = 4 if common else 1
    plain, plain_out = run_testum(tmp_path, capsys, "drv_plain", [], common)
    for word in NEW_WORDS:
        assert word not in plain_out, word
    plain_lines = [ln for ln in plain_out.splitlines() if ln.startswith(" Testing ")]
    assert len(plain_lines) == 2
    res, out = run_testum(tmp_path, capsys, "drv_speckle", ["--speckle", "--speckle-background", "3"], common)  # the default: grid:8x8
    lines = [ln for ln in out.splitlines() if ln.startswith(" Testing ")]
    words = ["ENL_AUTO=", "SSI=", "MEAN_RATIO=", "VAR_RATIO=", "EPI_in=", "EPI_gt="] + (["ENL_member=", "LAP_RATIO=", "LAP_RATIO_member="] if S > 1 else [])
    # the image's line is the plain run's with the statistics appended; every other file is byte for byte the plain run's
    for ln, before in zip(lines, plain_lines):
        assert ln.startswith(before + ", ENL=") and all(w in ln[len(before):] for w in words) and "None" not in ln[len(before):], ln
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2 and "speckle (grid:8x8) over" in out
    speckle = testUM.parse_speckle("grid:8x8", None, 3)
    for kind, v in done.items():
        folder, plain_folder = tmp_path / "results" / "drv_speckle" / kind, tmp_path / "results" / "drv_plain" / kind
        assert sorted(os.listdir(folder)) == sorted(os.listdir(plain_folder) + ["speckle.json"])
        for f in os.listdir(plain_folder):
            assert open(folder / f, "rb").read() == open(plain_folder / f, "rb").read(), f
        assert set(v) == set(plain[kind]) | {"speckle", "pooled_speckle"}
        wrote = json.load(open(folder / "speckle.json"))
        assert wrote["spec"] == "grid:8x8" and wrote["S"] == S and wrote["L"] == 64 and wrote["images"] == v['num'] and wrote["background"] == 3
        keys = ("input", "target") + (("members",) if S > 1 else ())
        assert all(k in wrote for k in keys) and ("members" in wrote) == (S > 1)
        for key in keys:  # speckle.json is despeckle_summary of the tensors the run returned
            tensors = [torch.cat([rec[key][q] for rec in v['speckle']]) for q in range(3)]
            assert tuple(tensors[0].shape) == (v['num'], S if key == "members" else 1, 64, 12)
            want = despeckle_summary(*tensors, speckle["names"], 3)
            assert wrote[key]["regions"] == json.loads(json.dumps(want["regions"])) and wrote[key]["outside"] == want["outside"] == 0
            assert sum(r["N_PIX"] for r in wrote[key]["regions"]) == tensors[0].shape[0] * tensors[0].shape[1] * HW * HW
            enl = [q["ENL"] for row in want["rows"] for q in row if q["ENL"] is not None]
            assert wrote[key]["ENL"] == sum(enl) / len(enl) or wrote[key]["ENL"] == pytest.approx(sum(enl) / len(enl), rel=1e-14)
            auto = homogeneous_cells(*tensors[:2])["ENL_AUTO"]
            assert wrote[key]["ENL_AUTO"] == pytest.approx(sum(auto) / len(auto), rel=1e-14)
            assert all(r["defined"]["CNR"] == tensors[0].shape[0] * tensors[0].shape[1] for r in wrote[key]["regions"])
        if S > 1:  # the mean image is smoother than its members
            assert wrote["input"]["LAP_RATIO"] < wrote["members"]["LAP_RATIO"]
