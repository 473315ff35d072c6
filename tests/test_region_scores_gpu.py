"""Region-wise ensemble scores on the device (idiff_region_scores / idiff_band_labels through the C ABI and through ops): counts and the
outside count exactly against the numpy emulation of the contract (tests/region_scores_ref.py), the fp64 sums within the bound of two
fp64 sums and bit for bit where every partial sum is exact, every label population the wave-level label set can trip on, the identities
against idiff_ensemble_scores, independence of the batch, of the run and of the form, the band labels bit for bit, the refusals, and the
driftSDE / model / testUM surface."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import region_scores_ref as ref  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import region_score_summary  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
# one float4; two; short of one 256-thread block; four blocks; a second sweep of the 64 x 256 grid with one live lane; the surface's image
N_S = [4, 8, 252, 1024, 4 * 64 * 256 + 4, 48 * 48]
S_ALL = [1, 2, 3, 4, 8, 16, 17, 33, 64]  # 16 | 17 straddles the register form
L_ALL = [1, 2, 3, 32, 33, 64]
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def values(S, n, kind, seed=0):
    """(x [S, n], y [n], the per-pixel record) on the host, shared and never modified.  kind: float (rounded terms), spoiled (NaN members,
    NaN targets and +-inf mixed in), int (integer-valued x and y in [-4, 4])"""
    if kind == "int":
        x, y = ref.draw_integers(S, n, 7000 + 100 * S + seed)
    else:
        x, y = ref.draw(S, n, 100 * S + n % 1000 + seed)
        if kind == "spoiled":
            x, y = ref.spoil(x, y, 5000 + S + seed)
    return x, y, ref.pixel_record(x, y)


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run(x, y, labels, L):
    """x [B, S, n], y [B, n], labels [B, n] or [n] on the host -> (sums [B, L, 4], counts [B, L, S + 2], outside [B]) as numpy"""
    sums, counts, outside = ops.region_scores(*dev(x, y, labels), L)
    B, S = x.shape[:2]
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (B, L, 4)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, L, S + 2)
    assert outside.dtype == torch.int32 and tuple(outside.shape) == (B,)
    return sums.cpu().numpy(), counts.cpu().numpy(), outside.cpu().numpy()


def check_image(em, n_s, sums, counts, outside, what, exact=False):
    """one image's device results against its emulation (ref.group's dict)"""
    assert counts.tolist() == em["counts"].tolist(), what
    assert int(outside) == em["outside"], what
    assert int(counts.sum()) + int(outside) == n_s, what  # sum_l (hist + invalid) + outside = n_s
    L = sums.shape[0]
    worst = 0.0
    for l in range(L):
        for q in range(4):
            g, w = float(sums[l, q]), float(em["sums"][l, q])
            if em["n"][l] == 0:
                assert g == 0.0 and not np.signbit(g), (what, l, q, g)  # an empty region's sums are +0.0
            elif exact:
                assert np.float64(g).view(np.int64) == np.float64(w).view(np.int64), (what, l, q, g, w)
            elif not np.isfinite(w):
                assert ref.same(g, w), (what, l, q, g, w)
            else:
                bound = ref.sum_bound(int(em["n"][l]), float(em["abs"][l, q]))
                assert abs(g - w) <= bound, (what, l, q, g, w, bound)
                worst = max(worst, abs(g - w) / bound if bound else 0.0)
    print(f"{what}: worst |sum - host| / bound {worst:.3f}")


def check_against_ensemble_scores(x, y, labels, L, counts):
    """sum_l counts[l] = idiff_ensemble_scores' counts on the pixels not outside (handed over as an image of their own: their number
    must be a multiple of 4)"""
    inside = labels < L
    if inside.sum() == 0 or inside.sum() % 4:
        return False
    _, whole, _ = ops.ensemble_scores(*dev(x[None][:, :, inside], y[None][:, inside]))
    assert whole[0].cpu().tolist() == counts.sum(axis=0).tolist()
    return True


# ---- 1. sizes and members ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
def test_against_the_emulation_over_sizes_and_members(n_s):
    """B = 2: coherent blobs over spoiled values, per-pixel random labels with outside ones over rounded values; image 1 alone bit for bit"""
    L = 3
    labels = np.stack([ref.labels_blobs(n_s, L, seed=n_s), ref.labels_outside(n_s, L, seed=n_s + 1)])
    for S in (S_ALL if n_s <= 48 * 48 else [1, 4, 17]):
        x0, y0, rec0 = values(S, n_s, "spoiled")
        x1, y1, rec1 = values(S, n_s, "float", seed=1)
        sums, counts, outside = run(np.stack([x0, x1]), np.stack([y0, y1]), labels, L)
        check_image(ref.group(rec0, labels[0], L, S), n_s, sums[0], counts[0], outside[0], f"n_s={n_s} S={S} blobs")
        check_image(ref.group(rec1, labels[1], L, S), n_s, sums[1], counts[1], outside[1], f"n_s={n_s} S={S} outside")
        s1, c1, o1 = run(x1[None], y1[None], labels[1:2], L)
        assert np.array_equal(s1[0].view(np.int64), sums[1].view(np.int64)) and np.array_equal(c1[0], counts[1]) and o1[0] == outside[1]


# ---- 2. label populations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.LABELS))
def test_label_populations(name):
    """every population at 252 pixels (one block has work) and at 48 x 48 (nine have), at every L, below and above the register form;
    spoiled values: NaN members, NaN targets and +-inf"""
    compared = 0
    for n_s in (252, 48 * 48):
        for L in L_ALL:
            labels = ref.LABELS[name](n_s, L, seed=L)
            for S in (2, 17):
                x, y, rec = values(S, n_s, "spoiled")
                em = ref.group(rec, labels, L, S)
                sums, counts, outside = run(x[None], y[None], labels[None], L)
                check_image(em, n_s, sums[0], counts[0], outside[0], f"{name} n_s={n_s} L={L} S={S}")
                compared += check_against_ensemble_scores(x, y, labels, L, counts[0])
                if name == "outside":
                    assert 0 < outside[0] < n_s and {int(L), 200, 255} & set(labels.tolist())
                else:
                    assert outside[0] == 0
                if name == "single" and L > 1:
                    assert int(counts[0, L - 1].sum()) == 1  # one element of one lane carries the label
                if name == "quad" and L >= 4:
                    assert all(len(set(labels[i:i + 4].tolist())) == 4 for i in range(0, n_s, 4))
                if name == "random" and L <= 3 and n_s == 48 * 48:
                    assert all(len(set(labels[i:i + 256].tolist())) == L for i in range(0, n_s, 256))  # every wave holds every label
    assert compared > 0


def test_a_region_of_invalid_pixels_only_and_an_image_of_them():
    n_s, L, S = 48 * 48, 4, 3
    x, y, _ = values(S, n_s, "float")
    labels = ref.labels_halves(n_s, L)
    labels[100:164] = 3  # region 3: 64 pixels, every one with a NaN target; region 2: no pixel at all
    y = y.copy()
    y[100:164] = NAN
    em = ref.emulate(x, y, labels, L)
    sums, counts, outside = run(x[None], y[None], labels[None], L)
    check_image(em, n_s, sums[0], counts[0], outside[0], "invalid region")
    assert counts[0, 3].tolist() == [0] * (S + 1) + [64] and not sums[0, 3].any() and not counts[0, 2].any() and not sums[0, 2].any()
    x = x.copy()
    x[1] = NAN  # no valid pixel anywhere
    sums, counts, outside = run(x[None], y[None], labels[None], L)
    assert not sums.any() and not np.signbit(sums).any() and not counts[0, :, :S + 1].any() and int(counts[0, :, S + 1].sum()) == n_s
    sums, counts, outside = run(x[None], y[None], np.full((1, n_s), 255, dtype=np.uint8), L)  # and no pixel in any region
    assert not sums.any() and not counts.any() and outside.tolist() == [n_s]


def test_a_shared_map_is_the_map_repeated():
    n_s, L, S, B = 1024, 5, 4, 3
    labels = ref.labels_outside(n_s, L, seed=9)
    xs, ys = zip(*(values(S, n_s, "spoiled", seed=b)[:2] for b in range(B)))
    x, y = np.stack(xs), np.stack(ys)
    shared = run(x, y, labels, L)
    repeated = run(x, y, np.stack([labels] * B), L)
    for a, b in zip(shared, repeated):
        assert np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32), b.view(np.int64 if b.dtype == np.float64 else np.int32))
    xd, yd, ld = dev(x, y, labels.reshape(32, 32))  # through ops with image-shaped tensors: [B, S, 32, 32], [B, 32, 32], [32, 32]
    got = ops.region_scores(xd.view(B, S, 32, 32), yd.view(B, 32, 32), ld, L)
    assert np.array_equal(got[0].cpu().numpy().view(np.int64), shared[0].view(np.int64)) and np.array_equal(got[1].cpu().numpy(), shared[1])
    one = ops.region_scores(xd[:, 0].contiguous(), yd, ld.view(-1), L)  # [B, n] against [B, n]: S = 1
    assert tuple(one[1].shape) == (B, L, 3)


def test_every_L_at_every_S():
    """per-pixel random labels with outside ones, 1024 pixels: every (L, S) of the lists, so every instantiation meets every LDS layout"""
    n_s = 1024
    for S in S_ALL:
        x, y, rec = values(S, n_s, "spoiled")
        for L in L_ALL:
            labels = ref.labels_outside(n_s, L, seed=L + S)
            sums, counts, outside = run(x[None], y[None], labels[None], L)
            check_image(ref.group(rec, labels, L, S), n_s, sums[0], counts[0], outside[0], f"S={S} L={L}")


# ---- 3. exact populations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_s", [(1, 4 * 64 * 256 + 4), (2, 4 * 64 * 256 + 4), (4, 48 * 48), (8, 1024), (16, 252), (64, 252)])
def test_sums_are_bit_equal_where_every_partial_sum_is_exact(S, n_s):
    """integer-valued x and y in [-4, 4], S a power of two: every d_s is an integer of magnitude <= 8, so a and g are integers, m is a
    multiple of 1/S, crps, e = m*m and the (d_s - m)^2 are multiples of 1/S^2 of small magnitude and exact in fp32, and m too.  v = ss /
    (S - 1) is exact for S <= 2 and a rounded fp32 value above that, which is why the rows are shorter there.  Whatever the terms are,
    ref.every_partial_sum_is_exact states the sufficient condition and the test asserts it per region and quantity before it compares
    bits: all terms are multiples of one power of two q and sum |t| < 2^53 q, so every partial sum in any order is exact."""
    L = 5
    x, y, rec = values(S, n_s, "int")
    assert rec["valid"].all()
    for name in ("blobs", "random", "quad"):
        labels = ref.LABELS[name](n_s, L, seed=S)
        for l in range(L):
            for q in ref.QUANT:
                assert ref.every_partial_sum_is_exact(rec[q][labels == l]), (name, l, q)
        sums, counts, outside = run(x[None], y[None], labels[None], L)
        check_image(ref.group(rec, labels, L, S), n_s, sums[0], counts[0], outside[0], f"exact S={S} n_s={n_s} {name}", exact=True)


# ---- 4. against idiff_ensemble_scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", [252, 48 * 48, 65536, 4 * 64 * 256 + 4])
def test_one_region_is_the_whole_image(n_s):
    """L = 1 and no outside label: the counts are idiff_ensemble_scores'; the three shared sums carry its bits while the image is one
    sweep (n_s <= 65536: the same terms in the same order), and are within the bound of two fp64 sums above that"""
    labels = np.zeros(n_s, dtype=np.uint8)
    for S in (1, 4, 16, 17):
        x, y, rec = values(S, n_s, "float")
        sums, counts, outside = run(x[None], y[None], labels[None], 1)
        whole_sums, whole_counts, _ = ops.ensemble_scores(*dev(x[None], y[None]))
        whole_sums, whole_counts = whole_sums.cpu().numpy(), whole_counts.cpu().numpy()
        assert np.array_equal(counts[0, 0], whole_counts[0]) and outside[0] == 0
        if n_s <= 65536:
            assert np.array_equal(sums[0, 0, :3].view(np.int64), whole_sums[0].view(np.int64)), (n_s, S)
        em = ref.group(rec, labels, 1, S)
        for q in range(3):
            assert abs(sums[0, 0, q] - whole_sums[0, q]) <= ref.sum_bound(n_s, em["abs"][0, q]), (n_s, S, q)


# ---- 5. independence -------------------------------------------------------------------------------------------------------------------
def test_an_image_does_not_depend_on_the_batch_or_the_run():
    n_s, L, S, B = 4 * 64 * 256 + 4, 6, 3, 5
    xs, ys = zip(*(values(S, n_s, "spoiled", seed=b)[:2] for b in range(B)))
    x, y = np.stack(xs), np.stack(ys)
    labels = np.stack([ref.LABELS[name](n_s, L, seed=b) for b, name in enumerate(["blobs", "random", "outside", "quad", "single"])])
    first, again = run(x, y, labels, L), run(x, y, labels, L)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32), b.view(np.int64 if b.dtype == np.float64 else np.int32))
    for b in range(B):
        s1, c1, o1 = run(x[b:b + 1], y[b:b + 1], labels[b:b + 1], L)
        assert np.array_equal(s1[0].view(np.int64), first[0][b].view(np.int64)), b
        assert np.array_equal(c1[0], first[1][b]) and o1[0] == first[2][b], b


@pytest.mark.parametrize("S", [1, 5, 12, 16])
def test_register_and_second_read_forms_agree(S, monkeypatch):
    n_s, L = 1028, 4
    x, y, _ = values(S, n_s, "spoiled")
    labels = ref.labels_outside(n_s, L, seed=S)
    monkeypatch.delenv("IDIFF_ENSEMBLE_REREAD", raising=False)
    reg = run(x[None], y[None], labels[None], L)
    monkeypatch.setenv("IDIFF_ENSEMBLE_REREAD", "1")
    rr = run(x[None], y[None], labels[None], L)
    # the spoiled values make some sums NaN (0 * inf, inf - inf): IEEE 754 leaves a NaN's sign and payload open, and the two forms reach
    # it through different instructions, so a NaN is compared as a NaN and every other sum bit for bit
    nan = np.isnan(reg[0])
    assert np.array_equal(nan, np.isnan(rr[0])) and np.array_equal(reg[0][~nan].view(np.int64), rr[0][~nan].view(np.int64))
    assert np.array_equal(reg[1], rr[1]) and np.array_equal(reg[2], rr[2])
    x, y, _ = values(S, n_s, "float")  # and NaN-free values: every bit
    monkeypatch.delenv("IDIFF_ENSEMBLE_REREAD")
    reg = run(x[None], y[None], labels[None], L)
    monkeypatch.setenv("IDIFF_ENSEMBLE_REREAD", "1")
    rr = run(x[None], y[None], labels[None], L)
    assert np.isfinite(reg[0]).all() and np.array_equal(reg[0].view(np.int64), rr[0].view(np.int64)) and np.array_equal(reg[1], rr[1])


# ---- 6. band labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 48 * 48, 256 * 16 * 3 + 5])
def test_band_labels_are_searchsorted_right(n):
    rng = np.random.default_rng(n)
    edges = np.array([-0.5, -1e-40, 0.0, 1e-45, 0.25, 0.75], dtype=np.float32)
    special = np.array([-0.5, np.nextafter(np.float32(-0.5), np.float32(-1)), -0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 0.25, 0.75, INF, -INF, NAN,
                        np.nextafter(np.float32(0.75), np.float32(0))], dtype=np.float32)
    y = rng.uniform(-1, 1, n).astype(np.float32)
    where = rng.random(n) < 0.5
    y[where] = special[rng.integers(0, len(special), int(where.sum()))]
    if n > len(special):
        y[:len(special)] = special
    want = np.searchsorted(edges, y, side="right").astype(np.uint8)
    want[np.isnan(y)] = 255
    yd = torch.from_numpy(y).to(DEV)
    got = ops.band_labels(yd, edges.tolist())
    assert got.dtype == torch.uint8 and got.shape == yd.shape and np.array_equal(got.cpu().numpy(), want)
    for ne in (1, 63):  # the limits of the edge table
        e = np.linspace(-0.9, 0.9, ne).astype(np.float32)
        want = np.searchsorted(e, y, side="right").astype(np.uint8)
        want[np.isnan(y)] = 255
        assert np.array_equal(ops.band_labels(yd, e.tolist()).cpu().numpy(), want), ne


def test_band_labels_feed_region_scores():
    """error by intensity band of the truth, end to end: three bands of a 48 x 48 image, per-image labels"""
    n_s, S, B = 48 * 48, 4, 2
    xs, ys = zip(*(values(S, n_s, "float", seed=b)[:2] for b in range(B)))
    x, y = np.stack(xs), np.stack(ys)
    xd, yd = dev(x, y)
    labels = ops.band_labels(yd, [-0.5, 0.0])
    assert tuple(labels.shape) == (B, n_s)
    sums, counts, outside = (t.cpu().numpy() for t in ops.region_scores(xd, yd, labels, 3))
    for b in range(B):
        host = np.searchsorted(np.array([-0.5, 0.0], dtype=np.float32), y[b], side="right").astype(np.uint8)
        check_image(ref.emulate(x[b], y[b], host, 3), n_s, sums[b], counts[b], outside[b], f"bands image {b}")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, S, L, n_s = 2, 4, 8, 64
    x = torch.randn(B * S * n_s + 8, device=DEV)
    y = torch.randn(B * n_s + 8, device=DEV)
    lab = torch.zeros(B * n_s + 16, device=DEV, dtype=torch.uint8)
    held = [t.clone() for t in (x, y, lab)]
    canary = dict(sums=torch.full((B, 64, 4), 7.0, device=DEV, dtype=torch.float64), counts=torch.full((B, 64, 66), 7, device=DEV, dtype=torch.int32),
                  outside=torch.full((B + 2,), 7, device=DEV, dtype=torch.int32),
                  ws=torch.full((int(lib.idiff_region_scores_ws_bytes(B, 64, 64)) // 8 + 1,), 7.0, device=DEV, dtype=torch.float64),
                  band=torch.full((256,), 7, device=DEV, dtype=torch.uint8))

    def call(xp, yp, lp, bstride=n_s, L_=L, S_=S, n=n_s, B_=B, sums=None, counts=None, outside=None, ws=None):
        return lib.idiff_region_scores(xp, yp, lp, bstride, L_, sums or canary["sums"].data_ptr(), counts or canary["counts"].data_ptr(),
                                       outside or canary["outside"].data_ptr(), ws or canary["ws"].data_ptr(), B_, S_, n, None)

    def band(yp, lp, n, edges, ne=None):
        arr = (ctypes.c_float * max(len(edges), 1))(*edges)
        return lib.idiff_band_labels(yp, lp, n, arr, len(edges) if ne is None else ne, None)

    xp, yp, lp, bp = x.data_ptr(), y.data_ptr(), lab.data_ptr(), canary["band"].data_ptr()
    refused = {
        "no x": lambda: call(None, yp, lp),
        "no target": lambda: call(xp, None, lp),
        "no labels": lambda: call(xp, yp, None),
        "no sums": lambda: lib.idiff_region_scores(xp, yp, lp, n_s, L, None, canary["counts"].data_ptr(), canary["outside"].data_ptr(),
                                                   canary["ws"].data_ptr(), B, S, n_s, None),
        "no outside": lambda: lib.idiff_region_scores(xp, yp, lp, n_s, L, canary["sums"].data_ptr(), canary["counts"].data_ptr(), None,
                                                      canary["ws"].data_ptr(), B, S, n_s, None),
        "S = 0": lambda: call(xp, yp, lp, S_=0),
        "S = 65": lambda: call(xp, yp, lp, S_=65, n=4),
        "L = 0": lambda: call(xp, yp, lp, L_=0),
        "L = 65": lambda: call(xp, yp, lp, L_=65),
        "n_s = 6": lambda: call(xp, yp, lp, bstride=6, n=6),
        "n_s = 0": lambda: call(xp, yp, lp, bstride=0, n=0),
        "B = 0": lambda: call(xp, yp, lp, B_=0),
        "B = 65536": lambda: call(xp, yp, lp, B_=65536, n=4, bstride=4),
        "misaligned x": lambda: call(xp + 4, yp, lp),
        "misaligned target": lambda: call(xp, yp + 8, lp),
        "misaligned labels": lambda: call(xp, yp, lp + 2),
        "misaligned ws": lambda: call(xp, yp, lp, ws=canary["ws"].data_ptr() + 4),
        "labels_bstride = 32": lambda: call(xp, yp, lp, bstride=32),
        "labels_bstride = -64": lambda: call(xp, yp, lp, bstride=-64),
        "sums inside ws": lambda: call(xp, yp, lp, sums=canary["ws"].data_ptr() + 64),
        "outside inside counts": lambda: call(xp, yp, lp, outside=canary["counts"].data_ptr() + 8),
        "counts on target": lambda: call(xp, yp, lp, counts=yp),
        "outside on labels": lambda: call(xp, yp, lp, outside=lp),
        "sums on x": lambda: call(xp, yp, lp, sums=xp + 16),
        "band: no y": lambda: band(None, bp, 64, [0.0]),
        "band: no labels": lambda: band(yp, None, 64, [0.0]),
        "band: n = 0": lambda: band(yp, bp, 0, [0.0]),
        "band: ne = 0": lambda: band(yp, bp, 64, [0.0], ne=0),
        "band: ne = 64": lambda: band(yp, bp, 64, [i / 64 for i in range(64)]),
        "band: unordered": lambda: band(yp, bp, 64, [0.0, 0.5, 0.25]),
        "band: equal edges": lambda: band(yp, bp, 64, [0.0, 0.5, 0.5]),
        "band: NaN edge": lambda: band(yp, bp, 64, [0.0, NAN]),
        "band: infinite edge": lambda: band(yp, bp, 64, [0.0, INF]),
        "band: misaligned y": lambda: band(yp + 4, bp, 64, [0.0]),
        "band: misaligned labels": lambda: band(yp, bp + 4, 64, [0.0]),
        "band: labels on y": lambda: band(yp, yp + 64, 64, [0.0]),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert ("band_labels" if what.startswith("band") else "region_scores") in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert all(torch.equal(a, b) for a, b in zip((x, y, lab), held)), what
    xi, yi = torch.zeros(1, 2, 8, device=DEV), torch.zeros(1, 8, device=DEV)
    li = torch.zeros(1, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(_lib.IdiffError):
        ops.region_scores(torch.zeros(1, 2, 5, 5, device=DEV), torch.zeros(1, 5, 5, device=DEV), torch.zeros(5, 5, device=DEV, dtype=torch.uint8), 2)
    with pytest.raises(_lib.IdiffError):
        ops.region_scores(xi, yi, li, 65)
    with pytest.raises(_lib.IdiffError):
        ops.region_scores(xi, yi, li.to(torch.int32), 2)  # labels are uint8
    with pytest.raises(_lib.IdiffError):
        ops.region_scores(xi.cpu(), yi.cpu(), li.cpu(), 2)  # host tensors
    with pytest.raises(_lib.IdiffError):
        ops.region_scores(torch.zeros(1, 65, 8, device=DEV), yi, li, 2)  # S = 65
    with pytest.raises(AssertionError):
        ops.region_scores(xi, yi, torch.zeros(4, device=DEV, dtype=torch.uint8), 2)
    with pytest.raises(_lib.IdiffError):
        ops.band_labels(yi, [])
    with pytest.raises(_lib.IdiffError):
        ops.band_labels(yi, [0.5, 0.25])
    n0 = ops.launch_count()
    assert call(xp, yp, lp) == 0  # the same buffers are accepted as they stand
    assert band(yp, bp, 64, [0.0]) == 0
    torch.cuda.synchronize()
    assert ops.launch_count() == n0 + 3
    assert canary["counts"].view(-1)[:B * L * (S + 2)].view(B, L, S + 2)[:, 0].sum().item() == B * n_s and canary["outside"][:B].tolist() == [0, 0]
    assert set(canary["band"][:64].tolist()) <= {0, 1} and bool((canary["band"][64:] == 7).all())


# ---- 8. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, H = 10, 48


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=2, num_samples=4, interval=0.5))
    model.set_eval()
    return model, sde


def test_model_region_scores(built):
    model, sde = built
    model.feed_data(make_batch(2, H, seed=3))
    model.test(return_samples=True)
    assert model.samples.shape == (2, 4, 1, H, H) and model.output_median is not None
    grid = ops.grid_labels(H, H, 2, 2, DEV)
    assert grid.device.type == "cuda" and tuple(grid.shape) == (H, H)
    bands = ops.band_labels(model.target, [-0.5, 0.0])
    tgt = model.target.flatten(1).cpu().numpy()
    held = dict(ensemble=model.samples.flatten(2).cpu().numpy(), output=model.output.flatten(1).cpu().numpy()[:, None],
                median=model.output_median.flatten(1).cpu().numpy()[:, None])
    for what, S in (("ensemble", 4), ("output", 1), ("median", 1)):
        for labels, L, host in ((grid, 4, [grid.flatten().cpu().numpy()] * 2), (bands, 3, list(bands.flatten(1).cpu().numpy()))):
            n0 = ops.launch_count()
            sums, counts, outside = model.region_scores(labels, L, what=what)
            assert ops.launch_count() == n0 + 2  # the two launches of ops.region_scores and nothing else
            assert tuple(sums.shape) == (2, L, 4) and tuple(counts.shape) == (2, L, S + 2)
            for b in range(2):
                em = ref.emulate(held[what][b], tgt[b], host[b], L)
                check_image(em, H * H, sums[b].cpu().numpy(), counts[b].cpu().numpy(), outside[b].cpu().numpy(), f"model {what} L={L} image {b}")
            record = region_score_summary(sums, counts, outside, S)
            assert sum(r["N_PIX"] for r in record["regions"]) == 2 * H * H and record["outside"] == 0 and record["invalid"] == 0
            assert all((r["SSR"] is None) == (S == 1) for r in record["regions"] if r["N_PIX"])
    direct = sde.region_scores(model.samples, model.target, grid[None].contiguous(), 4)
    via = model.region_scores(grid, 4)
    assert torch.equal(direct[0].view(torch.int64), via[0].view(torch.int64)) and torch.equal(direct[1], via[1])
    with pytest.raises(ValueError, match="what must be"):
        model.region_scores(grid, 4, what="mean")
    with pytest.raises(ValueError, match="uint8"):
        model.region_scores(grid.to(torch.int32), 4)
    with pytest.raises(ValueError):
        sde.region_scores(model.samples, model.target, grid[:, :16].contiguous(), 4)
    model.test()  # the members are not kept
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.region_scores(grid, 4)
    assert model.region_scores(grid, 4, what="output")[1].shape == (2, 4, 3)


NEW_WORDS = ("RMSE_r", "CRPS_r", "BIAS_r", "SSR_r", "regions")


def run_testum(tmp_path, capsys, name, extra, common):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {H}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", f"name: {name}").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / f"{name}.yml"
    cfg.write_text(txt)
    torch.manual_seed(0)  # --random-init draws the weights from the global generator: the same nets in every run of this test
    res = testUM.main(["-opt", str(cfg), "--random-init", "--limit", "2", "--sample-T", "2"] + common + extra)
    return res, capsys.readouterr().out.replace(str(tmp_path), "")


@pytest.mark.parametrize("common", [[], ["--num-samples", "4"]], ids=["plain", "ensemble"])
def test_testum_regions_option(tmp_path, capsys, common):
    S = 4 if common else 1
    plain, plain_out = run_testum(tmp_path, capsys, "drv_plain", [], common)
    for word in NEW_WORDS:
        assert word not in plain_out, word
    plain_lines = [ln for ln in plain_out.splitlines() if ln.startswith(" Testing ")]
    assert len(plain_lines) == 2
    for spec, L in (("grid:2x2", 4), ("bands:0.25,0.5", 3)):
        name = "drv_" + spec.split(":")[0]
        res, out = run_testum(tmp_path, capsys, name, ["--regions", spec], common)
        lines = [ln for ln in out.splitlines() if ln.startswith(" Testing ")]
        # the image's line is the plain run's with the per-region scores appended; every other file is byte for byte the plain run's
        for ln, before in zip(lines, plain_lines):
            assert ln.startswith(before + ", RMSE_r=[") and all(w in ln[len(before):] for w in ("CRPS_r=[", "BIAS_r=[", "SSR_r=[")), ln
        done = {k: v for k, v in res.items() if v['num']}
        assert sum(v['num'] for v in done.values()) == 2 and "pooled over" in out
        for kind, v in done.items():
            folder, plain_folder = tmp_path / "results" / name / kind, tmp_path / "results" / "drv_plain" / kind
            assert sorted(os.listdir(folder)) == sorted(os.listdir(plain_folder) + ["regions.json"])
            for f in os.listdir(plain_folder):
                assert open(folder / f, "rb").read() == open(plain_folder / f, "rb").read(), f
            assert set(v) == set(plain[kind]) | {"regions", "pooled_regions"}
            wrote = json.load(open(folder / "regions.json"))
            assert wrote["spec"] == spec and wrote["S"] == S and wrote["L"] == L and wrote["images"] == v['num'] and len(wrote["regions"]) == L
            assert sum(r["N_PIX"] for r in wrote["regions"]) == wrote["N_PIX"] == v['num'] * H * H  # the regions tile the image
            assert wrote["invalid"] == 0 and wrote["outside"] == 0
            pooled = region_score_summary(*(torch.cat([rec[q] for rec in v['regions']]) for q in range(3)), S)["regions"]
            for r, want in zip(wrote["regions"], pooled):  # on RMSE's x/2 + 0.5 scale: half of what the [-1, 1] tensors give
                for tag in ("RMSE", "CRPS", "BIAS"):
                    assert r[tag] == (None if want[tag] is None else 0.5 * want[tag]), tag
                assert r["SSR"] == want["SSR"] and r["PSNR"] == want["PSNR"] and (r["SSR"] is None) == (S == 1 or r["N_PIX"] == 0)
            if spec.startswith("grid"):
                assert [r["N_PIX"] for r in wrote["regions"]] == [v['num'] * H * H // 4] * 4
    # the image's RMSE is the regions' pooled: sum e over all regions / pixels, on the printed scale
    kind, v = next(iter(done.items()))
    rec = v['regions'][0]
    whole = 0.5 * float(np.sqrt(float(rec[0][0, :, 1].sum()) / (H * H)))
    if S == 1:  # the plain chain's output is what image_metrics scored
        assert whole == pytest.approx(v['RMSE'][0], rel=1e-5)
