"""No-reference despeckling statistics on the host: the C ABI's new symbols, the emulation of the contract (tests/despeckle_stats_ref.py)
against the float64 textbook, despeckle_summary (the None cases, the flat rule, the mean over images), homogeneous_cells and its ties,
known speckle (gamma of 4 looks), and the parsing and the refusals of testUM --speckle."""
import ctypes
import math

import numpy as np
import pytest
import torch
import despeckle_stats_ref as ref

from instancediff_amd import _lib, ops, pipeline, testUM
from instancediff_amd.models.SDEs.driftSDE import DESPECKLE_METRICS, despeckle_summary, homogeneous_cells

NEW_SYMBOLS = ["idiff_despeckle_stats", "idiff_despeckle_stats_ws_bytes"]


def record(x, y, labels, L, **kw):
    """one row's emulated record as despeckle_summary takes it: sums [1, L, 12], counts [1, L, 4], outside [1]"""
    em = ref.emulate(x, y, labels, L, **kw)
    return em["sums"][None], em["counts"][None], np.array([em["outside"]])


def whole(x, y, **kw):
    """the summary of one H x W image as one region"""
    x, y = np.asarray(x, np.float32)[None], np.asarray(y, np.float32)[None]
    return despeckle_summary(*record(x, y, np.zeros(x.shape, np.uint8), 1, **kw))["rows"][0][0]


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header
    P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    # (x, ref, labels, labels_bstride, L, scale, shift, ratio_floor, sums, counts, outside, ws, B, S, P, H, W, stream), (B, S, L)
    assert _lib.SIGNATURES["idiff_despeckle_stats"] == (I, [P, P, P, I64, I, F, F, F, P, P, P, P, I, I, I, I, I, P])
    assert _lib.SIGNATURES["idiff_despeckle_stats_ws_bytes"] == (I64, [I, I, I])
    assert ops.DESPECKLE_NQ == 12 and ops.DESPECKLE_NC == 4


def test_workspace_size():
    """64 partial blocks per row (b, s) of 12 L fp64 sums, 4 L int32 counts and one outside count; 0 for what the call refuses"""
    lib = _lib.load()
    for B, S, L in [(1, 1, 1), (3, 8, 3), (16, 16, 64), (1023, 64, 64), (65535, 1, 2)]:
        assert lib.idiff_despeckle_stats_ws_bytes(B, S, L) == B * S * 64 * (L * 12 * 8 + (L * 4 + 1) * 4)
    for B, S, L in [(0, 4, 4), (1024, 64, 4), (65536, 1, 4), (1, 0, 4), (1, 65, 4), (1, 4, 0), (1, 4, 65)]:
        assert lib.idiff_despeckle_stats_ws_bytes(B, S, L) == 0


# ---- 2. the emulation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,H,W", [(1, 1, 4), (1, 2, 8), (2, 5, 12), (1, 17, 20)])
def test_emulation_against_the_textbook(P, H, W):
    L = 3
    x, y = ref.draw(P, H, W, seed=H)
    x[0, H // 2, 1] = ref.NAN
    y[P - 1, 0, W - 1] = ref.INF
    labels = ref.labels_outside(P, H, W, L, seed=W)
    em, tb = ref.emulate(x, y, labels, L), ref.textbook(x, y, labels, L)
    assert np.array_equal(em["counts"], tb["counts"]) and em["outside"] == tb["outside"] == int((labels >= L).sum())
    assert int(em["counts"][:, [0, 3]].sum()) + em["outside"] == P * H * W
    assert int(em["counts"][:, 3].sum()) == int(((labels < L) & ~(np.isfinite(x) & np.isfinite(y))).sum()) > 0
    if H <= 2:  # no interior line: no stencil pixel, untouched sums
        assert not em["counts"][:, 2].any() and not em["sums"][:, 7:].any() and not np.signbit(em["sums"][:, 7:]).any()
    # a and y lie in [0, 1] after two roundings (|error| <= 2^-23); rho <= 2^8 carries one more on a quotient whose operands carry those,
    # relative to a >= 2^-8: |error| <= 2^8 (2^-23 + 2^8 2^-23) + 2^-16 < 2^-6 at worst, far less at the values drawn (a >= 0.05: 2^-16);
    # La, Ly are five more operations on magnitudes <= 4: |error| <= 2^-19.  Squares and products double the relative error.
    tol = np.array([2.0 ** -23, 2.0 ** -21, 2.0 ** -23, 2.0 ** -21, 2.0 ** -21, 2.0 ** -10, 2.0 ** -4, 2.0 ** -19, 2.0 ** -19, 2.0 ** -15,
                    2.0 ** -15, 2.0 ** -15])
    n = em["counts"][:, [0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2]]
    assert np.all(np.abs(em["sums"] - tb["sums"]) <= tol[None] * np.maximum(n, 1))
    assert float(em["terms"][5].max()) < 40  # the drawn ratios stay small: the rho tolerance above is loose for them


def test_the_emulation_keeps_a_stencil_inside_its_plane():
    """P = 2 at 5 x 12: the last line of plane 0 and the first of plane 1 have no stencil pixel, whatever their neighbours in memory"""
    x, y = ref.draw(2, 5, 12, seed=1)
    t = ref.pixel_terms(x, y)
    want = np.zeros((2, 5, 12), dtype=bool)
    want[:, 1:4, 1:11] = True
    assert np.array_equal(t["stencil"], want)
    lap = x.astype(np.float64) * 0.5 + 0.5
    full = lap[:, :-2, 1:-1] + lap[:, 2:, 1:-1] + lap[:, 1:-1, :-2] + lap[:, 1:-1, 2:] - 4 * lap[:, 1:-1, 1:-1]
    assert np.abs(t["la"][:, 1:4, 1:11] - full).max() < 2.0 ** -19


# ---- 3. the summary ------------------------------------------------------------------------------------------------------------------
def test_a_constant_plane_is_flat():
    """a constant 0.3 plane of 48 x 48: variance 0.0 against the threshold 8 * 2^-53 * sum a^2 = 1.8e-13; ENL is None, nothing divides"""
    x = np.full((48, 48), 0.3, dtype=np.float32)
    got = whole(x, x, scale=1.0, shift=0.0)
    assert got["FLAT"] is True and got["ENL"] is None and got["ENL_REF"] is None and got["SSI"] is None and got["SMPI"] is None
    assert got["STD"] == 0.0 and got["MEAN"] == float(np.float32(0.3)) and got["N_PIX"] == 48 * 48
    assert got["MEAN_RATIO"] == 1.0 and got["VAR_RATIO"] == 0.0 and got["ENL_RATIO"] is None
    assert got["EPI"] is None and got["LAP_RATIO"] is None and got["N_STENCIL"] == 46 * 46  # the Laplacian of a constant is 0
    assert 8 * 2.0 ** -53 * float(np.float32(0.3)) ** 2 * 48 * 48 == pytest.approx(1.8e-13, rel=0.05)
    # sums rounded as a device sum may round them (one ulp off the exact sum) stay flat
    s, c, o = record(x[None], x[None], np.zeros((1, 48, 48), np.uint8), 1, scale=1.0, shift=0.0)
    s = s.copy()
    s[0, 0, 0] = np.nextafter(s[0, 0, 0], np.inf)
    s[0, 0, 1] = np.nextafter(s[0, 0, 1], -np.inf)
    assert despeckle_summary(s, c, o)["rows"][0][0]["FLAT"] is True


def test_summary_none_cases_never_divide_by_zero():
    L = 4
    sums, counts = torch.zeros(1, L, 12, dtype=torch.float64), torch.zeros(1, L, 4, dtype=torch.int32)
    # region 0: empty.  region 1: pixels, all invalid.  region 2: valid pixels of a varying image against a constant reference, no ratio
    # and no stencil pixel.  region 3: two valid pixels with a = 0 exactly.
    counts[0, 1] = torch.tensor([0, 0, 0, 9])
    counts[0, 2] = torch.tensor([4, 0, 0, 0])
    sums[0, 2, :5] = torch.tensor([1 + 2 + 3 + 4, 1 + 4 + 9 + 16, 4 * 0.5, 4 * 0.25, 0.5 * 10], dtype=torch.float64)
    counts[0, 3] = torch.tensor([2, 0, 0, 0])
    got = despeckle_summary(sums, counts, torch.tensor([7]))
    rows = got["rows"][0]
    for l in (0, 1):
        assert all(rows[l][m] is None for m in DESPECKLE_METRICS) and rows[l]["FLAT"] is None and rows[l]["N_PIX"] == 0
    assert rows[1]["invalid"] == 9 and got["outside"] == 7
    r = rows[2]
    assert r["MEAN"] == 2.5 and r["STD"] == pytest.approx(math.sqrt(1.25)) and r["ENL"] == pytest.approx(5.0) and r["FLAT"] is False
    assert r["MEAN_REF"] == 0.5 and r["ENL_REF"] is None and r["SSI"] is None and r["SMPI"] is None  # zero variance of the reference
    assert r["MEAN_RATIO"] is None and r["VAR_RATIO"] is None and r["ENL_RATIO"] is None  # no ratio pixel
    assert r["EPI"] is None and r["LAP_RATIO"] is None  # no stencil pixel
    assert r["CNR"] is None  # the background, region 0, is empty
    assert rows[3]["MEAN"] == 0.0 and rows[3]["FLAT"] is True and rows[3]["ENL"] is None and rows[3]["SSI"] is None
    again = despeckle_summary(sums, counts, torch.tensor([7]), background=2)["rows"][0]
    assert again[2]["CNR"] == 0.0 and again[3]["CNR"] == pytest.approx(2.5 / math.sqrt(1.25)) and again[0]["CNR"] is None
    for bad in (dict(names=["a"]), dict(background=4), dict(background=True), dict(background=-1)):
        with pytest.raises(ValueError):
            despeckle_summary(sums, counts, torch.tensor([7]), **bad)
    with pytest.raises(ValueError):
        despeckle_summary(sums[..., :4], counts, torch.tensor([7]))
    with pytest.raises(ValueError):
        despeckle_summary(sums, counts[:, :2], torch.tensor([7]))


def test_summary_takes_the_mean_over_images_and_counts_where_defined():
    """[B, S, L, 12] flattens into B S rows; a region reports the mean of a metric over the rows where it is defined, not pooled sums"""
    L = 2
    sums, counts = torch.zeros(2, 2, L, 12, dtype=torch.float64), torch.zeros(2, 2, L, 4, dtype=torch.int32)
    vals = {(0, 0): [1.0, 3.0], (0, 1): [10.0, 30.0], (1, 0): [2.0, 2.0]}  # row (1, 1) stays empty; row (1, 0) is flat
    for (b, s), v in vals.items():
        counts[b, s, 0, 0] = len(v)
        sums[b, s, 0, 0], sums[b, s, 0, 1] = sum(v), sum(t * t for t in v)
    got = despeckle_summary(sums, counts, torch.zeros(2, dtype=torch.int32), names=["roi", "rest"])
    assert got["shape"] == [2, 2] and len(got["rows"]) == 4 and got["names"] == ["roi", "rest"]
    roi = got["regions"][0]
    assert roi["defined"]["MEAN"] == 3 and roi["MEAN"] == pytest.approx((2.0 + 20.0 + 2.0) / 3)
    assert roi["defined"]["ENL"] == 2 and roi["ENL"] == pytest.approx(4.0)  # both 4 = 2^2 / 1 = 20^2 / 100; pooled sums would give 1.2
    assert roi["N_PIX"] == 6 and got["regions"][1]["MEAN"] is None and got["regions"][1]["defined"]["MEAN"] == 0


def test_homogeneous_cells_and_their_ties():
    L = 6
    sums, counts = torch.zeros(1, L, 12, dtype=torch.float64), torch.zeros(1, L, 4, dtype=torch.int32)
    # the reference's (y) values per cell; cell 4 is empty; cells 1 and 3 tie at the lowest CV (a scaled copy has the same CV exactly)
    ys = {0: [1.0, 3.0], 1: [2.0, 2.5], 2: [1.0, 5.0], 3: [4.0, 5.0], 5: [1.0, 2.0]}
    for l, v in ys.items():
        counts[0, l, 0] = 2
        sums[0, l, 2], sums[0, l, 3] = sum(v), sum(t * t for t in v)
        sums[0, l, 0], sums[0, l, 1] = 2.0 * (l + 1), (l + 1.0) ** 2 + 1.0 + (l + 1.0) ** 2 - 1.0 + 2.0  # a = (l + 1) -+ 1: ENL = (l + 1)^2
    one = homogeneous_cells(sums, counts)  # ceil(0.25 * 5) = 2 cells
    assert one["cells"] == [[1, 3]] and one["ENL_AUTO"] == [pytest.approx((4.0 + 16.0) / 2)]
    assert homogeneous_cells(sums, counts, share=0.2)["cells"] == [[1]]  # the tie goes to the lower index
    assert homogeneous_cells(sums, counts, share=0.6)["cells"] == [[1, 3, 5]]
    assert homogeneous_cells(sums, counts, share=1.0)["cells"] == [[1, 3, 5, 0, 2]]
    assert homogeneous_cells(sums, counts, share=0.1)["cells"] == [[1]]  # never none of a non-empty row
    empty = homogeneous_cells(torch.zeros(2, L, 12, dtype=torch.float64), torch.zeros(2, L, 4, dtype=torch.int32))
    assert empty["cells"] == [[], []] and empty["ENL_AUTO"] == [None, None]
    for bad in (0, 1.5, -0.25, True):
        with pytest.raises(ValueError):
            homogeneous_cells(sums, counts, share=bad)


# ---- 4. known speckle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [(0, 64), (1, 64), (2, 48)])
def test_known_speckle(seed, n):
    """gamma speckle of 4 looks on a constant 0.5.  The ENL estimator's sampling standard deviation at 4096 pixels is about 3.3 %: 13 %
    is 4 sigma; the ratio image against the clean constant has variance 1 / looks and mean 1."""
    clean = np.full((n, n), 0.5, dtype=np.float32)
    noisy = (np.random.default_rng(seed).gamma(4, 0.25, (n, n)) * 0.5).astype(np.float32)
    kw = dict(scale=1.0, shift=0.0)
    self_ = whole(noisy, noisy, **kw)
    assert abs(self_["ENL"] - 4.0) <= 0.13 * 4.0 and self_["ENL_REF"] == self_["ENL"] and self_["FLAT"] is False
    assert abs(self_["SSI"] - 1.0) <= 2.0 ** -50 and abs(self_["EPI"] - 1.0) <= 2.0 ** -50 and self_["LAP_RATIO"] == 1.0
    assert self_["MEAN_RATIO"] == 1.0 and self_["ENL_RATIO"] is None  # y / y: a flat ratio image
    restored = whole(clean, noisy, **kw)
    assert abs(restored["VAR_RATIO"] - 0.25) <= 0.13 * 0.25 and abs(restored["MEAN_RATIO"] - 1.0) <= 0.02
    assert abs(restored["ENL_RATIO"] - 4.0) <= 0.3 * 4.0  # the quotient of the two above
    assert restored["FLAT"] is True and restored["ENL"] is None and abs(restored["ENL_REF"] - 4.0) <= 0.13 * 4.0
    assert restored["SSI"] == 0.0 and restored["EPI"] is None  # nothing of the speckle is left; the Laplacian of the constant is 0
    print(f"seed {seed} n {n}: ENL {self_['ENL']:.4f} VAR_RATIO {restored['VAR_RATIO']:.4f} MEAN_RATIO {restored['MEAN_RATIO']:.4f}")


def test_cnr_and_smoothing_on_a_two_region_image():
    """a bright square on a darker ground, speckled: CNR of the square against the ground from the textbook formula; a 3 x 3 box mean of
    the image has the higher ENL, SSI < 1 and LAP_RATIO < 1 against it"""
    rng = np.random.default_rng(5)
    n = 48
    scene = np.full((n, n), 0.2)
    scene[12:36, 12:36] = 0.6
    labels = (scene > 0.4).astype(np.uint8)[None]
    noisy = (scene * rng.gamma(8, 1 / 8, (n, n))).astype(np.float32)
    pad = np.pad(noisy.astype(np.float64), 1, mode="edge")
    box = (sum(pad[i:i + n, j:j + n] for i in range(3) for j in range(3)) / 9).astype(np.float32)
    kw = dict(scale=1.0, shift=0.0)
    raw = despeckle_summary(*record(noisy[None], noisy[None], labels, 2, **kw))["rows"][0]
    smooth = despeckle_summary(*record(box[None], noisy[None], labels, 2, **kw))["rows"][0]
    a = noisy.astype(np.float64)
    want = abs(a[labels[0] == 1].mean() - a[labels[0] == 0].mean()) / math.sqrt(a[labels[0] == 1].var() + a[labels[0] == 0].var())
    assert raw[1]["CNR"] == pytest.approx(want, rel=1e-12) and raw[0]["CNR"] == 0.0
    for l in (0, 1):
        assert smooth[l]["ENL"] > 2 * raw[l]["ENL"] and smooth[l]["SSI"] < 0.7 and smooth[l]["LAP_RATIO"] < 0.5
        assert smooth[l]["SMPI"] < raw[l]["SMPI"] == pytest.approx(1.0)
    assert smooth[1]["CNR"] > raw[1]["CNR"]
    # EPI is the Pearson correlation of the two Laplacians over the stencil pixels of the region (np.corrcoef on the float64 values)
    tb = ref.textbook(box[None], noisy[None], labels, 2, **kw)
    for l in (0, 1):
        sel = (labels == l) & tb["masks"][2]
        want = float(np.corrcoef(tb["terms"][7][sel], tb["terms"][8][sel])[0, 1])
        assert smooth[l]["EPI"] == pytest.approx(want, abs=1e-5) and abs(want) < 1


# ---- 5. testUM ------------------------------------------------------------------------------------------------------------------------
def test_testum_parser_takes_the_option():
    parser = testUM.build_parser()
    plain = parser.parse_args(["-opt", "x.yml"])
    assert not any(hasattr(plain, a) for a in ("speckle", "speckle_L", "speckle_background"))  # without the flag: as it was
    assert parser.parse_args(["-opt", "x.yml", "--speckle"]).speckle == "grid:8x8"
    assert parser.parse_args(["-opt", "x.yml", "--speckle", "bands:0.5"]).speckle == "bands:0.5"
    got = parser.parse_args(["-opt", "x.yml", "--speckle", "file", "--speckle-L", "3", "--speckle-background", "2"])
    assert got.speckle == "file" and got.speckle_L == 3 and got.speckle_background == 2


def test_speckle_specs():
    grid = testUM.parse_speckle("grid:8x8")
    assert (grid["kind"], grid["L"], grid["background"]) == ("grid", 64, 0) and len(grid["names"]) == 64
    assert testUM.parse_speckle("bands:0.25,0.5", None, 2)["background"] == 2
    f = testUM.parse_speckle("file", 5, 4)
    assert f["kind"] == "file" and f["L"] == 5 and f["background"] == 4
    for spec, L, bg in [("grid:9x8", None, None), ("bands:0.5,0.25", None, None), ("file", None, None), ("file", 65, None),
                        ("grid:2x2", 4, None), ("blobs", None, None), ("grid:2x2", None, 4), ("grid:2x2", None, -1),
                        ("file", 3, 3), ("grid:2x2", None, True)]:
        with pytest.raises(ValueError, match="--speckle") as e:
            testUM.parse_speckle(spec, L, bg)
        assert "--regions" not in str(e.value)


def test_testum_refuses_bad_speckle_before_the_model_is_built(tmp_path, capsys):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results"))
    common = ["-opt", str(cfg), "--random-init", "--limit", "1"]
    for extra, word in [(["--speckle", "grid:9x9"], "GY*GX <= 64"), (["--speckle", "file"], "--speckle-L"),
                        (["--speckle", "file", "--speckle-L", "65"], "[1, 64]"), (["--speckle-L", "4"], "go with --speckle"),
                        (["--speckle-background", "1"], "go with --speckle"), (["--speckle", "grid:2x2", "--speckle-L", "4"], "--speckle file"),
                        (["--speckle", "grid:2x2", "--speckle-background", "4"], "[0, 4)"), (["--speckle", "circles:3"], "bands:e1,e2")]:
        with pytest.raises(SystemExit):
            testUM.main(common + extra)
        assert word in capsys.readouterr().err, extra
    assert not (tmp_path / "results").exists()  # before the model is built or any image ran
