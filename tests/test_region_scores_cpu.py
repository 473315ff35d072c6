"""Region-wise scores on the host: the C ABI's new symbols, the emulation of the contract (tests/region_scores_ref.py) against the textbook
grouping, region_score_summary (pooling before dividing, empty regions, S = 1, regions add to the image), the parsing and the refusals
of testUM --regions, ops.grid_labels against its formula, the band rule against np.searchsorted, and the dataset's optional "label" key."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
import region_scores_ref as ref
from ensemble_scores_ref import image_record

from instancediff_amd import _lib, ops, pipeline, testUM
from instancediff_amd.data import SpeckleMedDataset
from instancediff_amd.models.SDEs.driftSDE import ensemble_score_summary, region_score_summary

NEW_SYMBOLS = ["idiff_region_scores", "idiff_region_scores_ws_bytes", "idiff_band_labels"]


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    # (x, target, labels, labels_bstride, L, sums, counts, outside, ws, B, S, n_s, stream), (B, S, L), (y, labels, n, edges, ne, stream)
    assert _lib.SIGNATURES["idiff_region_scores"] == (I, [P, P, P, I64, I, P, P, P, P, I, I, I64, P])
    assert _lib.SIGNATURES["idiff_region_scores_ws_bytes"] == (I64, [I, I, I])
    assert _lib.SIGNATURES["idiff_band_labels"] == (I, [P, P, I64, ctypes.POINTER(ctypes.c_float), I, P])
    assert ops.REGION_MAX_L == 64


def test_workspace_size():
    """64 partial blocks per image of 4 L fp64 sums, L (S + 2) int32 bins and one outside count; 0 for what the call refuses"""
    lib = _lib.load()
    for B, S, L in [(1, 1, 1), (3, 8, 3), (16, 16, 16), (16, 17, 64), (65535, 64, 64)]:
        assert lib.idiff_region_scores_ws_bytes(B, S, L) == B * 64 * (L * 4 * 8 + (L * (S + 2) + 1) * 4)
        assert lib.idiff_region_scores_ws_bytes(B, S, L) % 4 == 0 and (B * 64 * L * 4 * 8) % 8 == 0
    for B, S, L in [(0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 65, 4), (1, 4, 0), (1, 4, 65)]:
        assert lib.idiff_region_scores_ws_bytes(B, S, L) == 0


# ---- 2. the emulation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 5])
def test_emulation_against_the_textbook_grouping(S):
    n, L = 600, 5
    x, y = ref.draw(S, n, seed=S)
    labels = ref.labels_outside(n, L, seed=S)
    em, tb = ref.emulate(x, y, labels, L), ref.textbook(x, y, labels, L)
    assert np.array_equal(em["counts"], tb["counts"]) and em["outside"] == tb["outside"] == int((labels >= L).sum())
    assert int(em["counts"].sum()) + em["outside"] == n
    # a float32 per-pixel term is within a few S rounding errors of the textbook's, relative to the magnitudes it was made of (|d| <= 1)
    assert np.all(np.abs(em["sums"] - tb["sums"]) <= 8 * (S + 2) * 2.0 ** -24 * np.maximum(em["n"][:, None], 1))
    if S == 1:  # crps = |d|, e = d*d, v = 0, k in {0, 1}
        rec = ref.pixel_record(x, y)
        d = rec["d"][0]
        assert np.array_equal(rec["crps"], np.abs(d)) and np.array_equal(rec["e"], d * d) and np.array_equal(rec["m"], d)
        assert not rec["v"].any() and set(rec["k"].tolist()) <= {0, 1}


def test_regions_add_to_the_whole_image_on_an_emulated_record():
    S, n, L = 4, 6000, 6  # blobs of up to 400 pixels: every region holds some
    x, y = ref.spoil(*ref.draw(S, n, seed=3), seed=4)
    labels = ref.labels_blobs(n, L, seed=5)
    rec = ref.pixel_record(x, y)
    em = ref.group(rec, labels, L, S)
    finite = rec["valid"] & np.isfinite(rec["d"]).all(axis=0)  # an infinite d makes the sums non-finite: compare where sums mean something
    whole_sums, whole_counts = image_record({**rec, "valid": finite}, S)
    parts = ref.group({**rec, "valid": finite}, labels, L, S)
    assert np.allclose(parts["sums"][:, :3].sum(axis=0), whole_sums, rtol=1e-12, atol=0)
    assert np.array_equal(parts["counts"][:, :S + 1].sum(axis=0), whole_counts[:S + 1])
    assert int(em["counts"].sum()) == n and em["outside"] == 0 and (em["counts"][:, S + 1] > 0).any()
    # and through the summary: the shares of the regions add to one, the pooled N_PIX to the valid pixels
    out = region_score_summary(parts["sums"], parts["counts"], [0], S)
    assert math.isclose(sum(r["ERR_SHARE"] for r in out["regions"]), 1.0, rel_tol=1e-12)
    assert math.isclose(sum(r["PIX_SHARE"] for r in out["regions"]), 1.0, rel_tol=1e-12)
    assert out["N_PIX"] == int(parts["n"].sum()) and out["invalid"] == int(parts["counts"][:, S + 1].sum())


# ---- 3. region_score_summary ---------------------------------------------------------------------------------------------------------
def test_summary_pools_before_dividing():
    S, L = 2, 2
    # image 0: region 0 has 10 pixels with sum e = 10, image 1: 90 pixels with sum e = 0: pooled RMSE^2 = 0.1, the mean of ratios 0.5
    sums = torch.zeros(2, L, 4, dtype=torch.float64)
    counts = torch.zeros(2, L, S + 2, dtype=torch.int64)
    sums[0, 0] = torch.tensor([5.0, 10.0, 2.5, -10.0])
    counts[0, 0] = torch.tensor([10, 0, 0, 1])
    counts[1, 0] = torch.tensor([30, 30, 30, 0])
    sums[1, 1] = torch.tensor([4.0, 16.0, 3.0, 8.0])
    counts[1, 1] = torch.tensor([0, 4, 0, 2])
    out = region_score_summary(sums, counts, [3, 4], S, names=["air", "bone"], data_range=2.0)
    r0, r1 = out["regions"]
    assert (r0["name"], r1["name"]) == ("air", "bone") and out["names"] == ["air", "bone"]
    assert r0["N_PIX"] == 100 and r1["N_PIX"] == 4 and out["N_PIX"] == 104 and out["invalid"] == 3 and out["outside"] == 7
    assert r0["CRPS"] == 0.05 and r0["RMSE"] == math.sqrt(0.1) and r0["BIAS"] == -0.1
    assert r0["PSNR"] == 20 * math.log10(2.0 / math.sqrt(0.1))
    assert r1["RMSE"] == 2.0 and r1["BIAS"] == 2.0 and r1["PSNR"] == 0.0 and r1["CRPS"] == 1.0
    assert r0["ERR_SHARE"] == 10 / 26 and r1["ERR_SHARE"] == 16 / 26 and r0["PIX_SHARE"] == 100 / 104
    # SSR, RANK_DEV, OUTLIERS exactly as ensemble_score_summary gives them for the same pooled sums and counts
    for l, r in enumerate(out["regions"]):
        want = ensemble_score_summary(sums[:, l, :3], counts[:, l], S)
        assert r["SSR"] == want["SSR"] and r["RANK_DEV"] == want["RANK_DEV"] and r["OUTLIERS"] == want["OUTLIERS"]
        assert r["hist"] == want["hist"] and r["invalid"] == want["invalid"] and r["CRPS"] == want["CRPS"] and r["RMSE"] == want["SKILL"]
    # per image: image 0 alone has RMSE 1 in region 0 and nothing in region 1
    i0, i1 = out["images"]
    assert i0[0]["RMSE"] == 1.0 and i0[0]["N_PIX"] == 10 and i0[1]["N_PIX"] == 0 and i1[0]["RMSE"] == 0.0 and i1[0]["PSNR"] is None
    assert i0[0]["ERR_SHARE"] == 1.0 and i1[0]["ERR_SHARE"] == 0.0 and i1[1]["ERR_SHARE"] == 1.0
    assert json.loads(json.dumps(out)) == out  # plain numbers, lists and None


def test_summary_of_empty_regions_and_of_one_member():
    S, L = 1, 3
    sums = torch.zeros(1, L, 4, dtype=torch.float64)
    counts = torch.zeros(1, L, S + 2, dtype=torch.int64)
    sums[0, 0] = torch.tensor([6.0, 18.0, 0.0, -6.0])
    counts[0, 0] = torch.tensor([2, 0, 0])
    counts[0, 2] = torch.tensor([0, 0, 5])  # only invalid pixels
    out = region_score_summary(sums, counts, [0], S)
    full, none, bad = out["regions"]
    assert full["CRPS"] == 3.0 and full["RMSE"] == 3.0 and full["BIAS"] == -3.0 and full["ERR_SHARE"] == 1.0 and full["PIX_SHARE"] == 1.0
    assert full["SSR"] is None and full["RANK_DEV"] is None and full["OUTLIERS"] is None  # one member has no spread and no ranks
    for r in (none, bad):
        assert r["N_PIX"] == 0 and r["PIX_SHARE"] == 0.0
        assert all(r[q] is None for q in ("CRPS", "RMSE", "PSNR", "BIAS", "SSR", "RANK_DEV", "OUTLIERS", "ERR_SHARE"))
    assert bad["invalid"] == 5 and out["invalid"] == 5
    nothing = region_score_summary(torch.zeros(2, L, 4), torch.zeros(2, L, S + 2, dtype=torch.int32), [4, 4], S)
    assert nothing["N_PIX"] == 0 and nothing["outside"] == 8
    assert all(r[q] is None for r in nothing["regions"] for q in ("CRPS", "RMSE", "PSNR", "BIAS", "ERR_SHARE", "PIX_SHARE"))
    with pytest.raises(ValueError, match="names"):
        region_score_summary(sums, counts, [0], S, names=["a"])
    with pytest.raises(ValueError, match="rows"):
        region_score_summary(sums, counts, [0, 0], S)
    assert region_score_summary(sums.tolist(), counts.numpy(), np.array([0]), S)["regions"] == out["regions"]  # lists and arrays too


# ---- 4. labels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,gy,gx", [(48, 48, 2, 2), (7, 9, 3, 4), (224, 224, 8, 8), (5, 64, 1, 64), (10, 10, 10, 1)])
def test_grid_labels_against_the_formula(H, W, gy, gx):
    lab = ops.grid_labels(H, W, gy, gx)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (H, W) and lab.device.type == "cpu"
    r, c = np.arange(H)[:, None], np.arange(W)[None]
    assert np.array_equal(lab.numpy(), (r * gy // H) * gx + (c * gx // W))
    assert sorted(set(lab.flatten().tolist())) == list(range(gy * gx))  # every cell holds a pixel
    assert ops.grid_labels(H, W, gy, gx) is lab  # cached


def test_grid_labels_refusals():
    for bad in [(48, 48, 9, 8), (48, 48, 0, 2), (4, 48, 5, 2), (48, 48, 2.0, 2), (48, 48, True, 2)]:
        with pytest.raises(ValueError):
            ops.grid_labels(*bad)


def test_the_band_rule_is_searchsorted_right():
    """labels = #{ j : edges[j] <= y }, written out, against np.searchsorted(side="right") on edges, +-0, +-inf and denormals"""
    edges = np.array([-0.5, 0.0, 1e-40, 0.75], dtype=np.float32)
    y = np.array([-np.inf, -1.0, -0.5, np.nextafter(np.float32(-0.5), np.float32(-1)), -0.0, 0.0, 1e-45, 1e-40, 0.5, 0.75, 1.0, np.inf],
                 dtype=np.float32)
    rule = (edges[None, :] <= y[:, None]).sum(axis=1)
    assert np.array_equal(rule, np.searchsorted(edges, y, side="right"))
    assert rule.tolist() == [0, 0, 1, 0, 2, 2, 2, 3, 3, 4, 4, 4]


# ---- 5. testUM ------------------------------------------------------------------------------------------------------------------------
def test_testum_parser_takes_the_option():
    parser = testUM.build_parser()
    plain = parser.parse_args(["-opt", "x.yml"])
    assert not hasattr(plain, "regions") and not hasattr(plain, "regions_L")  # without the flag the namespace is what it was
    assert parser.parse_args(["-opt", "x.yml", "--regions", "grid:2x2"]).regions == "grid:2x2"
    got = parser.parse_args(["-opt", "x.yml", "--regions", "file", "--regions-L", "3"])
    assert got.regions == "file" and got.regions_L == 3


def test_regions_specs():
    bands = testUM.parse_regions("bands:0.25,0.5,0.875")
    assert bands["kind"] == "bands" and bands["L"] == 4 and bands["edges"] == [-0.5, 0.0, 0.75]  # x/2 + 0.5 -> the tensors' [-1, 1]
    assert len(bands["names"]) == 4
    third = testUM.parse_regions("bands:0.3")["edges"][0]
    assert third == float(np.float32(2 * 0.3 - 1))  # what the kernel compares against: the float32 value
    grid = testUM.parse_regions("grid:2x3")
    assert (grid["kind"], grid["gy"], grid["gx"], grid["L"]) == ("grid", 2, 3, 6) and len(grid["names"]) == 6
    assert testUM.parse_regions("grid:8X8")["L"] == 64
    f = testUM.parse_regions("file", 5)
    assert f["kind"] == "file" and f["L"] == 5 and f["names"] == ["0", "1", "2", "3", "4"]
    assert len(testUM.parse_regions("bands:" + ",".join(str(i / 100) for i in range(63)))["edges"]) == 63
    for spec, L in [("bands:", None), ("bands:0.5,0.25", None), ("bands:0.5,0.5", None), ("bands:nan", None), ("bands:0.1,inf", None),
                    ("bands:a,b", None), ("bands:" + ",".join(str(i / 100) for i in range(64)), None), ("bands:0.75,0.75000000001", None),
                    ("grid:9x8", None), ("grid:0x4", None), ("grid:4", None), ("grid:2x2x2", None), ("grid:-1x2", None), ("grid:axb", None),
                    ("file", None), ("file", 0), ("file", 65), ("file:x", 4), ("grid:2x2", 4), ("bands:0.5", 2), ("blobs", None), ("", None)]:
        with pytest.raises(ValueError, match="--regions"):
            testUM.parse_regions(spec, L)


def test_testum_refuses_bad_regions_before_the_model_is_built(tmp_path, capsys):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results"))
    common = ["-opt", str(cfg), "--random-init", "--limit", "1"]
    for extra, word in [(["--regions", "grid:9x9"], "GY*GX <= 64"), (["--regions", "bands:0.5,0.25"], "strictly ascending"),
                        (["--regions", "file"], "--regions-L"), (["--regions", "file", "--regions-L", "65"], "[1, 64]"),
                        (["--regions-L", "4"], "--regions file"), (["--regions", "grid:2x2", "--regions-L", "4"], "--regions file"),
                        (["--regions", "circles:3"], "bands:e1,e2")]:
        with pytest.raises(SystemExit):
            testUM.main(common + extra)
        assert word in capsys.readouterr().err, extra
    assert not (tmp_path / "results").exists()  # before the model is built or any image ran


# ---- 6. the dataset's optional label map ------------------------------------------------------------------------------------------------
def test_the_dataset_reads_an_optional_label_map(tmp_path):
    s = 8
    rng = np.random.default_rng(0)
    for name in ("a.raw", "b.raw"):
        (rng.random((s, s)) * 255).astype(np.float32).tofile(tmp_path / name)
    rng.random(16).astype(np.float32).tofile(tmp_path / "emb.raw")
    lab = rng.integers(0, 256, (s, s)).astype(np.uint8)
    lab.tofile(tmp_path / "lab.raw")
    lab[:4].tofile(tmp_path / "short.raw")
    item = dict(A=str(tmp_path / "a.raw"), B=str(tmp_path / "b.raw"), A_emb=str(tmp_path / "emb.raw"), name="noise in cryo-EM image")
    flist = tmp_path / "list.json"
    flist.write_text(json.dumps(dict(test=[item, dict(item, label=str(tmp_path / "lab.raw")), dict(item, label=str(tmp_path / "short.raw"))])))
    ds = SpeckleMedDataset(str(flist), phase="test", use_artifact_type=("noise in cryo-EM image",))
    plain, labelled = ds[0], ds[1]
    assert set(plain) == {"LQ", "GT", "LQ_path", "GT_path", "name", "A_emb"}  # an item without the key is what it was
    assert set(labelled) == set(plain) | {"LABEL"}
    assert labelled["LABEL"].dtype == torch.uint8 and tuple(labelled["LABEL"].shape) == (s, s)
    assert np.array_equal(labelled["LABEL"].numpy(), lab)
    assert torch.equal(labelled["GT"], plain["GT"]) and torch.equal(labelled["LQ"], plain["LQ"])
    with pytest.raises(ValueError, match="labels for an image"):
        ds[2]
