"""One trainUM -> testUM round trip on real-format files (`mode: SpeckleMed`): raw float32 LQ / GT / A_emb files behind a JSON list,
one cryo-EM item (0..255 with values outside it, so the clamp acts) and one OCT item (not normalised).  The LQ and GT thirds of each
result triptych are the dataset's tensors bit for bit, and the RMSE / PSNR / SSIM the driver lists for an image are the reference
metrics of its pred and GT thirds, within the bounds of tests/test_image_metrics_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from image_metrics_ref import PSNR_TOL, RMSE_TOL, reference, ssim_bound  # noqa: E402
from instancediff_amd import data, pipeline, testUM, trainUM  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

SIDE = 32
NAMES = ["noise in cryo-EM image", "speckle in OCT"]


def _write_files(root):
    b = make_batch(2, SIDE, seed=21)
    gt01, lq01 = b["target"] / 2 + 0.5, b["input"] / 2 + 0.5
    items = []
    for k, name in enumerate(NAMES):
        scale, shift = (295.0, -20.0) if k == 0 else (1.0, 0.0)  # cryo-EM: -20 .. 275 and beyond, clamped to 0 .. 255 by the dataset
        paths = {key: os.path.join(str(root), f"{k}_{key}.raw") for key in ("A", "B", "A_emb")}
        (lq01[k, 0] * scale + shift).numpy().astype("<f4").tofile(paths["A"])
        (gt01[k, 0] * scale + shift).numpy().astype("<f4").tofile(paths["B"])
        b["A_emb"][k].numpy().astype("<f4").tofile(paths["A_emb"])
        items.append(dict(paths, name=name))
    flist = os.path.join(str(root), "flist.json")
    with open(flist, "w") as f:
        json.dump({"train": items, "val": items[:1]}, f)
    return flist


def test_train_then_test_drivers_on_raw_files(tmp_path):
    files = tmp_path / "files"
    files.mkdir()
    flist = _write_files(files)
    ds = data.SpeckleMedDataset(flist, phase="train", use_artifact_type=NAMES)
    assert len(ds) == 2 and tuple(ds[0]["LQ"].shape) == (1, SIDE, SIDE) and tuple(ds[0]["A_emb"].shape) == (1, 512)
    raw = np.fromfile(os.path.join(str(files), "0_A.raw"), dtype="<f4")
    assert raw.min() < 0 and raw.max() > 255 and float(ds[0]["LQ"].min()) == -1.0 and float(ds[0]["LQ"].max()) == 1.0

    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_data").replace("image_size: 64", f"image_size: {SIDE}")
    assert txt.count("mode: Synthetic") == 2
    txt = txt.replace("mode: Synthetic", f"mode: SpeckleMed\n    dataset_file: {flist}")
    txt = txt.replace("T: 100", "T: 4").replace("val_freq: 3", "val_freq: 2\n  max_iters: 2").replace("save_checkpoint_freq: 8", "save_checkpoint_freq: 2")
    txt = txt.replace("path:\n", f"path:\n  root: {tmp_path}\n")
    txt = txt.replace("pth_dir: experiments/UM_IDDM_SM_IB/models", f"pth_dir: {tmp_path}/experiments/drv_data/models")
    txt = txt.replace("iter: latest", "iter: 2").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    assert trainUM.main(["-opt", str(cfg)]) == 2
    vals = [f for f in os.listdir(tmp_path / "experiments" / "drv_data" / "val_images") if f.endswith(".raw")]
    assert vals
    res = testUM.main(["-opt", str(cfg), "--limit", "2"])
    assert {k: v["num"] for k, v in res.items() if v["num"]} == {NAMES[0]: 1, NAMES[1]: 1}
    for i, name in enumerate(NAMES):
        path = os.path.join(str(tmp_path), "results", "drv_data", name, f"{i}_{3 * SIDE}x{SIDE}x1.raw")
        trip = np.fromfile(path, dtype="<f4").reshape(SIDE, 3 * SIDE)
        lq, pred, gt = (np.ascontiguousarray(trip[:, k * SIDE:(k + 1) * SIDE]) for k in range(3))
        it = ds[i]
        assert it["name"] == name
        assert torch.equal(torch.from_numpy(lq), it["LQ"][0]) and torch.equal(torch.from_numpy(gt), it["GT"][0])
        assert np.isfinite(pred).all()
        r, ps, s = reference(pred, gt)
        bound, e_row = ssim_bound(pred, gt)
        got = (res[name]["RMSE"][0], res[name]["PSNR"][0], res[name]["SSIM"][0])
        print(f"{name}: listed {got}, reference {(r, ps, s)}, SSIM bound {bound:.3e} (E_row {e_row:.2e})")
        assert abs(got[0] - r) <= RMSE_TOL and abs(got[1] - ps) <= PSNR_TOL, (name, got, (r, ps, s))
        assert abs(got[2] - s) <= bound, (name, abs(got[2] - s), bound, e_row)
