"""The dataset and sampler cases shared by make_golden_data.py (which runs the reference's classes on them) and tests/test_data_cpu.py
(which runs instancediff_amd.data on the same files).  Everything is a closed integer formula: no RNG, nothing to seed."""
import json
import os

import numpy as np

SIDE = 224  # the reference hard-codes 224 x 224 (data/MedSpeckle.py:44-45)
EMB = 8
USE = ["scatter artifact in CT", "noise in cryo-EM image", "speckle in OCT"]
# file order; the first name is outside USE (so truncation before filtering would show), the last repeats a type
NAMES = ["Gaussian noise in MRI", "scatter artifact in CT", "noise in cryo-EM image", "speckle in OCT", "noise in cryo-EM image"]
MAX_SIZES = (1000000, 2)
PHASE = "train"

SAMPLER_CASES = [(n, world, rank, ratio, epoch) for n in (1, 5, 8) for world in (1, 2, 3) for rank in range(world)
                 for ratio in (1, 100) for epoch in (0, 1, 7)]


def image(k, which, side=SIDE):
    """item k, which = 0 (A / LQ) or 1 (B / GT): integers in [-300, 2100] -- below 0, above 255 and above 1800 -- that differ under
    a transpose"""
    y, x = np.meshgrid(np.arange(side, dtype=np.int64), np.arange(side, dtype=np.int64), indexing="ij")
    v = (3 * y * y + 37 * y + 101 * x + 577 * k + 1013 * which) % 2401 - 300
    return v.astype(np.float32)


def embedding(k, n=EMB):
    return (((7 * k + 3 * np.arange(n)) % 11) / 4.0 - 1.0).astype(np.float32)


def write_dataset(root, side=SIDE, names=NAMES, emb=EMB):
    """writes the raw little-endian float32 files and the JSON list; returns the list's path"""
    items = []
    for k, name in enumerate(names):
        paths = {key: os.path.join(str(root), f"{k}_{key}.raw") for key in ("A", "B", "A_emb")}
        image(k, 0, side).astype("<f4").tofile(paths["A"])
        image(k, 1, side).astype("<f4").tofile(paths["B"])
        embedding(k, emb).astype("<f4").tofile(paths["A_emb"])
        items.append(dict(paths, name=name))
    flist = os.path.join(str(root), "flist.json")
    with open(flist, "w") as f:
        json.dump({PHASE: items, "val": items[:1]}, f)
    return flist


def sampler_key(case):
    return "sampler/" + "_".join(str(int(v)) for v in case)
