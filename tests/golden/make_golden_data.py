#!/usr/bin/env python3
"""Generate golden vectors for the data path from the REAL reference classes.

Runs only in the dev container (needs /root/reference).  It imports /root/reference/data/MedSpeckle.py and data/data_sampler.py
*by path* (the reference's `data/__init__.py` pulls in the whole training stack) after inserting a stub `torchvision.transforms`
module: `Resize`, `Normalize` and `Compose` are only constructed on this path, never applied (MedSpeckle.py:5-10,32).  Nothing from
the reference is copied: the output is data only (the items `SpeckleMedDataset` returns for the files of data_fixture_util.py, and
the index lists of `DistIterSampler`), written to tests/golden/data_golden.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_data.py
"""
import importlib.util
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from data_fixture_util import MAX_SIZES, PHASE, SAMPLER_CASES, USE, sampler_key, write_dataset  # noqa: E402

REF = "/root/reference/data"
OUT = os.path.join(HERE, "data_golden.npz")


def load_reference(fname, modname):
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")

    class _Constructed:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            raise RuntimeError("the torchvision stub is only constructed on this path")

    tvt.Resize = tvt.Normalize = tvt.Compose = _Constructed
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    med = load_reference("MedSpeckle.py", "ref_medspeckle")
    samp = load_reference("data_sampler.py", "ref_data_sampler")
    out = {}
    with tempfile.TemporaryDirectory() as root:
        flist = write_dataset(root)
        for m in MAX_SIZES:
            ds = med.SpeckleMedDataset(flist, phase=PHASE, max_dataset_size=m, use_artifact_type=list(USE))
            out[f"ds{m}/len"] = np.array(len(ds))
            out[f"ds{m}/names"] = np.array([ds[i]["name"] for i in range(len(ds))])
            out[f"ds{m}/order"] = np.array([int(os.path.basename(ds[i]["LQ_path"]).split("_")[0]) for i in range(len(ds))])
            for i in range(len(ds)):
                it = ds[i]
                for key in ("LQ", "GT", "A_emb"):
                    assert it[key].dtype == torch.float32
                    out[f"ds{m}/{i}/{key}"] = it[key].numpy()

    class _Len:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    for case in SAMPLER_CASES:
        n, world, rank, ratio, epoch = case
        s = samp.DistIterSampler(_Len(n), num_replicas=world, rank=rank, ratio=ratio)
        s.set_epoch(epoch)
        idx = list(iter(s))
        assert len(idx) == len(s)
        out[sampler_key(case)] = np.array(idx, dtype=np.int64)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
