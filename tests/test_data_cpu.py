"""The file-to-tensor path of the drivers (instancediff_amd/data.py) on real-format files.

`SpeckleMedDataset` and `DistIterSampler` against what the REAL reference classes returned for the same files and arguments
(tests/golden/data_golden.npz, written by tests/golden/make_golden_data.py from data/MedSpeckle.py and data/data_sampler.py): the
files are regenerated here from the closed formula of data_fixture_util.py and every item and index list must be equal bit for bit.
Beyond the fixture, on 8x8 files: side inference, refusals, filter order, truncation, the sampler's partition, `iterate_batches`,
`dump_raw` and `create_dataset`."""
import os
import sys

import numpy as np
import pytest
import torch

from instancediff_amd import data

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from data_fixture_util import EMB, MAX_SIZES, NAMES, PHASE, SAMPLER_CASES, SIDE, USE, embedding, image, sampler_key, write_dataset  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_golden.npz"))


@pytest.fixture(scope="module")
def flist224(tmp_path_factory):
    return write_dataset(tmp_path_factory.mktemp("speckle224"))


@pytest.fixture(scope="module")
def flist8(tmp_path_factory):
    return write_dataset(tmp_path_factory.mktemp("speckle8"), side=8)


class _Len:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_the_formula_spans_the_clamps():
    for k in range(len(NAMES)):
        for which in (0, 1):
            v = image(k, which)
            assert v.min() < 0 and v.max() > 1800 and ((v > 255) & (v < 1800)).any() and not np.array_equal(v, v.T)
    assert NAMES[0] not in USE and NAMES.count("noise in cryo-EM image") == 2 and set(USE) <= set(NAMES)


@pytest.mark.parametrize("max_size", MAX_SIZES)
def test_dataset_equals_the_reference(golden, flist224, max_size):
    ds = data.SpeckleMedDataset(flist224, phase=PHASE, max_dataset_size=max_size, use_artifact_type=list(USE))
    assert len(ds) == int(golden[f"ds{max_size}/len"]) == min(max_size, 4)
    for i in range(len(ds)):
        it = ds[i]
        assert set(it) == {"LQ", "GT", "LQ_path", "GT_path", "name", "A_emb"}
        assert it["name"] == str(golden[f"ds{max_size}/names"][i])
        k = int(golden[f"ds{max_size}/order"][i])
        assert os.path.basename(it["LQ_path"]) == f"{k}_A.raw" and os.path.basename(it["GT_path"]) == f"{k}_B.raw"
        for key, shape in (("LQ", (1, SIDE, SIDE)), ("GT", (1, SIDE, SIDE)), ("A_emb", (1, EMB))):
            want = torch.from_numpy(golden[f"ds{max_size}/{i}/{key}"])
            assert it[key].dtype == torch.float32 and tuple(it[key].shape) == shape
            assert torch.equal(it[key], want), (max_size, i, key, float((it[key] - want).abs().max()))


def test_the_golden_items_are_what_the_modalities_say(golden):
    """the fixture itself: CT clamps at 1800, cryo-EM at 255, OCT is not clamped; rows are rows"""
    names = [str(n) for n in golden["ds1000000/names"]]
    assert names == [n for n in NAMES if n in USE]
    for i, name in enumerate(names):
        k = int(golden["ds1000000/order"][i])
        for key, which in (("LQ", 0), ("GT", 1)):
            raw, got = image(k, which).astype(np.float64), golden[f"ds1000000/{i}/{key}"][0].astype(np.float64)
            top = {"scatter artifact in CT": 1800.0, "noise in cryo-EM image": 255.0}.get(name)
            want = (np.clip(raw, 0, top) / top if top else raw) * 2 - 1
            assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (name, key)
            assert (got.min(), got.max()) == ((-1.0, 1.0) if top else (-601.0, 4199.0))


@pytest.mark.parametrize("case", SAMPLER_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sampler_equals_the_reference(golden, case):
    n, world, rank, ratio, epoch = case
    s = data.DistIterSampler(_Len(n), num_replicas=world, rank=rank, ratio=ratio)
    s.set_epoch(epoch)
    got = torch.tensor(list(iter(s)), dtype=torch.int64)
    assert len(s) == len(got) and torch.equal(got, torch.from_numpy(golden[sampler_key(case)]))


# ---- beyond the fixture, on 8x8 files ------------------------------------------------------------------------------------------------
def test_side_is_inferred_and_misfits_raise(flist8, tmp_path):
    ds = data.SpeckleMedDataset(flist8, phase=PHASE, use_artifact_type=list(USE))
    it = ds[0]
    assert tuple(it["LQ"].shape) == (1, 8, 8) and tuple(it["GT"].shape) == (1, 8, 8) and tuple(it["A_emb"].shape) == (1, EMB)
    assert torch.equal(it["A_emb"][0], torch.from_numpy(embedding(1)))
    want = torch.from_numpy(image(1, 0, 8)).clamp(0, 1800) / 1800.0 * 2.0 - 1.0  # item 1 is CT; [y, x] stays [y, x]
    assert torch.equal(it["LQ"][0], want)
    explicit = data.SpeckleMedDataset(flist8, phase=PHASE, use_artifact_type=list(USE), image_size=8)
    assert torch.equal(explicit[0]["LQ"], it["LQ"])
    with pytest.raises(ValueError):
        data.SpeckleMedDataset(flist8, phase=PHASE, use_artifact_type=list(USE), image_size=4)[0]
    with pytest.raises(ValueError):
        data.SpeckleMedDataset(flist8, phase=PHASE, use_artifact_type=list(USE), image_size=16)[0]
    bad = write_dataset(tmp_path, side=8)
    np.arange(60, dtype="<f4").tofile(os.path.join(str(tmp_path), "1_A.raw"))  # 60 floats: no square
    with pytest.raises(ValueError):
        data.SpeckleMedDataset(bad, phase=PHASE, use_artifact_type=list(USE))[0]


def test_filter_keeps_file_order_and_truncation_comes_after_it(flist8):
    def order(**kw):
        ds = data.SpeckleMedDataset(flist8, phase=PHASE, **kw)
        return [int(os.path.basename(ds[i]["LQ_path"]).split("_")[0]) for i in range(len(ds))]
    assert order(use_artifact_type=list(USE)) == [1, 2, 3, 4]
    assert order(use_artifact_type=list(reversed(USE))) == [1, 2, 3, 4]
    assert order(use_artifact_type=list(USE), max_dataset_size=2) == [1, 2]  # truncation first would leave [1]
    assert order(use_artifact_type=["noise in cryo-EM image"], max_dataset_size=2) == [2, 4]
    assert order(use_artifact_type=list(NAMES)) == [0, 1, 2, 3, 4]
    assert order(use_artifact_type=[]) == []
    assert len(data.SpeckleMedDataset(flist8, phase="val", use_artifact_type=list(NAMES))) == 1


@pytest.mark.parametrize("n, world, ratio", [(5, 2, 1), (5, 3, 1), (8, 3, 1), (1, 3, 1), (5, 2, 100)])
def test_sampler_ranks_partition_total_size(n, world, ratio):
    ranks = [data.DistIterSampler(_Len(n), world, r, ratio) for r in range(world)]
    total = ranks[0].total_size
    assert total == ranks[0].num_samples * world >= n * ratio and total - n * ratio < world
    for epoch in (0, 3):
        for s in ranks:
            s.set_epoch(epoch)
        lists = [list(iter(s)) for s in ranks]
        perm = torch.randperm(total, generator=torch.Generator().manual_seed(epoch)).tolist()
        merged = [None] * total
        for r, idx in enumerate(lists):
            assert len(idx) == len(ranks[r]) == total // world
            merged[r::world] = idx
        assert merged == [v % n for v in perm]  # together the ranks are the whole permutation, each position once
        assert lists == [list(iter(s)) for s in ranks]  # reproducible
    ranks[0].set_epoch(0)
    a = list(iter(ranks[0]))
    ranks[0].set_epoch(1)
    b = list(iter(ranks[0]))
    ranks[0].set_epoch(0)
    assert list(iter(ranks[0])) == a and (a != b or total // world == 1)


def test_iterate_batches(flist8):
    ds = data.SpeckleMedDataset(flist8, phase=PHASE, use_artifact_type=list(NAMES))  # 5 items
    items = [ds[i] for i in range(5)]
    batches = list(data.iterate_batches(ds, 2))
    assert [len(b["name"]) for b in batches] == [2, 2, 1]
    for bi, b in enumerate(batches):
        assert set(b) == {"LQ", "GT", "A_emb", "name", "LQ_path", "GT_path"}
        n = len(b["name"])
        assert tuple(b["LQ"].shape) == (n, 1, 8, 8) == tuple(b["GT"].shape) and tuple(b["A_emb"].shape) == (n, 1, EMB)
        assert b["LQ"].dtype == b["GT"].dtype == b["A_emb"].dtype == torch.float32
        for j in range(n):
            it = items[2 * bi + j]
            assert torch.equal(b["LQ"][j], it["LQ"]) and torch.equal(b["GT"][j], it["GT"]) and torch.equal(b["A_emb"][j], it["A_emb"])
            assert (b["name"][j], b["LQ_path"][j], b["GT_path"][j]) == (it["name"], it["LQ_path"], it["GT_path"])
    assert [len(b["name"]) for b in data.iterate_batches(ds, 2, drop_last=True)] == [2, 2]
    assert [len(b["name"]) for b in data.iterate_batches(ds, 5, drop_last=True)] == [5]
    assert [len(b["name"]) for b in data.iterate_batches(ds, 6, drop_last=True)] == []

    def paths(**kw):
        return [p for b in data.iterate_batches(ds, 2, **kw) for p in b["LQ_path"]]
    plain = paths()
    assert plain == [it["LQ_path"] for it in items]
    s3, s3b, s4 = paths(shuffle=True, seed=3), paths(shuffle=True, seed=3), paths(shuffle=True, seed=4)
    assert s3 == s3b and s3 != s4 and sorted(s3) == sorted(plain) == sorted(s4)
    assert s3 == [plain[i] for i in torch.randperm(5, generator=torch.Generator().manual_seed(3)).tolist()]
    sampler = data.DistIterSampler(ds, 2, 1, 1)
    sampler.set_epoch(5)
    want = [plain[i] for i in iter(sampler)]
    assert len(want) == 3 and paths(sampler=sampler, shuffle=True, seed=3) == want  # the sampler wins over shuffle


def test_dump_raw_is_lq_pred_gt_side_by_side(tmp_path):
    lq, pred, gt = (torch.from_numpy(image(k, 0, 8)[:6])[None] for k in (0, 1, 2))  # [1, 6, 8]: H != W
    path = tmp_path / "sub" / "x.raw"
    shape = data.dump_raw(str(path), lq.numpy(), pred[None].numpy(), gt.numpy())
    assert tuple(shape) == (6, 24)
    back = np.fromfile(str(path), dtype="<f4")
    assert back.size == 6 * 24
    back = back.reshape(6, 24)
    assert np.array_equal(back[:, :8], lq[0].numpy()) and np.array_equal(back[:, 8:16], pred[0].numpy()) and np.array_equal(back[:, 16:], gt[0].numpy())


def test_create_dataset(flist8):
    ds = data.create_dataset(dict(mode="SpeckleMed", dataset_file=flist8, phase=PHASE, max_dataset_size=3, use_artifact_type=list(USE)))
    assert isinstance(ds, data.SpeckleMedDataset) and len(ds) == 3 and tuple(ds[0]["LQ"].shape) == (1, 8, 8)
    assert isinstance(data.create_dataset(dict(mode="Synthetic", max_dataset_size=2, image_size=16)), data.SyntheticDataset)
    with pytest.raises(NotImplementedError):
        data.create_dataset(dict(mode="LMDB"))
