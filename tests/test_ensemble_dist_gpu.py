"""Ensemble member distances on the device (idiff_ensemble_distances / idiff_ensemble_pick_rows through the C ABI and ops): the matrix
against the float64 emulation of the contract (tests/ensemble_dist_ref.py) within the bound of an fp64 sum, bit for bit on integers, the
identities against ops.ensemble_scores, independence of the batch and of the run, invalid pixels, the picks, the row copy, the refusals,
and the driftSDE / model / testUM surface."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ensemble_dist_ref import draw, draw_int, emulate, exact_int, picks  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import ensemble_distance_summary  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
# one float4 group; one group past a 256-thread block; one group past one sweep of the 64 x 256-thread grid of an image
N_S = [4, 1028, 64 * 1024 + 4]
# M = S + 1 rows with the target, S without: one partial tile; a full 8-row tile and one row; two tiles; edge tiles on both sides of 4 and 8
S_ALL = [1, 2, 5, 16, 17, 33, 64]
B_MAX = 3
QNAN = 0x7fc00000


@functools.lru_cache(maxsize=None)
def case(S, n_s):
    """(x [3, S, n_s], y [3, n_s] float32 on the host, the emulation of each image): computed once and shared, never modified"""
    pairs = [draw(S, n_s, seed=104729 * S + n_s + b) for b in range(B_MAX)]
    x, y = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return torch.from_numpy(x), torch.from_numpy(y), [emulate(x[b], y[b]) for b in range(B_MAX)]


def bits64(t):
    return t.contiguous().view(torch.int64)


def bits(t):
    return t.contiguous().view(torch.int32)


def check_image(em, d2, counts, pick, S, has_target, what):
    """one image's device results against its emulation: counts exactly, every entry within the bound of an fp64 sum of `valid`
    non-negative terms (each term carries the rounding of its square, the sum `valid` - 1 more; a factor 2 as the only margin), the
    diagonal +0.0, the two halves the same bits, and the picks exactly what the device matrix gives under the stated scan"""
    M = S + has_target
    assert tuple(d2.shape) == (M, M) and counts.tolist() == list(em["counts"]), what
    got, want = d2.numpy(), em["d2"][:M, :M]
    err, bound = np.abs(got - want), 2 * (em["counts"][0] + 2) * 2.0 ** -53 * want
    worst = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{what}: worst |d2 - host| / bound {worst:.3f}")
    assert (err <= bound).all(), (what, worst)
    assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64)), what
    assert not got.diagonal().view(np.int64).any(), what  # +0.0, not -0.0
    assert tuple(pick.tolist()) == picks(got, S, has_target), what


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_distances_against_the_emulation(S, n_s):
    """B = 3 and B = 1 on the same data, with the target: matrix, counts and picks of every image, and image 0 of the batch bit for bit
    what it is alone; without the target: the member block bit for bit that of the call with it, and no best member"""
    x, y, ems = case(S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    d3, c3, p3 = ops.ensemble_distances(xd, yd)
    assert d3.dtype == torch.float64 and d3.shape == (3, S + 1, S + 1) and d3.is_cuda
    assert c3.dtype == torch.int32 and c3.shape == (3, 2) and p3.dtype == torch.int32 and p3.shape == (3, 2)
    for b in range(B_MAX):
        check_image(ems[b], d3[b].cpu(), c3[b].cpu(), p3[b].cpu(), S, 1, f"B=3 S={S} n_s={n_s} image {b}")
        assert c3[b].tolist() == [n_s, 0]
    d1, c1, p1 = ops.ensemble_distances(xd[:1].contiguous(), yd[:1].contiguous())
    assert torch.equal(bits64(d1[0]), bits64(d3[0])) and torch.equal(c1[0], c3[0]) and torch.equal(p1[0], p3[0])
    dn, cn, pn = ops.ensemble_distances(xd)
    assert dn.shape == (3, S, S) and torch.equal(bits64(dn), bits64(d3[:, :S, :S])) and torch.equal(cn, c3)
    assert pn[:, 1].tolist() == [-1] * 3 and torch.equal(pn[:, 0], p3[:, 0])


@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_distances_are_bit_exact_on_integers(S, n_s):
    """integer-valued rows, |value| <= 2^10: every partial sum is an integer below 2^53, so the device matrix equals int64 arithmetic
    bit for bit whatever the order: pair indexing and tile edges with no tolerance"""
    x, y = draw_int(S, n_s, seed=S + n_s)
    want = exact_int(x, y)
    xd, yd = torch.from_numpy(x)[None].to(DEV), torch.from_numpy(y)[None].to(DEV)
    d2, counts, pick = ops.ensemble_distances(xd, yd)
    assert np.array_equal(d2[0].cpu().numpy().view(np.int64), want.astype(np.float64).view(np.int64))
    assert counts[0].tolist() == [n_s, 0] and tuple(pick[0].tolist()) == picks(want, S, True)
    bare = ops.ensemble_distances(xd)[0]
    assert np.array_equal(bare[0].cpu().numpy().view(np.int64), want[:S, :S].astype(np.float64).view(np.int64))


def test_identities_against_the_scores_on_the_device():
    """S = 5, members y + 5 k, small integers: the sums of ops.ensemble_scores are exact there (tests/test_ensemble_dist_cpu.py), so
    sum_{i<j} d2[i][j] == S (S - 1) sum v and sum_i d2[i][S] == S sum e + (S - 1) sum v hold as equalities between the two kernels"""
    S, n = 5, 1028
    rng = np.random.default_rng(5)
    y = rng.integers(-20, 21, (2, n)).astype(np.float32)
    x = (y[:, None] + 5 * rng.integers(-6, 7, (2, S, n))).astype(np.float32)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    sums = ops.ensemble_scores(xd, yd)[0].cpu()
    d2 = ops.ensemble_distances(xd, yd)[0].cpu()
    for b in range(2):
        sum_e, sum_v = float(sums[b, 1]), float(sums[b, 2])
        assert sum(float(d2[b, i, j]) for i in range(S) for j in range(i + 1, S)) == S * (S - 1) * sum_v
        assert sum(float(d2[b, i, S]) for i in range(S)) == S * sum_e + (S - 1) * sum_v


@pytest.mark.parametrize("S", [2, 16, 17])
def test_distances_do_not_depend_on_the_batch_or_the_run(S):
    n_s = 64 * 1024 + 4
    x, y, _ = case(S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    d2, counts, pick = ops.ensemble_distances(xd, yd)
    again = ops.ensemble_distances(xd, yd)
    assert torch.equal(bits64(d2), bits64(again[0])) and torch.equal(counts, again[1]) and torch.equal(pick, again[2])
    for b in range(B_MAX):
        one = ops.ensemble_distances(xd[b:b + 1].contiguous(), yd[b:b + 1].contiguous())
        assert torch.equal(bits64(one[0][0]), bits64(d2[b])) and torch.equal(one[1][0], counts[b]) and torch.equal(one[2][0], pick[b])


# ---- 2. invalid pixels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 16, 17])
def test_invalid_pixels_add_to_no_pair(S):
    n_s = 1028
    x, y, _ = case(S, n_s)
    x, y = x.clone(), y.clone()
    x[0, S // 2, 5] = float("nan")      # a NaN member
    x[0, 0, 1027] = float("inf")        # an infinite member, in the last pixel
    y[0, 300] = float("-inf")           # an infinite target
    y[1, 7] = float("nan")
    x[1, S - 1, 7] = float("nan")       # both in one pixel: counted once
    x[2] = float("nan")                 # no valid pixel at all
    bad = {0: [5, 300, 1027], 1: [7]}
    d2, counts, pick = ops.ensemble_distances(x.to(DEV), y.to(DEV))
    for b in range(2):
        em = emulate(x[b].numpy(), y[b].numpy())
        assert np.nonzero(~em["valid"])[0].tolist() == bad[b] and counts[b].tolist() == [n_s - len(bad[b]), len(bad[b])]
        check_image(em, d2[b].cpu(), counts[b].cpu(), pick[b].cpu(), S, 1, f"invalid S={S} image {b}")
        assert torch.isfinite(d2[b]).all()
    assert counts[2].tolist() == [0, n_s] and not bits64(d2[2]).any() and pick[2].tolist() == [0, 0]
    # without the target its pixels do not decide: image 0 loses pixels 5 and 1027 only
    dn, cn, pn = ops.ensemble_distances(x.to(DEV))
    assert cn[0].tolist() == [n_s - 2, 2] and pn[0, 1].item() == -1
    check_image(emulate(x[0].numpy()), dn[0].cpu(), cn[0].cpu(), pn[0].cpu(), S, 0, f"invalid, no target, S={S}")


# ---- 3. the picks and the row copy ---------------------------------------------------------------------------------------------------
def test_duplicated_members_pick_the_lower_index():
    S, n_s = 6, 1028
    x, y, _ = case(5, n_s)
    x = torch.cat([x, x[:, 1:2]], dim=1).contiguous()  # member 5 is member 1
    x[:, 3] = x[:, 1]
    d2, _, pick = ops.ensemble_distances(x.to(DEV), y.to(DEV))
    for b in range(B_MAX):
        assert float(d2[b, 1, 3]) == 0.0 and float(d2[b, 1, 5]) == 0.0 and torch.equal(bits64(d2[b, 1]), bits64(d2[b, 3]))
        assert pick[b, 0].item() not in (3, 5) and pick[b, 1].item() not in (3, 5)
        assert tuple(pick[b].tolist()) == picks(d2[b].cpu().numpy(), S, True)
    same = torch.zeros(1, 4, 8).to(DEV)
    assert ops.ensemble_distances(same, torch.ones(1, 8).to(DEV))[2].tolist() == [[0, 0]]


def test_pick_rows_copies_bits_and_never_reads_out_of_range():
    B, S, n_s = 4, 5, 64 * 1024 + 4
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, S, n_s), generator=g, dtype=torch.int64).to(torch.int32)  # every bit pattern: NaN payloads too
    raw[:, :, 0] = -2 ** 31                    # -0.0
    raw[:, :, 1] = 0x7fa00001                  # a signalling NaN with a payload
    x = raw.view(torch.float32).to(DEV)
    table = torch.tensor([[0, -1, 4], [4, S, 2], [2, 2 ** 31 - 1, 0], [3, -2 ** 31, 1]], dtype=torch.int32).to(DEV)
    for col in (0, 2):
        n0 = ops.launch_count()
        out = ops.ensemble_pick_rows(x, table, col)
        assert ops.launch_count() == n0 + 1 and out.shape == (B, n_s) and out.dtype == torch.float32
        want = torch.stack([x[b, int(table[b, col])] for b in range(B)])
        assert torch.equal(bits(out), bits(want))
    out = ops.ensemble_pick_rows(x, table, 1)
    assert bool((bits(out) == QNAN).all())
    small = ops.ensemble_pick_rows(x[:, :, :4].contiguous(), table, 0)  # one float4 group
    assert torch.equal(bits(small), bits(torch.stack([x[b, int(table[b, 0]), :4] for b in range(B)])))
    shaped = ops.ensemble_pick_rows(x[:, :, :4096].reshape(B, S, 1, 64, 64).contiguous(), table, 2)
    assert shaped.shape == (B, 1, 64, 64)
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_pick_rows(x, table, 3)
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_pick_rows(x, table.to(torch.int64), 0)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, S, n_s = 2, 4, 64
    x = torch.randn(B, S, n_s + 4, device=DEV)[:, :, :n_s].contiguous()
    y = torch.randn(B, n_s, device=DEV)
    x0, y0 = x.clone(), y.clone()
    big = torch.randn(1, 65, 4, device=DEV)
    canary = dict(d2=torch.full((B, 66, 66), 7.0, device=DEV, dtype=torch.float64), counts=torch.full((B, 2), 7, device=DEV, dtype=torch.int32),
                  pick=torch.full((B, 2), 7, device=DEV, dtype=torch.int32), out=torch.full((B, n_s), 7.0, device=DEV),
                  ws=torch.full((int(lib.idiff_ensemble_distances_ws_bytes(B, 64, 1)) // 8,), 7.0, device=DEV, dtype=torch.float64))
    ptr = {k: t.data_ptr() for k, t in canary.items()}
    xp, yp = x.data_ptr(), y.data_ptr()

    def call(xp_, yp_, B_, S_, n, d2=ptr["d2"], counts=ptr["counts"], pick=ptr["pick"], ws=ptr["ws"]):
        return lib.idiff_ensemble_distances(xp_, yp_, d2, counts, pick, ws, B_, S_, n, None)

    def rows(xp_, pk, stride, out, B_, S_, n):
        return lib.idiff_ensemble_pick_rows(xp_, pk, stride, out, B_, S_, n, None)

    refused = {
        "n_s % 4": lambda: call(xp, yp, B, S, n_s - 2),
        "n_s = 0": lambda: call(xp, yp, B, S, 0),
        "misaligned x": lambda: call(xp + 4, yp, B, S, n_s - 4),
        "misaligned target": lambda: call(xp, yp + 8, B, S, n_s - 4),
        "misaligned d2": lambda: call(xp, yp, B, S, n_s, d2=ptr["d2"] + 4),
        "misaligned ws": lambda: call(xp, yp, B, S, n_s, ws=ptr["ws"] + 4),
        "S = 0": lambda: call(xp, yp, B, 0, n_s),
        "S = 65": lambda: call(big.data_ptr(), yp, 1, 65, 4),
        "B = 0": lambda: call(xp, yp, 0, S, n_s),
        "B = 65536": lambda: call(xp, yp, 65536, S, 4),
        "null x": lambda: call(None, yp, B, S, n_s),
        "null d2": lambda: call(xp, yp, B, S, n_s, d2=None),
        "null counts": lambda: call(xp, yp, B, S, n_s, counts=None),
        "null pick": lambda: call(xp, yp, B, S, n_s, pick=None),
        "null ws": lambda: call(xp, yp, B, S, n_s, ws=None),
        "d2 == x": lambda: call(xp, yp, B, S, n_s, d2=xp),
        "ws == target": lambda: call(xp, yp, B, S, n_s, ws=yp),
        "ws == d2": lambda: call(xp, yp, B, S, n_s, ws=ptr["d2"]),
        "pick == counts": lambda: call(xp, yp, B, S, n_s, pick=ptr["counts"]),
        "pick inside d2": lambda: call(xp, yp, B, S, n_s, pick=ptr["d2"] + 8),
        "counts inside x": lambda: call(xp, yp, B, S, n_s, counts=xp + 16),
        "rows: n_s % 4": lambda: rows(xp, ptr["pick"], 2, ptr["out"], B, S, n_s - 2),
        "rows: S = 0": lambda: rows(xp, ptr["pick"], 2, ptr["out"], B, 0, n_s),
        "rows: S = 65": lambda: rows(xp, ptr["pick"], 2, ptr["out"], 1, 65, 4),
        "rows: stride 0": lambda: rows(xp, ptr["pick"], 0, ptr["out"], B, S, n_s),
        "rows: misaligned x": lambda: rows(xp + 4, ptr["pick"], 2, ptr["out"], B, S, n_s - 4),
        "rows: misaligned out": lambda: rows(xp, ptr["pick"], 2, ptr["out"] + 8, B, S, n_s - 4),
        "rows: misaligned pick": lambda: rows(xp, ptr["pick"] + 2, 2, ptr["out"], B, S, n_s),
        "rows: null pick": lambda: rows(xp, None, 2, ptr["out"], B, S, n_s),
        "rows: null out": lambda: rows(xp, ptr["pick"], 2, None, B, S, n_s),
        "rows: out == x": lambda: rows(xp, ptr["pick"], 2, xp, B, S, n_s),
        "rows: out inside x": lambda: rows(xp, ptr["pick"], 2, xp + 4 * n_s, B, S, n_s),
        "rows: out == pick": lambda: rows(xp, ptr["out"], 2, ptr["out"], B, S, n_s),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert ("ensemble_pick_rows" if what.startswith("rows") else "ensemble_distances") in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert torch.equal(x, x0) and torch.equal(y, y0), what
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_distances(torch.zeros(1, 2, 1, 5, 5, device=DEV), torch.zeros(1, 1, 5, 5, device=DEV))  # n_s % 4 through the wrapper
    with pytest.raises(AssertionError):
        ops.ensemble_distances(torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 4, device=DEV))
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_distances(torch.zeros(1, 2, 8), torch.zeros(1, 8))  # host tensors: there is no CPU path
    assert call(xp, yp, B, S, n_s) == 0  # and the same buffers are accepted as they stand
    assert rows(xp, ptr["pick"], 2, ptr["out"], B, S, n_s) == 0
    torch.cuda.synchronize()
    assert canary["counts"].tolist() == [[n_s, 0]] * B
    med = canary["pick"][:, 0].tolist()
    assert torch.equal(canary["out"], torch.stack([x[b, med[b]] for b in range(B)]))


# ---- 5. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, H = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=4, num_samples=4))
    model.set_eval()
    return model, sde


def test_model_member_distances_and_pick_member(built):
    model, sde = built
    model.feed_data(make_batch(2, H, seed=3))
    model.test(return_samples=True)
    assert model.samples.shape == (2, 4, 1, H, H)
    n0 = ops.launch_count()
    d2, counts, pick = model.member_distances()
    assert ops.launch_count() == n0 + 2  # the two launches of ops.ensemble_distances and nothing else
    want = ops.ensemble_distances(model.samples, model.target)
    assert torch.equal(bits64(d2), bits64(want[0])) and torch.equal(counts, want[1]) and torch.equal(pick, want[2])
    direct = sde.member_distances(model.samples, model.target)
    assert torch.equal(bits64(direct[0]), bits64(d2)) and torch.equal(direct[2], pick)
    for b in range(2):
        em = emulate(model.samples[b].flatten(1).cpu().numpy(), model.target[b].flatten().cpu().numpy())
        check_image(em, d2[b].cpu(), counts[b].cpu(), pick[b].cpu(), 4, 1, f"model image {b}")
    n0 = ops.launch_count()
    medoid = model.pick_member("medoid")
    assert ops.launch_count() == n0 + 1
    best = model.pick_member("best")
    assert ops.launch_count() == n0 + 2 and medoid.shape == best.shape == model.target.shape
    for b in range(2):
        assert torch.equal(bits(medoid[b]), bits(model.samples[b, int(pick[b, 0])]))
        assert torch.equal(bits(best[b]), bits(model.samples[b, int(pick[b, 1])]))
    record = ensemble_distance_summary(d2, counts, 4, True)
    assert record["valid"] == [H * H] * 2 and record["medoid"] == pick[:, 0].tolist() and record["best"] == pick[:, 1].tolist()
    assert all(0 < f < e < m for f, e, m in zip(record["ES_FAIR"], record["ES"], record["RMS_member"]))
    assert all(bst <= med and bst <= mem for bst, med, mem in zip(record["RMS_best"], record["RMS_medoid"], record["RMS_member"]))
    bare = model.member_distances(with_target=False)
    assert bare[0].shape == (2, 4, 4) and bare[2][:, 1].tolist() == [-1, -1] and torch.equal(bits64(bare[0]), bits64(d2[:, :4, :4]))
    n0 = ops.launch_count()
    again = model.pick_member("best")  # the held picks have no best member: the distances are taken again, with the target
    assert ops.launch_count() == n0 + 3 and torch.equal(bits(again), bits(best))
    with pytest.raises(ValueError):
        model.pick_member("mean")
    model.test()  # the members are not kept: nothing to compare
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.member_distances()
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.pick_member("medoid")
    with pytest.raises(ValueError):
        sde.member_distances(model.output, model.target)
    with pytest.raises(ValueError):
        sde.member_distances(torch.zeros(2, 4, 1, H, H, device=DEV), torch.zeros(2, 1, H, H // 2, device=DEV))


NEW_WORDS = ("ES=", "ES_FAIR", "DIVERSITY", "PSNR_best", "PSNR_medoid", "_medoid_")


def test_testum_distances_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {H}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_dist").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "2", "--num-samples", "4", "--sample-T", "4"]
    res = testUM.main(common + ["--distances"])
    out = capsys.readouterr().out
    for word in ("ES=", "ES_FAIR=", "DIVERSITY=", "PSNR_best=", "PSNR_medoid=", "AVG ES:", "AVG ES_FAIR:", "AVG DIVERSITY:", "AVG PSNR_best:",
                 "AVG PSNR_medoid:"):
        assert word in out, word
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2
    for name, v in done.items():
        assert len(v['ES']) == len(v['ES_FAIR']) == len(v['DIVERSITY']) == len(v['PSNR_best']) == len(v['PSNR_medoid']) == v['num']
        assert all(0 < f < e and d > 0 for f, e, d in zip(v['ES_FAIR'], v['ES'], v['DIVERSITY']))
        # the best member is the member of the highest PSNR: no lower than the medoid's or the members' average
        assert all(bst >= med and bst >= mem - 1e-9 for bst, med, mem in zip(v['PSNR_best'], v['PSNR_medoid'], v['PSNR_member']))
        folder = tmp_path / "results" / "drv_dist" / name
        maps = sorted(f for f in os.listdir(folder) if "_medoid_" in f)
        assert len(maps) == v['num'] and all(f.endswith(f"_medoid_{H}x{H}x1.raw") for f in maps)
        assert len(os.listdir(folder)) == 3 * v['num']
        for f in maps:
            m = np.fromfile(folder / f, dtype=np.float32)
            assert m.size == H * H and np.isfinite(m).all()
    # without --distances the driver prints, writes and launches what it did before, with and without --scores
    cfg.write_text(txt.replace("name: drv_dist", "name: drv_plain"))
    n0 = ops.launch_count()
    res = testUM.main(common)
    n_plain = ops.launch_count() - n0
    printed = capsys.readouterr().out.replace(str(tmp_path), "")
    for word in NEW_WORDS:
        assert word not in printed, word
    for name, v in res.items():
        if v['num']:
            assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD'}
            files = os.listdir(tmp_path / "results" / "drv_plain" / name)
            assert len(files) == 2 * v['num'] and not any("_medoid_" in f for f in files)
    cfg.write_text(txt.replace("name: drv_dist", "name: drv_scores"))
    n0 = ops.launch_count()
    res = testUM.main(common + ["--scores"])
    printed = capsys.readouterr().out.replace(str(tmp_path), "")
    assert ops.launch_count() - n0 == n_plain + 2 * 2  # two images, the two launches of the scores each: as before this option existed
    for word in NEW_WORDS:
        assert word not in printed, word
    for name, v in res.items():
        if v['num']:
            assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD', 'CRPS', 'SSR', 'RANK_DEV', 'scores', 'pooled'}
            assert not any("_medoid_" in f for f in os.listdir(tmp_path / "results" / "drv_scores" / name))


def test_testum_distances_needs_an_ensemble(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--distances"])
    assert "num_samples > 1" in capsys.readouterr().err
    assert not (tmp_path / "results").exists()  # before any image ran
