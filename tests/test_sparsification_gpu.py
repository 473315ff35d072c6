"""Sparsification curves on the device (idiff_sparsification through the C ABI and ops.sparsification): counts and thresholds bit for bit
against the numpy emulation of the contract (tests/sparsification_ref.py), the fp64 sums bit for bit where every partial sum is exact and
within the bound of two fp64 sums elsewhere, every key population the selection can trip on, the oracle, independence of the batch and of
the run, the refusals, and the driftSDE / model / testUM surface."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sparsification_ref import close, emulate, squared_error, summary  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import sparsification_summary  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
# one float4; two; short of one 256-thread block; one sweep of the selection's 1024 threads; one float4 past a sweep of the sums' 64 x 256
# grid (and 16 sweeps of the selection); the smallest image the nets take, squared up
N_S = [4, 8, 252, 1024, 4 * 64 * 256 + 4, 48 * 48]
K_ALL = [1, 2, 3, 8, 9, 20, 64]  # 8 and 9 straddle a register group of eight thresholds
NAN, INF = float("nan"), float("inf")


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def population(name, n, seed):
    """(key, pred, target) float32 [n] on the host.  `exact` populations have integer pred - target in [-8, 8]: every fp64 partial sum of
    e is an integer below 2^53, so the sums are the same in any order."""
    rng = np.random.default_rng(seed)
    target = rng.integers(-4, 5, n).astype(np.float32)
    pred = rng.integers(-4, 5, n).astype(np.float32)
    if name == "float":  # distinct keys, rounded errors
        key = rng.normal(0, 1, n).astype(np.float32)
        pred = (target + rng.normal(0, 0.3, n)).astype(np.float32)
    elif name == "ties":  # 33 levels: long tie groups at every threshold from n = 252 on
        key = (np.round(rng.normal(0, 1, n) * 4) / 4).astype(np.float32)
    elif name == "equal":  # one tie group holds every threshold
        key = np.full(n, 0.75, dtype=np.float32)
    elif name == "low_byte":  # decided in the last pass only
        key = (np.uint32(0x3f800000) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    elif name == "high_byte":  # decided in the first pass; both signs; bit 23 clear, so no exponent is all ones
        key = ((rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32)
    elif name == "mixed":  # both signs with +-0, +-inf and denormals
        key = rng.normal(0, 1, n).astype(np.float32)
        special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff], dtype=np.uint32)
        where = rng.random(n) < 0.5
        key[where] = special[rng.integers(0, len(special), int(where.sum()))].view(np.float32)
    elif name == "nans":  # NaN in the key only, in pred only, in target only, inf - inf, and all at once
        key = (np.round(rng.normal(0, 1, n) * 4) / 4).astype(np.float32)
        kind = rng.integers(0, 8, n)
        key[kind == 0] = NAN
        pred[kind == 1] = NAN
        target[kind == 2] = NAN
        pred[kind == 3], target[kind == 3] = INF, INF
        key[kind == 4], pred[kind == 4], target[kind == 4] = np.uint32(0xffc00001).view(np.float32), NAN, NAN
    elif name == "none_valid":
        key = np.full(n, NAN, dtype=np.float32)
    elif name == "inf_error":  # an infinite e among the highest keys and one among the lowest: non-finite sums, finite counts
        key = rng.permutation(n).astype(np.float32)
        pred[int(np.argmax(key))] = INF
        target[int(np.argmin(key))] = -INF
    else:
        raise KeyError(name)
    return key, pred, target


POPULATIONS = ["float", "ties", "equal", "low_byte", "high_byte", "mixed", "nans", "none_valid", "inf_error"]
EXACT = {"ties", "equal", "low_byte", "high_byte", "mixed", "nans", "none_valid"}


@functools.lru_cache(maxsize=None)
def case(name, n, seed=0):
    """the population on the host and its emulation per K (computed on demand, shared, never modified)"""
    key, pred, target = population(name, n, 1000 * POPULATIONS.index(name) + n + seed)
    return key, pred, target, {}


def emulation(name, n, K, seed=0):
    key, pred, target, cache = case(name, n, seed)
    if K not in cache:
        cache[K] = emulate(key, pred, target, K)
    return cache[K]


def dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def check_image(em, K, n_s, sums, counts, tau, exact, what):
    """one image's device results (host tensors) against its emulation"""
    assert counts.tolist() == em["counts"].tolist(), what
    assert np.array_equal(bits32(tau.numpy()), em["tau"]), what  # bit for bit, NaN sentinels included
    got, want = sums.numpy(), em["sums"]
    assert not np.signbit(got).any(), what  # empty sums are +0.0
    if exact:
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), what
        return
    # two fp64 sums of n non-negative terms in different orders differ by at most 2 (n - 1) 2^-53 times the sum; a non-finite sum is equal
    worst = 0.0
    for k in range(K + 1):
        for col in range(2):
            g, w = float(got[k, col]), float(want[k, col])
            if not np.isfinite(w):
                assert g == w, (what, k, col, g, w)
                continue
            bound = 2 * n_s * 2.0 ** -53 * w
            assert abs(g - w) <= bound, (what, k, col, g, w, bound)
            worst = max(worst, abs(g - w) / bound if bound else 0.0)
    print(f"{what}: worst |sum - host| / bound {worst:.3f}")


def run(key, pred, target, K):
    sums, counts, tau = ops.sparsification(*dev(key, pred, target), K)
    return sums.cpu(), counts.cpu(), tau.cpu()


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
def test_against_the_emulation_over_sizes_and_K(n_s):
    """B = 3 (rounded errors and distinct keys; integer errors and tied keys; integer errors and one key) at every K, and image 1 alone
    at B = 1 bit for bit.  At n_s = 4 and 8, N < K from K = 8 on: repeated sentinels and repeated thresholds."""
    names = ["float", "ties", "equal"]
    key, pred, target = (np.stack([case(nm, n_s)[i] for nm in names]) for i in range(3))
    for K in K_ALL:
        sums, counts, tau = run(key, pred, target, K)
        assert sums.dtype == torch.float64 and sums.shape == (3, K + 1, 2)
        assert counts.dtype == torch.int32 and counts.shape == (3, K + 1, 2)
        assert tau.dtype == torch.float32 and tau.shape == (3, K)
        for b, nm in enumerate(names):
            em = emulation(nm, n_s, K)
            check_image(em, K, n_s, sums[b], counts[b], tau[b], nm in EXACT, f"n_s={n_s} K={K} {nm}")
            assert counts[b, K].tolist() == [n_s, 0]
            if n_s < K:
                assert int((em["m"] == 0).sum()) > 1 and np.isnan(tau[b].numpy()[em["m"] == 0]).all()
        s1, c1, t1 = run(key[1:2], pred[1:2], target[1:2], K)
        assert torch.equal(s1[0].view(torch.int64), sums[1].view(torch.int64)) and torch.equal(c1[0], counts[1])
        assert torch.equal(t1[0].view(torch.int32), tau[1].view(torch.int32))


# ---- 2. key populations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POPULATIONS)
def test_key_populations(name):
    """every population at 252 pixels (one block of the sums launch has work) and at 48 x 48 (nine have), with K below, at and above a
    register group of eight thresholds and at the limit"""
    for n_s in (252, 48 * 48):
        key, pred, target, _ = case(name, n_s)
        for K in (3, 8, 9, 64):
            em = emulation(name, n_s, K)
            sums, counts, tau = run(key[None], pred[None], target[None], K)
            check_image(em, K, n_s, sums[0], counts[0], tau[0], name in EXACT, f"{name} n_s={n_s} K={K}")
            N, invalid = counts[0, K].tolist()
            assert N + invalid == n_s
            if name == "none_valid":
                assert N == 0 and not sums.any() and not counts[0, :K].any() and np.isnan(tau.numpy()).all()
            if name == "nans":
                assert 0 < invalid < n_s and torch.isfinite(sums).all()
            if name == "inf_error":
                assert invalid == 0 and sums[0, K, 0] == INF and sums[0, 1, 0] == INF and torch.isfinite(sums[0, 1:K, 1]).all()
            if name == "equal":
                assert counts[0, 1:K, 0].tolist() == [0] * (K - 1) and counts[0, 1:K, 1].tolist() == [n_s] * (K - 1)


def test_mixed_population_holds_what_it_is_about():
    key = case("mixed", 48 * 48)[0]
    b = bits32(key)
    for special in (0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001):
        assert (b == special).any(), hex(special)
    em = emulation("mixed", 48 * 48, 64)
    assert (em["tau"] != 0x80000000).all()  # a threshold on a zero is +0


# ---- 3. the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["float", "nans", "inf_error"])
def test_the_oracle_is_the_error_as_key(name):
    n_s = 48 * 48
    _, pred, target, _ = case(name, n_s)
    e = squared_error(pred, target)
    for K in (9, 20):
        none = run(None, pred[None], target[None], K)
        as_key = run(e[None], pred[None], target[None], K)
        assert torch.equal(none[0].view(torch.int64), as_key[0].view(torch.int64)) and torch.equal(none[1], as_key[1])
        assert torch.equal(none[2].view(torch.int32), as_key[2].view(torch.int32))
        em = emulate(None, pred, target, K)
        check_image(em, K, n_s, none[0][0], none[1][0], none[2][0], False, f"oracle {name} K={K}")


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
def test_an_image_does_not_depend_on_the_batch_or_the_run():
    n_s = 4 * 64 * 256 + 4
    names = ["float", "mixed", "nans"]
    key, pred, target = (np.stack([case(nm, n_s)[i] for nm in names]) for i in range(3))
    for K in (9, 64):
        first = run(key, pred, target, K)
        again = run(key, pred, target, K)
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32), b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
        for b, nm in enumerate(names):
            s1, c1, t1 = run(key[b:b + 1], pred[b:b + 1], target[b:b + 1], K)
            assert torch.equal(s1[0].view(torch.int64), first[0][b].view(torch.int64)), (K, nm)
            assert torch.equal(c1[0], first[1][b]) and torch.equal(t1[0].view(torch.int32), first[2][b].view(torch.int32)), (K, nm)
            check_image(emulation(nm, n_s, K), K, n_s, s1[0], c1[0], t1[0], nm in EXACT, f"alone {nm} K={K}")


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, K, n_s = 2, 8, 64
    key, pred, target = (torch.randn(B, n_s + 4, device=DEV) for _ in range(3))
    held = [t.clone() for t in (key, pred, target)]
    canary = dict(sums=torch.full((B, 66, 2), 7.0, device=DEV, dtype=torch.float64), counts=torch.full((B, 66, 2), 7, device=DEV, dtype=torch.int32),
                  tau=torch.full((B, 65), 7.0, device=DEV),
                  ws=torch.full((int(lib.idiff_sparsification_ws_bytes(B, 64, n_s)) // 8 + 1,), 7.0, device=DEV, dtype=torch.float64))

    def call(kp, pp, tp, K_, n, B_=B, sums=None, counts=None, tau=None, ws=None):
        return lib.idiff_sparsification(kp, pp, tp, K_, sums or canary["sums"].data_ptr(), counts or canary["counts"].data_ptr(),
                                        tau or canary["tau"].data_ptr(), ws or canary["ws"].data_ptr(), B_, n, None)

    kp, pp, tp = key.data_ptr(), pred.data_ptr(), target.data_ptr()
    refused = {
        "K = 0": lambda: call(kp, pp, tp, 0, n_s),
        "K = 65": lambda: call(kp, pp, tp, 65, n_s),
        "n_s = 6": lambda: call(kp, pp, tp, K, 6),
        "n_s = 0": lambda: call(kp, pp, tp, K, 0),
        "misaligned key": lambda: call(kp + 4, pp, tp, K, n_s),
        "misaligned pred": lambda: call(kp, pp + 8, tp, K, n_s),
        "misaligned ws": lambda: call(kp, pp, tp, K, n_s, ws=canary["ws"].data_ptr() + 4),
        "sums inside ws": lambda: call(kp, pp, tp, K, n_s, sums=canary["ws"].data_ptr() + 64),
        "tau inside counts": lambda: call(kp, pp, tp, K, n_s, tau=canary["counts"].data_ptr() + 8),
        "counts on target": lambda: call(kp, pp, tp, K, n_s, counts=tp),
        "tau on key": lambda: call(kp, pp, tp, K, n_s, tau=kp),
        "B = 0": lambda: call(kp, pp, tp, K, n_s, B_=0),
        "B = 65536": lambda: call(kp, pp, tp, K, 4, B_=65536),
        "no pred": lambda: call(kp, None, tp, K, n_s),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert "sparsification" in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert all(torch.equal(a, b) for a, b in zip((key, pred, target), held)), what
    with pytest.raises(_lib.IdiffError):
        ops.sparsification(None, torch.zeros(1, 1, 5, 5, device=DEV), torch.zeros(1, 1, 5, 5, device=DEV))  # n_s % 4 through the wrapper
    with pytest.raises(_lib.IdiffError):
        ops.sparsification(None, torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV), K=65)
    with pytest.raises(_lib.IdiffError):
        ops.sparsification(None, torch.zeros(1, 8), torch.zeros(1, 8))  # host tensors
    with pytest.raises(AssertionError):
        ops.sparsification(torch.zeros(1, 4, device=DEV), torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV))
    n0 = ops.launch_count()
    assert call(kp, pp, tp, K, n_s) == 0  # the same buffers are accepted as they stand (rows of n_s: the tensors' first 2 * 64 floats)
    torch.cuda.synchronize()
    assert ops.launch_count() == n0 + 3
    assert canary["counts"].view(-1)[:B * (K + 1) * 2].view(B, K + 1, 2)[:, K].tolist() == [[n_s, 0]] * B


# ---- 6. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, H = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=2, num_samples=4))
    model.set_eval()
    return model, sde


def host_records(sums, counts):
    return [dict(sums=s.cpu().numpy(), counts=c.cpu().numpy()) for s, c in zip(sums, counts)]


def test_model_sparsification(built):
    model, sde = built
    model.feed_data(make_batch(2, H, seed=3))
    model.test(return_samples=True)
    K = 8
    n0 = ops.launch_count()
    sums, counts, sums_o, counts_o, tau = model.sparsification(K=K)
    assert ops.launch_count() == n0 + 6  # the three launches of the map's call and of the oracle's, nothing else
    out, std, tgt = (t.flatten(1).cpu().numpy() for t in (model.output, model.output_std, model.target))
    for b in range(2):
        check_image(emulate(std[b], out[b], tgt[b], K), K, H * H, sums[b].cpu(), counts[b].cpu(), tau[b].cpu(), False, f"model std image {b}")
        check_image(emulate(None, out[b], tgt[b], K), K, H * H, sums_o[b].cpu(), counts_o[b].cpu(),
                    ops.sparsification(None, model.output, model.target, K)[2][b].cpu(), False, f"model oracle image {b}")
    direct = sde.sparsification(model.output, model.output_std, model.target, K=K)
    for a, b in zip(direct, (sums, counts, sums_o, counts_o, tau)):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32), b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    got = sparsification_summary(sums, counts, sums_o, counts_o, K)
    want = summary(host_records(sums, counts), host_records(sums_o, counts_o), K)
    for name in ("curve", "oracle", "random", "AUSE", "AURG", "AUSE_RMSE", "AURG_RMSE"):
        assert close(got[name], want[name]), name
    assert got["N"] == 2 * H * H and got["invalid"] == 0 and got["AUSE"] >= 0
    # a key that knows the truth ranks better than noise
    crps = sparsification_summary(*model.sparsification(K=K, key="crps")[:4], K)
    noise = ops.randn(tuple(model.output.shape), model.output.device, seed=5)
    rand = sparsification_summary(*sde.sparsification(model.output, noise, model.target, K=K)[:4], K)
    print(f"AUSE: std {got['AUSE']:.4f}, crps {crps['AUSE']:.4f}, noise {rand['AUSE']:.4f}; AURG: std {got['AURG']:.4f}, crps {crps['AURG']:.4f}, "
          f"noise {rand['AURG']:.4f}")
    assert crps["AUSE"] < rand["AUSE"] and crps["AURG"] > rand["AURG"]
    with pytest.raises(ValueError, match="interval"):
        model.sparsification(K=K, key="width")  # no interval maps are held
    with pytest.raises(ValueError, match="key must be"):
        model.sparsification(K=K, key="entropy")
    with pytest.raises(ValueError, match="K must be"):
        model.sparsification(K=65)
    sde.set_interval(0.5)
    try:
        model.test(return_samples=True)
        width = model.sparsification(K=K, key="width")
        w = (model.output_hi - model.output_lo).flatten(1).cpu().numpy()
        out, tgt = (t.flatten(1).cpu().numpy() for t in (model.output, model.target))
        check_image(emulate(w[0], out[0], tgt[0], K), K, H * H, width[0][0].cpu(), width[1][0].cpu(), width[4][0].cpu(), False, "model width image 0")
    finally:
        sde.set_interval(None)
    model.test()  # the members are not kept: nothing to rank by
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.sparsification()
    with pytest.raises(ValueError):
        sde.sparsification(model.output, model.output[:, :, :16], model.target)


NEW_WORDS = ("AUSE", "AURG", "sparsification")


def test_testum_sparsification_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {H}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_sp").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "2", "--num-samples", "4", "--sample-T", "2"]
    res = testUM.main(common + ["--sparsification", "8"])
    out = capsys.readouterr().out
    for word in ("AUSE=", "AURG=", "AUSE_RMSE=", "sparsification pooled over", "AUSE: ", "AURG: ", "AURG_RMSE: ", "invalid: 0"):
        assert word in out, word
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2
    for name, v in done.items():
        assert len(v['AUSE']) == len(v['AURG']) == len(v['AUSE_RMSE']) == v['num']
        assert all(np.isfinite(a) and a >= 0 for a in v['AUSE'])
        recs = [host_records(torch.cat([r[q] for r in v['sparsification']]), torch.cat([r[q + 1] for r in v['sparsification']])) for q in (0, 2)]
        want = summary(recs[0], recs[1], 8)  # the type's images pooled, by the independent restatement
        wrote = json.load(open(tmp_path / "results" / "drv_sp" / name / "sparsification.json"))
        assert set(wrote) == {"S", "K", "fractions", "curve", "oracle", "random", "AUSE", "AURG", "N", "invalid"}
        assert wrote["S"] == 4 and wrote["K"] == 8 and wrote["N"] == v['num'] * H * H and wrote["invalid"] == 0
        assert wrote["fractions"] == [k / 8 for k in range(8)]
        for key in ("curve", "oracle", "random"):  # on RMSE's x/2 + 0.5 scale: a quarter of the [-1, 1] tensors' squared errors, exactly
            assert close(wrote[key], 0.25 * np.asarray(want[key])), key
        assert close(wrote["AUSE"], want["AUSE"]) and close(wrote["AURG"], want["AURG"])
        assert wrote["curve"] == [0.25 * c for c in v['pooled_sparsification']['curve']]
    # without the flag the driver prints and writes what it did before
    cfg.write_text(txt.replace("name: drv_sp", "name: drv_plain"))
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
            assert len(files) == 2 * v['num'] and "sparsification.json" not in files
    cfg.write_text(txt.replace("name: drv_sp", "name: drv_sp2"))
    n0 = ops.launch_count()
    testUM.main(common + ["--sparsification", "8"])
    capsys.readouterr()
    assert ops.launch_count() - n0 == n_plain + 2 * 6  # two images, the map's and the oracle's three launches each: nothing else differs
