"""Principal modes of an ensemble on the device (idiff_ensemble_modes / idiff_ensemble_project through the C ABI and ops): the solver
against np.linalg.eigh of the emulated centring of the device's own distance matrix, within 4 x the constants the emulation itself
reaches on the host (tests/ensemble_modes_ref.py, tests/test_ensemble_modes_cpu.py); the leading eigenvectors within the Davis-Kahan
bound; the target's coordinates; the projection bit for bit on integers and within the fp64 bound otherwise; unit-norm modes that
reproduce the members; independence of the batch and of the run; degenerate and hostile matrices; the refusals; and the driftSDE /
model / testUM surface."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ensemble_dist_ref import draw  # noqa: E402
from ensemble_modes_ref import (C_EV, C_ORTH, C_RES, EPS, MODE_SEEDS, REL_FLOOR, centre, draw_modes, leading_gaps, project)  # noqa: E402

from instancediff_amd import _lib, ops, pipeline, testUM  # noqa: E402
from instancediff_amd.models.SDEs.driftSDE import driftSDE, ensemble_mode_summary  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
# one float4 group; one group past a 256-thread block; one group past one sweep of the 64 x 256-thread grid of an image
N_S = [4, 1028, 64 * 1024 + 4]
# no pair; one pair; odd with a padding index; the projection's register and re-read forms on both sides of 16; the full 64
S_ALL = [1, 2, 3, 5, 16, 17, 33, 64]
B_MAX = 3
QNAN = 0x7fc00000
MARGIN = 4  # over the emulation's own constants: FMA contraction and the association of a rotation's products, where the kernel may differ


def bits64(t):
    return t.contiguous().view(torch.int64)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def members(kind, S, n_s):
    """(x [3, S, n_s], y [3, n_s]) float32 host tensors: computed once and shared, never modified.  kind "modes": image 0 is the
    draw_modes ensemble of the recorded seed, the others follow it"""
    if kind == "draw":
        pairs = [draw(S, n_s, seed=31337 * S + n_s + b) for b in range(B_MAX)]
    else:
        pairs = [draw_modes(S, n_s, MODE_SEEDS[(S, n_s)])] + [draw_modes(S, n_s, 10 ** 6 + b) for b in range(1, B_MAX)]
    return torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs]))


@functools.lru_cache(maxsize=None)
def device_run(kind, S, n_s):
    """the device's distance matrix of members(kind, S, n_s) with the target and what ops.ensemble_modes makes of it, as host arrays, and
    the float64 eigen-decomposition of the emulated centring of that matrix per image: computed once, shared, never modified"""
    x, y = members(kind, S, n_s)
    d2, counts, _ = ops.ensemble_distances(x.to(DEV), y.to(DEV))
    n0 = ops.launch_count()
    out = ops.ensemble_modes(d2, S, True)
    assert ops.launch_count() == n0 + 1
    names = ("lam", "vec", "coef", "tcoord", "tnorm2", "info")
    for name, t in zip(names, out):
        assert t.is_cuda and t.dtype == (torch.int32 if name == "info" else torch.float64), name
    rec = {name: t.cpu().numpy() for name, t in zip(names, out)}
    rec["d2"], rec["counts"] = d2.cpu().numpy(), counts.cpu().numpy()
    rec["centre"] = [centre(rec["d2"][b], S) for b in range(B_MAX)]
    rec["eigh"] = [np.linalg.eigh(c["G"]) for c in rec["centre"]]
    return rec


def live_count(lam, rel_floor=REL_FLOOR):
    return sum(1 for v in lam if lam[0] > 0 and v > rel_floor * lam[0])


# ---- 1. the solver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_solver_against_eigh(S, n_s):
    """per image: eigenvalue error, residual and orthogonality within MARGIN x (C_EV, C_RES, C_ORTH) x S 2^-52 (the first two relative
    to lam_0); sweeps in [1, 32) -- at S = 1 the matrix is the scalar 0, the contract's degenerate case, whose sweeps is 0 --; the rank
    is the count the device's own lam gives under the stated rule; lam descends; the sign rule holds on every row of vec; coef is
    vec / sqrt(lam) to 2 ulp on the live modes and exactly zero on the dead ones"""
    rec = device_run("draw", S, n_s)
    assert rec["lam"].shape == (3, S) and rec["vec"].shape == (3, S, S) and rec["coef"].shape == (3, S, S) and rec["info"].shape == (3, 2)
    for b in range(B_MAX):
        G = rec["centre"][b]["G"]
        lam, vec, coef = rec["lam"][b], rec["vec"][b], rec["coef"][b]
        rank, sweeps = rec["info"][b].tolist()
        assert rank == live_count(lam) and (np.diff(lam) <= 0).all()
        if S == 1:
            assert (rank, sweeps) == (0, 0) and lam.view(np.int64).tolist() == [0] and vec.tolist() == [[1.0]] and not coef.view(np.int64).any()
            continue
        assert 1 <= sweeps < 32, sweeps
        lam_ref = rec["eigh"][b][0][::-1]
        lam0 = lam_ref[0]
        ev = float(np.abs(lam - lam_ref).max() / lam0) / (S * EPS)
        res = float(np.abs(G @ vec.T - vec.T * lam[None]).max() / lam0) / (S * EPS)
        orth = float(np.abs(vec @ vec.T - np.eye(S)).max()) / (S * EPS)
        print(f"S={S} n_s={n_s} image {b}: sweeps {sweeps}, rank {rank}, eigenvalues {ev:.2f}, residual {res:.2f}, orthogonality {orth:.2f} "
              f"(x S 2^-52; allowed {MARGIN * C_EV}, {MARGIN * C_RES}, {MARGIN * C_ORTH})")
        assert ev <= MARGIN * C_EV and res <= MARGIN * C_RES and orth <= MARGIN * C_ORTH
        for k in range(S):
            big = int(np.argmax(np.abs(vec[k])))  # the first maximum
            assert vec[k, big] > 0, (k, big)
            if k < rank:
                want = vec[k] / math.sqrt(lam[k])
                assert (np.abs(coef[k] - want) <= 2 * np.spacing(np.abs(want))).all(), k
            else:
                assert not coef[k].view(np.int64).any(), k  # +0.0


# ---- 2. the leading eigenvectors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_s", [sn for sn in sorted(MODE_SEEDS) if sn[0] in S_ALL and sn[1] in N_S])
def test_leading_eigenvectors_within_davis_kahan(S, n_s):
    """draw_modes (four separated modes and noise; the seeds' gaps are asserted on the host): each of the min(4, S) leading device
    eigenvectors against eigh's of the same matrix.  With the residual bound of the solver test, Davis-Kahan gives
    sin(angle) <= 4 C_RES S^2 2^-52 lam_0 / gap_k, gap_k from eigh's eigenvalues, and 1 - |<v, w>| = 1 - cos <= sin^2.  The bound lies
    far below 2^-53, where 1 - |<v, w>| cannot be evaluated by a dot product: for unit vectors it equals |v - sign w|^2 / 2, which
    can.  (S, n_s) = (33, 4) and (64, 4) have no seed with such gaps (tests/ensemble_modes_ref.py says why)."""
    rec = device_run("modes", S, n_s)
    w, q = rec["eigh"][0]
    lam_ref, q = w[::-1], q[:, ::-1]
    count = min(4, S)
    gaps = leading_gaps(lam_ref, count)
    assert all(gp >= 0.019 * lam_ref[0] for gp in gaps)  # the device matrix is the host's up to its rounding
    for k in range(count):
        v, ref = rec["vec"][0][k], q[:, k]
        diff = v - (ref if float(v @ ref) >= 0 else -ref)
        got = 0.5 * float(diff @ diff)
        bound = (MARGIN * C_RES * S * S * EPS * lam_ref[0] / gaps[k]) ** 2
        print(f"S={S} n_s={n_s} mode {k}: 1 - |<v, v_eigh>| = {got:.3e}, bound {bound:.3e}, gap / lam_0 = {gaps[k] / lam_ref[0]:.4f}")
        assert got <= bound, k


# ---- 3. the target's coordinates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_target_coordinates(S, n_s):
    """tcoord against the emulation's formula, the index-order sum of vec[k][s] g_s over sqrt(lam_k), on the device's own matrix,
    eigenvectors and eigenvalues (an eigenvector of a close pair moves by far more than a rounding between two correct solvers; the
    sum's own error is what the bound 8 S 2^-52 |g| |v| / sqrt(lam_k) is about); tnorm2 against the emulated centring within
    8 S 2^-52 max d2; tnorm2 and sum lam against ops.ensemble_scores' fp32-per-pixel sum e and (S - 1) sum v to relative 2^-20; and
    without a target +0.0 in both with every other output bit for bit the same"""
    rec = device_run("draw", S, n_s)
    x, y = members("draw", S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    sums = ops.ensemble_scores(xd, yd)[0].cpu().numpy()
    bare = ops.ensemble_modes(ops.ensemble_distances(xd)[0], S, False)
    for b in range(B_MAX):
        c = rec["centre"][b]
        lam, vec, rank = rec["lam"][b], rec["vec"][b], int(rec["info"][b][0])
        for k in range(S):
            if k >= rank:
                assert rec["tcoord"][b].view(np.int64)[k] == 0
                continue
            acc = 0.0
            for s in range(S):
                acc = acc + float(vec[k, s]) * float(c["g"][s])
            want = acc / math.sqrt(lam[k])
            bound = 8 * S * EPS * float(np.linalg.norm(c["g"])) * float(np.linalg.norm(vec[k])) / math.sqrt(lam[k])
            assert abs(rec["tcoord"][b][k] - want) <= bound, (b, k)
        assert abs(rec["tnorm2"][b] - c["tnorm2"]) <= 8 * S * EPS * rec["d2"][b].max()
        assert abs(rec["tnorm2"][b] - sums[b, 1]) <= 2.0 ** -20 * sums[b, 1]
        assert abs(lam.sum() - (S - 1) * sums[b, 2]) <= 2.0 ** -20 * (S - 1) * sums[b, 2]
    assert not bits64(bare[3]).any() and not bits64(bare[4]).any()
    for i in (0, 1, 2, 5):
        name = ("lam", "vec", "coef", "tcoord", "tnorm2", "info")[i]
        assert np.array_equal(bare[i].cpu().numpy().view(np.int64 if i < 5 else np.int32), rec[name].view(np.int64 if i < 5 else np.int32)), name


# ---- 4. the projection alone ------------------------------------------------------------------------------------------------------------
def int_members(S, n_s, seed):
    """integer-valued members with |x| <= 2^10 whose sum over the members is divisible by S at every pixel"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-500, 501, (S, n_s))
    x[S - 1] = rng.integers(-400, 401, n_s)
    x[S - 1] -= x.sum(axis=0) % S
    assert np.abs(x).max() <= 1024 and not (x.sum(axis=0) % S).any()
    return x


@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_projection_is_bit_exact_on_integers(S, n_s):
    """integer members (the mean is an integer), coefficients m / 16 with |m| <= 8: every product and partial sum is a multiple of 1/16
    below 2^20, exact in fp64 and in fp32, so the planes equal int64 arithmetic bit for bit: indexing with no tolerance.  K = 8 and
    K = 1 (its first row), B = 2"""
    xi = np.stack([int_members(S, n_s, seed=S + n_s + b) for b in range(2)])
    rng = np.random.default_rng(S * n_s)
    m = rng.integers(-8, 9, (2, 8, S))
    want = (np.einsum("bks,bsn->bkn", m, xi - xi.sum(axis=1, keepdims=True) // S).astype(np.float64) / 16).astype(np.float32)
    xd = torch.from_numpy(xi.astype(np.float32)).to(DEV)
    cd = torch.from_numpy(m.astype(np.float64) / 16).to(DEV)
    n0 = ops.launch_count()
    got = ops.ensemble_project(xd, cd)
    assert ops.launch_count() == n0 + 1 and got.shape == (2, 8, n_s) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), (want + np.float32(0)).view(np.int32))
    one = ops.ensemble_project(xd, cd[:, :1].contiguous())
    assert one.shape == (2, 1, n_s) and torch.equal(bits(one[:, 0]), bits(got[:, 0]))
    view = ops.ensemble_project(xd, cd[:, :3])  # the leading rows of a larger table, read in place
    assert torch.equal(bits(view), bits(got[:, :3]))


@pytest.mark.parametrize("n_s", N_S)
@pytest.mark.parametrize("S", S_ALL)
def test_projection_against_the_emulation(S, n_s):
    """random float64 coefficients on ensemble_dist_ref.draw: within (S + 2) 2^-53 sum_s |coef_s| |x_s - c| of the emulation (a product's
    rounding where the kernel fuses it, the S sums, and the mean's own rounding) plus half an fp32 ulp of the result; K = 11 through ops
    is two launches whose rows are those of a K = 8 and a K = 3 call; a NaN or an infinite member makes its pixel the quiet NaN in every
    plane and changes nothing else"""
    x, _ = members("draw", S, n_s)
    rng = np.random.default_rng(S + 7 * n_s)
    coef = rng.normal(0, 1, (B_MAX, 11, S))
    xd, cd = x.to(DEV), torch.from_numpy(coef).to(DEV)
    n0 = ops.launch_count()
    got = ops.ensemble_project(xd, cd)
    assert ops.launch_count() == n0 + 2 and got.shape == (B_MAX, 11, n_s)
    lead, rest = ops.ensemble_project(xd, cd[:, :8].contiguous()), ops.ensemble_project(xd, cd[:, 8:].contiguous())
    assert torch.equal(bits(got[:, :8]), bits(lead)) and torch.equal(bits(got[:, 8:]), bits(rest))
    solo = ops.ensemble_project(xd[:1].contiguous(), cd[:1].contiguous())  # B = 1 writes both chunks in place
    assert torch.equal(bits(solo), bits(got[:1]))
    host = got.cpu().numpy()
    for b in range(B_MAX):
        acc, mag, ok = project(x[b].numpy(), coef[b])
        half_ulp = 0.5 * np.maximum(np.spacing(np.abs(host[b])), np.spacing(np.abs(acc).astype(np.float32))).astype(np.float64)
        err, bound = np.abs(host[b].astype(np.float64) - acc), (S + 2) * 2.0 ** -53 * mag + half_ulp
        assert ok.all() and (err <= bound).all(), (b, float((err / bound).max()))
    bad = x.clone()
    spots = {0: [(0, 0), (S - 1, n_s - 1)], 1: [(S // 2, min(777, n_s - 1))]}
    bad[0, 0, 0], bad[0, S - 1, n_s - 1], bad[1, S // 2, min(777, n_s - 1)] = float("nan"), float("inf"), float("-inf")
    hurt = ops.ensemble_project(bad.to(DEV), cd[:, :8].contiguous()).cpu()
    mask = torch.zeros(B_MAX, n_s, dtype=torch.bool)
    for b, where in spots.items():
        for _, pix in where:
            mask[b, pix] = True
    full = mask[:, None].expand(-1, 8, -1)
    assert bool((bits(hurt)[full] == QNAN).all()) and torch.equal(bits(hurt)[~full], bits(lead.cpu())[~full])


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", N_S[1:])
@pytest.mark.parametrize("S", [2, 3, 5, 9])
def test_modes_are_orthonormal_and_reproduce_the_members(S, n_s):
    """driftSDE.principal_modes with K = S - 1, all modes of S <= 9 members in one projection launch: the float64 dot products of the
    float32 mode images are delta_kl within 2^-20 (the planes' fp32 rounding dominates), and x_s - c = sum_k sqrt(lam_k) vec[k][s] u_k
    with a residual whose L2 norm over the pixels is within 2^-20 sqrt(lam_0): the planes' rounding leaves about
    sqrt(sum lam_k) 2^-25 there, so the bound holds a factor of ten.  (n_s = 4 has fewer pixels than modes for S > 5.)"""
    x, y = draw(S, n_s, seed=99 + S)
    xd, yd = torch.from_numpy(x)[None].to(DEV), torch.from_numpy(y)[None].to(DEV)
    n0 = ops.launch_count()
    rec = driftSDE.principal_modes(xd, yd, K=S - 1)
    assert ops.launch_count() == n0 + 4  # two of the distances, the solver, one projection
    assert set(rec) == {"modes", "lam", "vec", "tcoord", "tnorm2", "info", "counts"} and rec["modes"].shape == (1, S - 1, n_s)
    assert rec["info"][0, 0].item() == S - 1 and rec["counts"][0].tolist() == [n_s, 0]
    u = rec["modes"][0].cpu().numpy().astype(np.float64)
    lam, vec = rec["lam"][0].cpu().numpy(), rec["vec"][0].cpu().numpy()
    assert np.abs(u @ u.T - np.eye(S - 1)).max() <= 2.0 ** -20
    r = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    back = (np.sqrt(lam[:S - 1, None]) * vec[:S - 1]).T @ u
    worst = float(np.linalg.norm(back - r, axis=1).max())
    print(f"S={S} n_s={n_s}: reconstruction residual {worst / math.sqrt(lam[0]) * 2 ** 20:.3f} x 2^-20 sqrt(lam_0)")
    assert worst <= 2.0 ** -20 * math.sqrt(lam[0])
    # the target's coordinates are the projections of (y - c) on the mode images
    t = u @ (y.astype(np.float64) - x.astype(np.float64).mean(axis=0))
    assert np.abs(t - rec["tcoord"][0, :S - 1].cpu().numpy()).max() <= 2.0 ** -20 * math.sqrt(float(rec["tnorm2"][0]))


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 16, 17, 64])
def test_results_do_not_depend_on_the_batch_or_the_run(S):
    n_s = N_S[2]
    x, y = members("draw", S, n_s)
    xd, yd = x.to(DEV), y.to(DEV)
    d2 = ops.ensemble_distances(xd, yd)[0]
    first = ops.ensemble_modes(d2, S, True)
    again = ops.ensemble_modes(d2, S, True)
    alone = ops.ensemble_modes(d2[:1].contiguous(), S, True)
    K = min(8, S)
    planes = ops.ensemble_project(xd, first[2][:, :K])
    planes_again = ops.ensemble_project(xd, first[2][:, :K])
    planes_alone = ops.ensemble_project(xd[:1].contiguous(), alone[2][:, :K])
    for i in range(6):
        view = bits64 if i < 5 else bits
        assert torch.equal(view(first[i]), view(again[i])) and torch.equal(view(first[i][0]), view(alone[i][0])), i
    assert torch.equal(bits(planes), bits(planes_again)) and torch.equal(bits(planes[0]), bits(planes_alone[0]))
    last = ops.ensemble_modes(d2[2:].contiguous(), S, True)  # nor on the image's place in the batch
    assert all(torch.equal((bits64 if i < 5 else bits)(first[i][2]), (bits64 if i < 5 else bits)(last[i][0])) for i in range(6))


# ---- 7. degenerate and hostile matrices ----------------------------------------------------------------------------------------------
def assert_degenerate(out, b, S, tnorm2=None):
    lam, vec, coef, tcoord, tn, info = (t[b].cpu() for t in out)
    assert info.tolist() == [0, 0]
    assert not bits64(lam).any() and not bits64(coef).any() and not bits64(tcoord).any()  # +0.0 throughout
    assert torch.equal(vec, torch.eye(S, dtype=torch.float64))
    assert not torch.isnan(tn) and (tnorm2 is None or float(tn) == pytest.approx(tnorm2, rel=4 * EPS))  # (d + .. + d) / S: a rounding or two


def test_degenerate_images_are_no_errors():
    n_s = 1028
    x, y = members("draw", 5, n_s)
    one = ops.ensemble_distances(x[:, :1].contiguous().to(DEV), y.to(DEV))[0]  # S = 1
    out = ops.ensemble_modes(one, 1, True)
    for b in range(B_MAX):
        assert_degenerate(out, b, 1, tnorm2=float(one[b, 0, 1]))
    assert_degenerate(ops.ensemble_modes(one[:, :1, :1].contiguous(), 1, False), 0, 1, tnorm2=0.0)
    x = x.clone()
    x[0] = x[0, 2]            # all members equal
    x[1] = float("nan")       # no valid pixel
    d2, counts, _ = ops.ensemble_distances(x.to(DEV), y.to(DEV))
    out = ops.ensemble_modes(d2, 5, True)
    assert counts[1].tolist() == [0, n_s]
    assert_degenerate(out, 0, 5, tnorm2=float(d2[0, 0, 5]))
    assert_degenerate(out, 1, 5, tnorm2=0.0)
    assert out[5][2].tolist()[0] == 4 and 1 <= out[5][2].tolist()[1] < 32  # the ordinary neighbour
    modes = ops.ensemble_project(x.to(DEV), out[2][:, :4])
    assert not bits(modes[0]).any() and bool((bits(modes[1]) == QNAN).all())  # zero coefficients: zero planes; NaN members: NaN planes


def test_hostile_matrices_are_flagged_alone_and_the_lower_triangle_is_never_read():
    S = 5
    rec = device_run("draw", S, 1028)
    clean = torch.from_numpy(rec["d2"]).to(DEV)
    for i, (value, at) in enumerate([(float("inf"), (0, 1)), (float("nan"), (2, 5)), (-1e-300, (3, 4)), (float("-inf"), (0, 5))]):
        d2 = clean.clone()
        d2[1][at] = value
        out = ops.ensemble_modes(d2, S, True)
        lam, vec, coef, tcoord, tnorm2, info = (t.cpu() for t in out)
        assert info[1].tolist() == [-1, 0], (value, at)
        assert torch.isnan(lam[1]).all() and torch.isnan(tcoord[1]).all() and torch.isnan(tnorm2[1])
        assert not bits64(vec[1]).any() and not bits64(coef[1]).any()
        for b in (0, 2):  # the neighbours are untouched
            for name, t in zip(("lam", "vec", "coef", "tcoord", "tnorm2"), (lam, vec, coef, tcoord, tnorm2)):
                assert np.array_equal(t[b].numpy().view(np.int64), rec[name][b].view(np.int64)), (name, b)
            assert info[b].tolist() == rec["info"][b].tolist()
    junk = clean.clone()
    low = torch.tril_indices(S + 1, S + 1)
    junk[:, low[0], low[1]] = torch.tensor([float("nan"), -7.0, float("inf")], dtype=torch.float64, device=DEV).repeat(7)[:low.shape[1]]
    out = ops.ensemble_modes(junk, S, True)
    for name, t in zip(("lam", "vec", "coef", "tcoord", "tnorm2", "info"), out):
        a = t.cpu().numpy()
        assert np.array_equal(a.view(np.int32 if name == "info" else np.int64), rec[name].view(np.int32 if name == "info" else np.int64)), name


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers():
    lib = _lib.load()
    B, S, n_s, K = 2, 4, 64, 2
    x = torch.randn(B, S, n_s + 4, device=DEV)[:, :, :n_s].contiguous()
    d2 = ops.ensemble_distances(x)[0]
    cf = torch.randn(B, K, S, device=DEV, dtype=torch.float64)
    x0, d20, cf0 = x.clone(), d2.clone(), cf.clone()
    f64 = dict(lam=(B, 65), vec=(B, 65, 65), coef=(B, 65, 65), tcoord=(B, 65), tnorm2=(B + 1,))
    canary = {k: torch.full(shape, 7.0, device=DEV, dtype=torch.float64) for k, shape in f64.items()}
    canary["info"] = torch.full((B, 4), 7, device=DEV, dtype=torch.int32)
    canary["out"] = torch.full((B, 9, n_s + 4), 7.0, device=DEV)
    ptr = {k: t.data_ptr() for k, t in canary.items()}
    ptr.update(d2=d2.data_ptr(), x=x.data_ptr(), cf=cf.data_ptr())

    def modes(B_=B, S_=S, ht=0, floor=2.0 ** -30, **kw):
        a = dict(ptr, **kw)
        return lib.idiff_ensemble_modes(a["d2"], B_, S_, ht, floor, a["lam"], a["vec"], a["coef"], a["tcoord"], a["tnorm2"], a["info"], None)

    def proj(B_=B, S_=S, K_=K, n=n_s, stride=None, **kw):
        a = dict(ptr, **kw)
        return lib.idiff_ensemble_project(a["x"], a["cf"], K_ * S_ if stride is None else stride, a["out"], B_, S_, K_, n, None)

    refused = {
        "S = 0": lambda: modes(S_=0), "S = 65": lambda: modes(S_=65), "B = 0": lambda: modes(B_=0), "B = 65536": lambda: modes(B_=65536),
        "rel_floor = 0": lambda: modes(floor=0.0), "rel_floor = 1": lambda: modes(floor=1.0), "rel_floor NaN": lambda: modes(floor=float("nan")),
        "null d2": lambda: modes(d2=None), "null lam": lambda: modes(lam=None), "null vec": lambda: modes(vec=None),
        "null coef": lambda: modes(coef=None), "null tcoord": lambda: modes(tcoord=None), "null tnorm2": lambda: modes(tnorm2=None),
        "null info": lambda: modes(info=None), "misaligned d2": lambda: modes(d2=ptr["d2"] + 4), "misaligned vec": lambda: modes(vec=ptr["vec"] + 4),
        "misaligned info": lambda: modes(info=ptr["info"] + 4), "vec == coef": lambda: modes(coef=ptr["vec"]), "lam == d2": lambda: modes(lam=ptr["d2"]),
        "tcoord inside vec": lambda: modes(tcoord=ptr["vec"] + 8), "info inside lam": lambda: modes(info=ptr["lam"] + 8),
        "tnorm2 == tcoord": lambda: modes(tnorm2=ptr["tcoord"]),
        "project: S = 0": lambda: proj(S_=0), "project: S = 65": lambda: proj(S_=65), "project: K = 0": lambda: proj(K_=0),
        "project: K = 9": lambda: proj(K_=9), "project: B = 0": lambda: proj(B_=0), "project: B = 65536": lambda: proj(B_=65536),
        "project: n_s % 4": lambda: proj(n=n_s - 2), "project: n_s = 0": lambda: proj(n=0), "project: stride below K S": lambda: proj(stride=K * S - 1),
        "project: null x": lambda: proj(x=None), "project: null coef": lambda: proj(cf=None), "project: null out": lambda: proj(out=None),
        "project: misaligned x": lambda: proj(x=ptr["x"] + 4, n=n_s - 4), "project: misaligned out": lambda: proj(out=ptr["out"] + 8),
        "project: misaligned coef": lambda: proj(cf=ptr["cf"] + 4), "project: out == x": lambda: proj(out=ptr["x"]),
        "project: out inside x": lambda: proj(out=ptr["x"] + 4 * n_s), "project: out == coef": lambda: proj(out=ptr["cf"]),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert ("ensemble_project" if what.startswith("project") else "ensemble_modes") in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
        for name, t in canary.items():
            assert bool((t == 7).all()), (what, name)
        assert torch.equal(x, x0) and torch.equal(bits64(d2), bits64(d20)) and torch.equal(cf, cf0), what
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_modes(d2, S, False, rel_floor=1.5)
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_modes(d2.float(), S, False)
    with pytest.raises(AssertionError):
        ops.ensemble_modes(d2, S, True)  # the matrix has no target row
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_project(torch.zeros(1, 2, 1, 5, 5, device=DEV), torch.zeros(1, 1, 2, device=DEV, dtype=torch.float64))  # n_s % 4
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_project(x, cf.float())
    with pytest.raises(AssertionError):
        ops.ensemble_project(x, cf[:, :, :3].contiguous())
    assert modes() == 0 and proj() == 0  # and the same buffers are accepted as they stand
    torch.cuda.synchronize()
    want = ops.ensemble_modes(d2, S, False)
    assert torch.equal(bits64(canary["lam"].flatten()[:B * S]), bits64(want[0].flatten()))
    assert torch.equal(bits(canary["info"].flatten()[:B * 2]), bits(want[5].flatten()))
    assert torch.equal(bits(canary["out"].flatten()[:B * K * n_s]), bits(ops.ensemble_project(x, cf).flatten()))
    assert bool((canary["out"].flatten()[B * K * n_s:] == 7).all()) and bool((canary["lam"].flatten()[B * S:] == 7).all())


# ---- 9. driftSDE, the model, testUM --------------------------------------------------------------------------------------------------
T, H = 10, 32


@pytest.fixture(scope="module")
def built():
    model, sde = pipeline.build(phase="test", device=torch.device(DEV), T=T, seed=0, sde_overrides=dict(sample_T=4, num_samples=4))
    model.set_eval()
    return model, sde


def test_model_principal_modes_and_traversal(built):
    model, sde = built
    model.feed_data(make_batch(2, H, seed=3))
    model.test(return_samples=True)
    assert model.samples.shape == (2, 4, 1, H, H) and model.output_modes is None
    n0 = ops.launch_count()
    rec = model.principal_modes()
    assert ops.launch_count() == n0 + 4  # the distances' two launches, the solver, one projection: nothing else
    assert rec["modes"].shape == (2, 4, 1, H, H) and model.output_modes is rec["modes"] and rec["modes"].is_cuda
    direct = sde.principal_modes(model.samples, model.target, K=4)
    for key in rec:
        assert torch.equal(rec[key].contiguous().view(torch.uint8), direct[key].contiguous().view(torch.uint8)), key
    assert rec["info"][:, 0].tolist() == [3, 3] and not bits(rec["modes"][:, 3]).any()  # four members span three modes; the fourth image is zero
    u = rec["modes"][:, :3].flatten(2).double()
    assert (torch.bmm(u, u.transpose(1, 2)) - torch.eye(3, device=DEV, dtype=torch.float64)).abs().max().item() <= 2.0 ** -20
    one = ensemble_mode_summary(rec["lam"], rec["tcoord"], rec["tnorm2"], rec["info"], rec["counts"], 4, True)
    assert one["valid"] == [H * H] * 2 and all(1 <= e <= 3 for e in one["EFF_MODES"]) and all(0 <= s <= 1 + 1e-9 for s in one["SPAN_SHARE"])
    assert all(sum(e[:3]) == pytest.approx(1.0) and e[0] >= e[1] >= e[2] for e in one["EXPLAINED"]) and all(z > 0 for z in one["MODE_Z_RMS"])
    # the variance along the modes is the members' spread: sum lam = (S - 1) sum of the per-pixel variance
    var_sum = (model.output_std.double() ** 2).flatten(1).sum(dim=1)
    assert torch.allclose(rec["lam"].sum(dim=1), 3 * var_sum, rtol=1e-5)
    bare = model.principal_modes(K=2, with_target=False)
    assert bare["modes"].shape == (2, 2, 1, H, H) and not bits64(bare["tcoord"]).any() and torch.equal(bits(bare["modes"]), bits(rec["modes"][:, :2]))
    n0 = ops.launch_count()
    moved = model.mode_traversal(1, 2.0)
    assert ops.launch_count() == n0 + 2 and moved.shape == model.output.shape  # one axpby per image on the held modes
    for b in range(2):
        step = 2.0 * math.sqrt(float(rec["lam"][b, 1]) / 3)
        want = model.output[b].double() + step * rec["modes"][b, 1].double()
        assert (moved[b].double() - want).abs().max().item() <= 2.0 ** -22 * (1 + step)
    assert torch.equal(bits(model.mode_traversal(0, 0.0)), bits(model.output))
    n0 = ops.launch_count()
    third = model.mode_traversal(2, -1.0)  # beyond the held K = 2: the modes are taken again
    assert ops.launch_count() == n0 + 4 + 2 and not torch.equal(third, model.output)
    for k in (4, -1, 1.5):
        with pytest.raises(ValueError):
            model.mode_traversal(k, 1.0)
    model.test()  # the members are not kept: nothing to decompose
    assert model.output_modes is None
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.principal_modes()
    with pytest.raises(ValueError, match="return_samples=True.*num_samples"):
        model.mode_traversal(0, 1.0)
    with pytest.raises(ValueError):
        sde.principal_modes(model.output, model.target)
    with pytest.raises(ValueError):
        sde.principal_modes(torch.zeros(2, 4, 1, H, H, device=DEV), torch.zeros(2, 1, H, H // 2, device=DEV))
    with pytest.raises(ValueError):
        sde.principal_modes(torch.zeros(2, 4, 1, H, H, device=DEV), K=0)


NEW_WORDS = ("EFF_MODES", "EXPLAINED_1", "SPAN_SHARE", "MODE_Z_RMS", "_modes_", "modes pooled")


def test_testum_modes_option(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    assert "image_size: 64" in txt and "T: 100" in txt
    txt = txt.replace("image_size: 64", f"image_size: {H}").replace("T: 100", f"T: {T}")
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_modes").replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    common = ["-opt", str(cfg), "--random-init", "--limit", "2", "--num-samples", "4", "--sample-T", "4"]
    n0 = ops.launch_count()
    res = testUM.main(common + ["--modes"])
    n_modes = ops.launch_count() - n0
    out = capsys.readouterr().out
    for word in ("EFF_MODES=", "EXPLAINED_1=", "SPAN_SHARE=", "MODE_Z_RMS=", "modes pooled over", "EFF_MODES:", "MODE_Z_RMS:"):
        assert word in out, word
    done = {k: v for k, v in res.items() if v['num']}
    assert sum(v['num'] for v in done.values()) == 2
    for name, v in done.items():
        assert len(v['EFF_MODES']) == len(v['EXPLAINED_1']) == len(v['SPAN_SHARE']) == len(v['MODE_Z_RMS']) == v['num']
        assert all(1 <= e <= 3 for e in v['EFF_MODES']) and all(1 / 3 <= e <= 1 for e in v['EXPLAINED_1'])
        assert all(0 <= s <= 1 + 1e-9 for s in v['SPAN_SHARE']) and all(z > 0 for z in v['MODE_Z_RMS'])
        folder = tmp_path / "results" / "drv_modes" / name
        maps = sorted(f for f in os.listdir(folder) if "_modes_" in f)
        assert len(maps) == v['num'] and all(f.endswith(f"_modes_{H}x{H}x4.raw") for f in maps)
        assert len(os.listdir(folder)) == 3 * v['num'] + 1  # the triptych, the std map, the modes; and modes.json
        for f in maps:
            m = np.fromfile(folder / f, dtype=np.float32).reshape(4, H * H).astype(np.float64)
            assert np.abs(m[:3] @ m[:3].T - np.eye(3)).max() <= 2.0 ** -20 and not m[3].any()
        rec = json.load(open(folder / "modes.json"))
        assert rec["S"] == 4 and rec["K"] == 4 and rec["images"] == v['num'] and rec["refused"] == 0 and len(rec["EXPLAINED"]) == 4
        assert rec["EFF_MODES"] == v['pooled_modes']['EFF_MODES'] and 1 <= rec["EFF_MODES"] <= 3 and rec["valid"] == v['num'] * H * H
    # without --modes the driver prints, writes and launches what it did before
    cfg.write_text(txt.replace("name: drv_modes", "name: drv_plain"))
    n0 = ops.launch_count()
    res = testUM.main(common)
    n_plain = ops.launch_count() - n0
    assert n_modes == n_plain + 2 * 4  # two images: the distances' two launches, the solver and one projection each
    printed = capsys.readouterr().out.replace(str(tmp_path), "")
    for word in NEW_WORDS:
        assert word not in printed, word
    for name, v in res.items():
        if v['num']:
            assert set(v) == {'num', 'RMSE', 'SSIM', 'PSNR', 'PSNR_member', 'STD'}
            files = os.listdir(tmp_path / "results" / "drv_plain" / name)
            assert len(files) == 2 * v['num'] and not any("modes" in f for f in files)
    cfg.write_text(txt.replace("name: drv_modes", "name: drv_two"))
    res = testUM.main(common + ["--modes", "2"])
    capsys.readouterr()
    for name, v in res.items():
        if v['num']:
            maps = [f for f in os.listdir(tmp_path / "results" / "drv_two" / name) if "_modes_" in f]
            assert len(maps) == v['num'] and all(f.endswith(f"_modes_{H}x{H}x2.raw") for f in maps)


def test_testum_modes_needs_an_ensemble(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--modes"])
    assert "num_samples > 1" in capsys.readouterr().err
    assert not (tmp_path / "results").exists()  # before any image ran
