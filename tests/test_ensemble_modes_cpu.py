"""Principal modes of an ensemble on the host: the C ABI's new symbols, the Jacobi schedule as the library itself states it
(idiff_ensemble_modes_pair needs no GPU), the centring identity, the emulated solver (tests/ensemble_modes_ref.py) against np.linalg.eigh
-- which is where the constants C_EV / C_RES / C_ORTH of the GPU test's bounds come from --, ensemble_mode_summary against the
definitions, and the refusals of both entry points, which launch nothing."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from ensemble_dist_ref import draw, emulate
from ensemble_modes_ref import (C_EV, C_ORTH, C_RES, EPS, MODE_SEEDS, centre, check_gaps, decompose, draw_modes, gram, jacobi, pooled, project,
                                schedule, summary)

from instancediff_amd import _lib, ops, pipeline, testUM
from instancediff_amd.models.SDEs.driftSDE import ensemble_mode_summary

NEW_SYMBOLS = ["idiff_ensemble_modes", "idiff_ensemble_modes_pair", "idiff_ensemble_project"]
S_GRID = [1, 2, 3, 5, 8, 16, 17, 33, 64]
N_GRID = [4, 1028, 65540]


# ---- 1. the C ABI and the schedule ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == header
    assert ops.ENSEMBLE_PROJECT_MAX_K == 8 and ops.ENSEMBLE_MODES_REL_FLOOR == 2.0 ** -30


def library_schedule(S):
    """the rounds of a sweep as idiff_ensemble_modes_pair gives them: the function the kernel calls"""
    lib = _lib.load()
    Sp = S + (S & 1)
    p, q = ctypes.c_int(-7), ctypes.c_int(-7)
    rounds = []
    for r in range(Sp - 1):
        pairs = []
        for i in range(Sp // 2):
            rc = lib.idiff_ensemble_modes_pair(S, r, i, ctypes.byref(p), ctypes.byref(q))
            assert rc in (0, 1), (S, r, i, rc)
            if rc:
                assert 0 <= p.value < q.value < S, (S, r, i, p.value, q.value)
                pairs.append((p.value, q.value))
            else:
                assert S % 2 == 1 and (p.value, q.value) == (-1, -1)  # only an odd S has a padding index
        rounds.append(pairs)
    return rounds


@pytest.mark.parametrize("S", range(1, 65))
def test_the_schedule_covers_every_pair_once(S):
    rounds = library_schedule(S)
    assert len(rounds) == S + (S & 1) - 1
    seen = []
    for pairs in rounds:
        members = [m for pq in pairs for m in pq]
        assert len(members) == len(set(members)), f"S={S}: a round's pairs share a member"
        assert len(pairs) == S // 2  # an odd S leaves one member out per round
        seen += pairs
    assert sorted(seen) == [(p, q) for p in range(S) for q in range(p + 1, S)]
    assert rounds == schedule(S)  # and the reference's restatement of the header's words is the same schedule


def test_the_schedule_refuses_what_is_out_of_range():
    lib = _lib.load()
    p, q = ctypes.c_int(-7), ctypes.c_int(-7)
    for S, r, i in [(0, 0, 0), (65, 0, 0), (4, 3, 0), (4, -1, 0), (4, 0, 2), (4, 0, -1), (5, 5, 0), (5, 0, 3), (1, 1, 0)]:
        assert lib.idiff_ensemble_modes_pair(S, r, i, ctypes.byref(p), ctypes.byref(q)) == -1, (S, r, i)
        assert "ensemble_modes_pair" in lib.idiff_last_error().decode()
        assert (p.value, q.value) == (-7, -7)
    assert lib.idiff_ensemble_modes_pair(4, 0, 0, None, ctypes.byref(q)) == -1
    assert lib.idiff_ensemble_modes_pair(1, 0, 0, ctypes.byref(p), ctypes.byref(q)) == 0  # S = 1: one round, one padded pair


# ---- 2. the centring identity ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, S, n):
    """(x, y, the distance emulation's matrix with the target row): computed once, shared, never modified"""
    x, y = draw(S, n, seed=7919 * S + n) if kind == "draw" else draw_modes(S, n, MODE_SEEDS[(S, n)])
    return x, y, emulate(x, y)["d2"]


@pytest.mark.parametrize("n", N_GRID)
@pytest.mark.parametrize("S", S_GRID)
def test_centring_identity(S, n):
    """centre(d2) of the distance emulation's matrix against the directly formed (X - c)(X - c)^T, c the members' centroid, the target
    row included: within 8 S 2^-52 lam_0.  At S = 1 lam_0 = 0: the member block and g are exactly 0 there, and tnorm2, which is the one
    distance d2[0][1] itself, is compared within 8 ulp of its own size (the two sums run in different orders)."""
    x, y, d2 = case("draw", S, n)
    got = centre(d2, S)
    rows = np.concatenate([x, y[None]]).astype(np.float64)
    r = rows - rows[:S].mean(axis=0, keepdims=True)
    want = r @ r.T
    lam0 = float(np.linalg.eigvalsh(want[:S, :S])[-1]) if S > 1 else 0.0
    tol = 8 * S * EPS * lam0
    worst = max(np.abs(got["G"] - want[:S, :S]).max(), np.abs(got["g"] - want[S, :S]).max())
    err_t = abs(got["tnorm2"] - want[S, S])
    print(f"S={S} n={n}: worst centring error {max(worst, err_t) / (EPS * lam0) if lam0 else 0.0:.2f} x 2^-52 lam_0")
    assert worst <= tol
    assert err_t <= (tol if S > 1 else 8 * EPS * want[S, S])
    assert np.array_equal(got["G"], got["G"].T)  # h_i + h_j commutes: the matrix is symmetric bit for bit
    garbage = d2.copy()  # only the upper triangle is read
    garbage[np.tril_indices(S + 1)] = np.nan
    again = centre(garbage, S)
    assert np.array_equal(again["G"], got["G"]) and np.array_equal(again["g"], got["g"]) and again["tnorm2"] == got["tnorm2"]
    bare = centre(d2[:S, :S], S)
    assert np.array_equal(bare["G"], got["G"]) and bare["g"] is None and bare["tnorm2"] == 0.0


# ---- 3. the emulated solver against eigh -------------------------------------------------------------------------------------------------
def solver_errors(G, D, V):
    """(eigenvalue error, residual, loss of orthogonality) of a solver's result for the symmetric G, the first two relative to lam_0"""
    lam_ref = np.linalg.eigvalsh(G)[::-1]
    lam = np.sort(np.diag(D))[::-1]
    lam0 = lam_ref[0]
    ev = float(np.abs(lam - lam_ref).max() / lam0)
    res = float(np.abs(G @ V - V * np.diag(D)[None]).max() / lam0)
    orth = float(np.abs(V.T @ V - np.eye(len(G))).max())
    return ev, res, orth


WORST = {}


SOLVER_GRID = [("draw", S, n) for S in S_GRID for n in N_GRID] + [("modes", S, n) for S, n in sorted(MODE_SEEDS)]


@pytest.mark.parametrize("kind,S,n", SOLVER_GRID)
def test_emulated_solver_against_eigh(kind, S, n):
    """the emulation's eigenvalues, residual and orthogonality against np.linalg.eigh in units of S 2^-52: the figures behind C_EV, C_RES
    and C_ORTH, on ensemble_dist_ref.draw over the whole grid and on draw_modes wherever it has a seed (MODE_SEEDS).  No size is left
    out: the whole file takes seconds.  sweeps is in [1, 32); at S = 1 the matrix is the scalar 0, the degenerate case of the contract,
    whose sweeps is 0."""
    x, y, d2 = case(kind, S, n)
    G = centre(d2, S)["G"]
    D, V, sweeps = jacobi(G)
    if S == 1:
        assert sweeps == 0 and D[0, 0] == 0.0 and V[0, 0] == 1.0
        return
    assert 1 <= sweeps < 32, sweeps
    ev, res, orth = (e / (S * EPS) for e in solver_errors(G, D, V))
    WORST[(kind, S, n)] = (ev, res, orth, sweeps)
    print(f"{kind} S={S} n={n}: sweeps {sweeps}, eigenvalues {ev:.2f}, residual {res:.2f}, orthogonality {orth:.2f} (x S 2^-52)")
    assert ev <= C_EV and res <= C_RES and orth <= C_ORTH
    off = D - np.diag(np.diag(D))
    assert np.abs(off[np.triu_indices(S, 1)]).max() <= 2.0 ** -53 * np.trace(G)  # the stop rule: no upper entry is left above the threshold


def test_emulated_solver_on_a_decaying_spectrum():
    """64 members whose spectrum decays to 1e-17 lam_0: the iteration still ends well inside the cap, and the large eigenvalues keep
    their relative accuracy"""
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(0, 1, (64, 64)))
    lam = 10.0 ** -np.linspace(0, 17, 64)
    G = (q * lam[None]) @ q.T
    G = 0.5 * (G + G.T)
    D, V, sweeps = jacobi(G)
    print(f"decaying spectrum: {sweeps} sweeps")
    assert 1 <= sweeps < 32
    got = np.sort(np.diag(D))[::-1]
    assert np.abs(got - lam).max() <= C_EV * 64 * EPS * lam[0]


@pytest.mark.parametrize("S,n", sorted(MODE_SEEDS))
def test_draw_modes_gaps(S, n):
    """the gaps the eigenvector test of the GPU file relies on: each of the min(4, S) leading eigenvalues is at least 0.02 lam_0 away from
    every other one, for the recorded seed"""
    lam, gaps = check_gaps(draw_modes(S, n, MODE_SEEDS[(S, n)])[0])
    assert len(gaps) == min(4, S) and lam[0] > 0


def test_decompose_sort_sign_and_degenerate_cases():
    x, y, d2 = case("draw", 5, 1028)
    em = decompose(d2, 5, True)
    lam, vec = em["lam"], em["vec"]
    assert (np.diff(lam) <= 0).all() and em["info"][0] == 4 and 1 <= em["info"][1] < 32
    for k in range(5):
        big = int(np.argmax(np.abs(vec[k])))
        assert vec[k, big] > 0
    assert np.abs(vec @ vec.T - np.eye(5)).max() <= C_ORTH * 5 * EPS
    assert not em["coef"][4].any() and em["tcoord"][4] == 0.0  # the null mode (the constant vector) is dead
    np.testing.assert_allclose(em["coef"][:4], vec[:4] / np.sqrt(lam[:4, None]), rtol=4 * EPS)
    # the modes reproduce the members: x_s - c = sum_k sqrt(lam_k) vec[k][s] u_k, u_k = sum_s coef[k][s] (x_s - c)
    r = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    u = em["coef"][:4] @ r
    np.testing.assert_allclose(u @ u.T, np.eye(4), atol=1e-12)
    np.testing.assert_allclose((np.sqrt(lam[:4, None]) * vec[:4]).T @ u, r, atol=1e-12 * math.sqrt(lam[0]))
    np.testing.assert_allclose(em["tcoord"][:4], u @ (y.astype(np.float64) - x.astype(np.float64).mean(axis=0)), atol=1e-12 * math.sqrt(lam[0]))
    acc, mag, ok = project(x, em["coef"][:4])
    np.testing.assert_allclose(acc, u, atol=1e-13) and ok.all()
    # degenerate: equal members, and one member
    same = decompose(np.zeros((4, 4)), 4, False)
    assert same["info"] == (0, 0) and not same["lam"].any() and np.array_equal(same["vec"], np.eye(4)) and not same["coef"].any()
    one = decompose(np.array([[0.0, 9.0], [9.0, 0.0]]), 1, True)
    assert one["info"] == (0, 0) and one["lam"].tolist() == [0.0] and one["tnorm2"] == 9.0 and one["tcoord"].tolist() == [0.0]
    for v in (np.nan, np.inf, -1.0):
        bad = d2.copy()
        bad[1, 3] = v
        rec = decompose(bad, 5, True)
        assert rec["info"] == (-1, 0) and np.isnan(rec["lam"]).all() and not rec["vec"].any() and math.isnan(rec["tnorm2"])


# ---- 4. ensemble_mode_summary -----------------------------------------------------------------------------------------------------------
LIST_KEYS = ("EXPLAINED", "MODE_STD", "MODE_Z")
SCALAR_KEYS = ("EFF_MODES", "SPAN_SHARE", "MODE_Z_RMS")


def same(a, b, what):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for u, v in zip(a, b):
            same(u, v, what)
    else:
        assert (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-12), (what, a, b)


@pytest.mark.parametrize("has_target", [True, False])
@pytest.mark.parametrize("S", [1, 2, 5, 16])
def test_summary_against_the_definitions(S, has_target):
    recs = []
    for b in range(3):
        x, y = draw_modes(S, 260, seed=50 * S + b)
        em = emulate(x, y if has_target else None)
        recs.append((decompose(em["d2"], S, has_target), em["counts"]))
    nan = float("nan")
    # a refused image, an image with no valid pixel, and one whose mean is exact
    lam = [r["lam"] for r, _ in recs] + [np.full(S, nan), np.zeros(S), recs[0][0]["lam"]]
    tc = [r["tcoord"] for r, _ in recs] + [np.full(S, nan), np.zeros(S), np.zeros(S)]
    tn = [r["tnorm2"] for r, _ in recs] + [nan, 0.0, 0.0]
    info = [list(r["info"]) for r, _ in recs] + [[-1, 0], [0, 0], list(recs[0][0]["info"])]
    counts = [list(c) for _, c in recs] + [[260, 0], [0, 260], [260, 0]]
    got = ensemble_mode_summary(np.stack(lam), np.stack(tc), tn, info, counts, S, has_target)
    for b in range(6):
        want = summary(lam[b], tc[b], tn[b], info[b][0], counts[b][0], S, has_target)
        for q in LIST_KEYS + SCALAR_KEYS:
            same(got[q][b], want[q], (q, b))
        assert (got["rank"][b], got["sweeps"][b], got["valid"][b], got["invalid"][b]) == (info[b][0], info[b][1], counts[b][0], counts[b][1])
    assert all(math.isnan(got[q][3]) for q in SCALAR_KEYS) and all(math.isnan(got[q][4]) for q in SCALAR_KEYS)
    want = pooled(lam, tc, tn, [i[0] for i in info], [c[0] for c in counts], S, has_target)
    for q in ("EXPLAINED", "MODE_STD", "EFF_MODES", "SPAN_SHARE", "MODE_Z_RMS"):
        same(got["pooled"][q], want[q], ("pooled", q))
    assert got["pooled"]["images"] == 5 and got["pooled"]["refused"] == 1 and got["pooled"]["valid"] == want["valid"]
    # tensors and lists are taken alike
    again = ensemble_mode_summary(torch.tensor(np.stack(lam)), torch.tensor(np.stack(tc)), torch.tensor(tn, dtype=torch.float64),
                                  torch.tensor(info, dtype=torch.int32), torch.tensor(counts, dtype=torch.int32), S, has_target)
    for q in SCALAR_KEYS:
        same(again[q], got[q], q)


def test_summary_by_hand():
    # S = 3, two live modes with lam = 8 and 2 over 4 pixels: shares 0.8 / 0.2, participation 100 / 68, std sqrt(8 / 8) and sqrt(2 / 8)
    got = ensemble_mode_summary([[8.0, 2.0, 0.0]], [[2.0, -1.0, 0.0]], [10.0], [[2, 3]], [[4, 0]], 3, True)
    assert got["EXPLAINED"][0][:2] == [0.8, 0.2] and math.isnan(got["EXPLAINED"][0][2])
    assert got["EFF_MODES"] == [100.0 / 68.0] and got["MODE_STD"][0][:2] == [1.0, 0.5]
    assert got["SPAN_SHARE"] == [0.5]  # (4 + 1) / 10
    z = [2.0 / math.sqrt(8 / 2 * (4 / 3)), -1.0 / math.sqrt(2 / 2 * (4 / 3))]
    assert got["MODE_Z"][0][:2] == pytest.approx(z) and got["MODE_Z_RMS"][0] == pytest.approx(math.sqrt((z[0] ** 2 + z[1] ** 2) / 2))
    iso = ensemble_mode_summary([[1.0] * 4 + [0.0]], [[0.0] * 5], [0.0], [[4, 2]], [[16, 0]], 5, False)
    assert iso["EFF_MODES"] == [4.0]  # an isotropic ensemble: S - 1
    assert math.isnan(iso["SPAN_SHARE"][0]) and math.isnan(iso["MODE_Z_RMS"][0])
    empty = ensemble_mode_summary(np.zeros((0, 3)), np.zeros((0, 3)), [], np.zeros((0, 2)), np.zeros((0, 2)), 3, True)
    assert empty["EFF_MODES"] == [] and empty["pooled"]["images"] == 0 and math.isnan(empty["pooled"]["EFF_MODES"])
    with pytest.raises(ValueError):
        ensemble_mode_summary([[1.0, 0.0]], [[0.0, 0.0]], [0.0, 0.0], [[1, 2]], [[4, 0]], 2, True)
    with pytest.raises(ValueError):
        ensemble_mode_summary([[1.0]], [[0.0]], [0.0], [[0, 0]], [[4, 0]], 0, True)
    assert "biased" in ensemble_mode_summary.__doc__  # the small-S caveat is stated


# ---- 5. refusals that need no launch -----------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """neither entry point touches a pointer before its checks pass, so made-up (aligned, non-overlapping) addresses do"""
    lib = _lib.load()
    base = 0x7f0000000000
    buf = {k: base + i * (1 << 24) for i, k in enumerate(("d2", "lam", "vec", "coef", "tcoord", "tnorm2", "info", "x", "out"))}

    def modes(B=2, S=4, ht=1, floor=2.0 ** -30, **kw):
        a = dict(buf, **kw)
        return lib.idiff_ensemble_modes(a["d2"], B, S, ht, floor, a["lam"], a["vec"], a["coef"], a["tcoord"], a["tnorm2"], a["info"], None)

    def proj(B=2, S=4, K=2, n=64, stride=None, **kw):
        a = dict(buf, **kw)
        return lib.idiff_ensemble_project(a["x"], a["coef"], K * S if stride is None else stride, a["out"], B, S, K, n, None)

    refused = {
        "S = 0": lambda: modes(S=0), "S = 65": lambda: modes(S=65), "B = 0": lambda: modes(B=0), "B = 65536": lambda: modes(B=65536),
        "rel_floor = 0": lambda: modes(floor=0.0), "rel_floor = 1": lambda: modes(floor=1.0), "rel_floor < 0": lambda: modes(floor=-0.5),
        "rel_floor NaN": lambda: modes(floor=float("nan")), "rel_floor inf": lambda: modes(floor=float("inf")),
        "null d2": lambda: modes(d2=None), "null lam": lambda: modes(lam=None), "null vec": lambda: modes(vec=None),
        "null coef": lambda: modes(coef=None), "null tcoord": lambda: modes(tcoord=None), "null tnorm2": lambda: modes(tnorm2=None),
        "null info": lambda: modes(info=None),
        "misaligned d2": lambda: modes(d2=buf["d2"] + 4), "misaligned lam": lambda: modes(lam=buf["lam"] + 4),
        "misaligned info": lambda: modes(info=buf["info"] + 4),
        "vec == coef": lambda: modes(coef=buf["vec"]), "lam inside d2": lambda: modes(lam=buf["d2"] + 8),
        "tnorm2 == tcoord": lambda: modes(tnorm2=buf["tcoord"]), "info inside vec": lambda: modes(info=buf["vec"] + 8 * 2 * 16 - 8),
        "project: S = 0": lambda: proj(S=0), "project: S = 65": lambda: proj(S=65), "project: K = 0": lambda: proj(K=0),
        "project: K = 9": lambda: proj(K=9), "project: B = 0": lambda: proj(B=0), "project: B = 65536": lambda: proj(B=65536),
        "project: n_s % 4": lambda: proj(n=62), "project: n_s = 0": lambda: proj(n=0), "project: n_s = 2^31": lambda: proj(n=2 ** 31),
        "project: stride below K S": lambda: proj(stride=7), "project: null x": lambda: proj(x=None), "project: null coef": lambda: proj(coef=None),
        "project: null out": lambda: proj(out=None), "project: misaligned x": lambda: proj(x=buf["x"] + 8),
        "project: misaligned out": lambda: proj(out=buf["out"] + 4), "project: misaligned coef": lambda: proj(coef=buf["coef"] + 4),
        "project: out == x": lambda: proj(out=buf["x"]), "project: out inside x": lambda: proj(out=buf["x"] + 4 * 64),
        "project: out == coef": lambda: proj(out=buf["coef"]),
    }
    for what, fn in refused.items():
        n0 = ops.launch_count()
        rc = fn()
        assert rc == -1, (what, rc)  # IDIFF_E_BADARG
        assert ("ensemble_project" if what.startswith("project") else "ensemble_modes") in lib.idiff_last_error().decode(), what
        assert ops.launch_count() == n0, f"{what}: a kernel was launched before the argument check"
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_modes(torch.zeros(1, 3, 3, dtype=torch.float64), 2, True)  # host tensors: there is no CPU path
    with pytest.raises(_lib.IdiffError):
        ops.ensemble_project(torch.zeros(1, 2, 8), torch.zeros(1, 1, 2, dtype=torch.float64))


# ---- 6. the driver's option ----------------------------------------------------------------------------------------------------------------
def test_testum_modes_option_parses_and_needs_an_ensemble(tmp_path, capsys):
    parser = testUM.build_parser()
    assert not hasattr(parser.parse_args(["-opt", "x"]), "modes")  # absent without the flag
    assert parser.parse_args(["-opt", "x", "--modes"]).modes == 4 and parser.parse_args(["-opt", "x", "--modes", "2"]).modes == 2
    txt = open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--modes"])
    assert "num_samples > 1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--num-samples", "4", "--modes", "0"])
    assert "--modes takes K in [1, 64]" in capsys.readouterr().err
    assert not (tmp_path / "results").exists()  # before any image ran
