"""Geometric self-ensembles (driftSDE self_ensemble) on the host: the C ABI's new symbol, the code list and its inverses against numpy's
rot90 / fliplr, the numpy mirror of the kernel's index rule against the torch expression of the contract, the option's parsing, the
call-time refusals and the driver's."""
import ctypes

import numpy as np
import pytest
import torch
from dihedral_ref import dihedral_ref, dihedral_rows_ref, dihedral_torch

from instancediff_amd import _lib, ops, pipeline, testUM
from instancediff_amd.models.SDEs import create_sde
from instancediff_amd.models.SDEs import driftSDE as D


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "idiff_dihedral_rows" in header
    assert "idiff_dihedral_rows" in _lib.SIGNATURES
    assert hasattr(lib, "idiff_dihedral_rows")
    assert sorted(_lib.SIGNATURES) == header
    res, args = _lib.SIGNATURES["idiff_dihedral_rows"]
    assert res is ctypes.c_int and len(args) == 11 and args[9] is ctypes.c_uint32


# ---- 2. the codes -----------------------------------------------------------------------------------------------------------------
def test_the_eight_codes_are_the_eight_symmetries_of_the_square():
    a = np.arange(16, dtype=np.float32).reshape(4, 4)
    want = [np.rot90(a, k) for k in range(4)] + [np.rot90(np.fliplr(a), k) for k in range(4)]
    codes = D.self_ensemble_codes("dihedral")
    assert sorted(codes) == list(range(8))
    got = [dihedral_ref(a, k) for k in range(8)]
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(got[i], got[j]), (i, j)
    for g in got:
        assert sum(np.array_equal(g, w) for w in want) == 1
    for w in want:
        assert sum(np.array_equal(g, w) for g in got) == 1
    assert np.array_equal(got[0], a) and np.array_equal(got[4], np.fliplr(a)) and np.array_equal(got[2], np.flipud(a))
    assert np.array_equal(got[6], np.rot90(a, 2)) and np.array_equal(got[1], a.T)


def test_inverse_code_undoes_every_code():
    a = np.arange(64, dtype=np.float32).reshape(8, 8)
    for k in range(8):
        inv = D.inverse_code(k)
        assert np.array_equal(dihedral_ref(dihedral_ref(a, k), inv), a), k
        assert inv == (k if not k & 1 else 1 | ((k & 2) << 1) | ((k & 4) >> 1))
        assert D.inverse_code(inv) == k
    assert [D.inverse_code(k) for k in range(8)] == [0, 1, 2, 5, 4, 3, 6, 7]
    for bad in (-1, 8, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            D.inverse_code(bad)


def test_code_lists():
    dih, fl = D.self_ensemble_codes("dihedral"), D.self_ensemble_codes("flips")
    assert dih == [0, 4, 2, 6, 1, 5, 3, 7] and fl == [0, 4, 2, 6]
    assert dih[0] == 0 and fl[0] == 0
    assert all(not k & 1 for k in dih[:4]) and all(k & 1 for k in dih[4:])
    assert dih[:len(fl)] == fl and sorted(dih) == list(range(8))
    for s in range(24):  # the same code under both kinds while s % 8 < 4
        if s % 8 < 4:
            assert dih[s % 8] == fl[s % 4]
    dih.append(9)  # a copy: the caller cannot edit the rule
    assert D.self_ensemble_codes("dihedral") == [0, 4, 2, 6, 1, 5, 3, 7]
    for bad in (None, True, 8, "x8", "Dihedral"):
        with pytest.raises(ValueError):
            D.self_ensemble_codes(bad)


# ---- 3. the mirror against the torch expression -------------------------------------------------------------------------------------
def test_mirror_agrees_with_torch():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 8, 12)).astype(np.float32)
    flips = D.self_ensemble_codes("flips")
    assert sorted(flips) == [0, 2, 4, 6]
    for k in flips:
        assert np.array_equal(dihedral_ref(a, k), dihedral_torch(torch.from_numpy(a), k).numpy()), k
    for k in (1, 3, 5, 7):
        with pytest.raises(ValueError):
            dihedral_ref(a, k)
    sq = rng.standard_normal((3, 12, 12)).astype(np.float32)
    for k in range(8):
        assert np.array_equal(dihedral_ref(sq, k), dihedral_torch(torch.from_numpy(sq), k).numpy()), k
    rows = dihedral_rows_ref(sq[:2, None], [0, 4, 1], S=3, in_rep=3)  # [2, 1, 12, 12] -> 6 rows
    assert rows.shape == (6, 1, 12, 12)
    for r in range(6):
        assert np.array_equal(rows[r, 0], dihedral_ref(sq[r // 3], [0, 4, 1][r % 3]))


# ---- 4. the option ------------------------------------------------------------------------------------------------------------------
def test_option_parsing():
    assert D._self_ensemble(None) is None
    assert D._self_ensemble("flips") == "flips" and D._self_ensemble("dihedral") == "dihedral"
    sde = D.driftSDE(T=10)
    assert sde.self_ensemble is None and sde.last_member_ops is None
    for kind in ("flips", "dihedral"):
        assert D.driftSDE(T=10, self_ensemble=kind).self_ensemble == kind
        sde.set_self_ensemble(kind)
        assert sde.self_ensemble == kind
    sde.set_self_ensemble("flips")
    for bad in (True, False, 8, "x8", "Dihedral"):
        with pytest.raises(ValueError):
            D._self_ensemble(bad)
        with pytest.raises(ValueError):
            D.driftSDE(T=10, self_ensemble=bad)
        with pytest.raises(ValueError):
            sde.set_self_ensemble(bad)
        assert sde.self_ensemble == "flips"  # a refused value leaves the sde as it was
    sde.set_self_ensemble(None)
    assert sde.self_ensemble is None
    sde.set_self_ensemble("dihedral")
    sde.set_self_ensemble()
    assert sde.self_ensemble is None


def test_option_reaches_the_sde_through_create_sde():
    base = dict(class_name="driftSDE", T=10, max_sigma=0.4, drift_schedule="sigmoid", noise_schedule="sigmoid")
    assert create_sde({}, base).self_ensemble is None
    assert create_sde({}, dict(base, self_ensemble="dihedral", num_samples=8)).self_ensemble == "dihedral"
    assert create_sde({}, dict(base, self_ensemble="flips")).self_ensemble == "flips"
    with pytest.raises(ValueError):
        create_sde({}, dict(base, self_ensemble="x8"))


# ---- 5. refusals at call time, before any launch -----------------------------------------------------------------------------------------
def test_call_time_refusals_launch_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a launch was reached")

    for name in ("dihedral_rows", "ensemble_init", "chain_begin", "member_ids", "ensemble_stats"):
        monkeypatch.setattr(ops, name, boom)
    sde = D.driftSDE(T=20, sample_T=4, num_samples=4, self_ensemble="dihedral")
    with pytest.raises(ValueError, match="square"):
        sde.reverse_ddpm_ensemble(torch.zeros(1, 1, 32, 48), ["a"], None)
    with pytest.raises(ValueError, match="multiple of 4"):
        sde.reverse_ddpm_ensemble(torch.zeros(1, 1, 6, 6), ["a"], None)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        sde.reverse_ddpm_ensemble(torch.zeros(1, 32, 32), ["a"], None)
    sde.set_self_ensemble("flips")
    with pytest.raises(ValueError, match="multiple of 4"):
        sde.reverse_ddpm_ensemble(torch.zeros(1, 1, 8, 6), ["a"], None)
    assert sde._member_base == 1 and sde.last_member_ops is None  # no member id was handed out either


def test_ops_wrapper_states_the_shape_checks():
    x = torch.zeros(2, 1, 8, 12)
    for codes in ([], list(range(8)) + [0], [8], [-1], [True], [1.0], ["0"]):
        with pytest.raises(ValueError, match="codes"):
            ops.dihedral_rows(x, codes)
    with pytest.raises(ValueError, match="square"):
        ops.dihedral_rows(x, [0, 1])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dihedral_rows(torch.zeros(2, 1, 6, 6), [0])
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        ops.dihedral_rows(torch.zeros(2, 8, 12), [0])
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="in_rep"):
            ops.dihedral_rows(x, [0], in_rep=bad)
        with pytest.raises(ValueError, match="S must"):
            ops.dihedral_rows(x, [0], S=bad)
    with pytest.raises(_lib.IdiffError):  # a host tensor: the hot path has no CPU fallback
        ops.dihedral_rows(x, [0, 4])


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------
def test_testum_self_ensemble_needs_an_ensemble(tmp_path, capsys):
    txt = open(pipeline.DEFAULT_YAML).read().replace("result_root: results", f"result_root: {tmp_path}/results")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    for extra in ([], ["--num-samples", "1"]):
        with pytest.raises(SystemExit):
            testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--self-ensemble", "dihedral"] + extra)
        assert "num_samples > 1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        testUM.main(["-opt", str(cfg), "--random-init", "--limit", "1", "--num-samples", "2", "--self-ensemble", "x8"])
    assert "invalid choice" in capsys.readouterr().err
    assert not (tmp_path / "results").exists()  # before any image ran
