"""CPU mirror of the cross-attention key-split rows of test_step_kernels_gpu.py: idiff_smm_xattn_ws_floats is host-only, so the split
counts the GPU rows rely on are asserted without a GPU too -- a change of smm_split trips here first."""
import pytest

from instancediff_amd import _lib

from step_split_rows import SPLIT_ROWS, split_rule, witnessed_nsplit


@pytest.mark.parametrize("row,Cm,qh,B,N,ns,kps,boost", [pytest.param(*r, id=r[0]) for r in SPLIT_ROWS])
def test_split_rows(row, Cm, qh, B, N, ns, kps, boost):
    lib = _lib.load()
    assert split_rule(N) == (ns, kps), row
    assert witnessed_nsplit(lib, B, qh[0], qh[1], Cm, N) == ns, row
    nkb = -(-N // 32)
    assert (ns - 1) * kps < nkb <= ns * kps  # every split has a key block; the last may be short


def test_split_table_hits_every_clamp():
    got = {r[0]: (r[4], r[5], r[6]) for r in SPLIT_ROWS}
    nkbs = {-(-n // 32): (ns, k) for n, ns, k in got.values()}
    assert any(nkb == 1 and k == 1 for nkb, (ns, k) in nkbs.items())                     # k > nkb -> nkb
    assert any(nkb // 32 < 2 and k == 2 for nkb, (ns, k) in nkbs.items())                # k < 2 -> 2
    assert any(nkb // 32 > 64 and k == 64 and nkb % 64 for nkb, (ns, k) in nkbs.items())  # k > 64 -> 64, short last split
    assert {3, 4} <= {k for r in SPLIT_ROWS if r[1] == 72 for k in [r[6]]}               # both sides of the w-form switch
    assert any(n % 32 for n, _, _ in got.values())


def test_split_does_not_depend_on_the_batch():
    lib = _lib.load()
    for N in (4, 36, 4096, 131232):
        assert len({witnessed_nsplit(lib, B, 5, 4, 72, N) for B in (1, 2, 16)}) == 1
