"""The 16-byte gather of conv_wino4_kernel (csrc/conv_wino4.hip, G16) on the smallest shapes that reach each of its paths
(wino_gather16_rows.ROWS).  Every row runs the 16x32 F(4x4,3x3) kernel asked for by name, exactly as test_wino_fwd_gpu.py runs its
rows -- same operands inside sentinel buffers, same fp64 reference (conv_branch_ref.py), same metric and the same tolerances (4e-5 of
the output range, statistics 4e-5 / 1e-4, or the fp32 floor for rows with a prologue) -- and

  * six of them must reproduce, bit for bit, the outputs and GroupNorm partials that the parent commit's build (dword gather
    throughout) gave for the same inputs: tests/golden/wino_gather16/*.npz, written by scripts/record_wino_gather16_golden.py.  The
    change moves data only; every multiply and add is where it was;
  * the row whose source starts four bytes past a 16-byte boundary (dword gather) gives the bits of the same call on an aligned
    copy of the source (16-byte gather)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conv_branch_ref import make_inputs  # noqa: E402
from test_wino_fwd_gpu import _compare, _operands, _run_twice  # noqa: E402
from wino_fwd_rows import WINO4, eligible, expected_instantiation, geometry  # noqa: E402
from wino_gather16_rows import GOLDEN, ITEMS_BIG, ROWS, SEED0  # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_gather16")


def input_digest(inp):
    """float64 sums of a row's inputs (recorded beside the golden outputs: a changed random stream is told from a changed kernel)"""
    flat = []
    for k in sorted(inp):
        v = inp[k]
        for t in (v if isinstance(v, tuple) else (v,)):
            if t is not None:
                flat.append(float(t.double().sum()))
    return np.array(flat, dtype=np.float64)


def run_row(row, odd=None):
    """(inp, t, guards) of a launched row; `odd`: override of the row's list of operands one float past a 16-byte boundary"""
    assert row["claim"] == expected_instantiation(row) and eligible(row, WINO4)
    inp = make_inputs(row, SEED0 + [r["name"] for r in ROWS].index(row["name"]))
    if odd is not None:
        row = dict(row, odd=odd)
    t, guards = _operands(row, inp)
    _run_twice(row, WINO4, t)
    return inp, t, guards


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_gather16_row(row):
    inp, t, guards = run_row(row)
    if row["name"].endswith("384-items"):
        assert geometry(row, WINO4, 256)["total"] == ITEMS_BIG == 384
    _compare(row, WINO4, inp, t, guards)
    if row["name"] in GOLDEN:
        g = np.load(os.path.join(GOLDEN_DIR, row["name"] + ".npz"))
        assert np.array_equal(g["inputs"], input_digest(inp)), f"{row['name']}: the inputs are not the recorded ones"
        assert torch.equal(t["out"].cpu(), torch.from_numpy(g["out"])), f"{row['name']}: output bits differ from the parent's"
        assert torch.equal(t["stats"].cpu(), torch.from_numpy(g["stats"])), f"{row['name']}: GroupNorm partials differ from the parent's"
    if row["odd"]:
        assert t["x0"].data_ptr() % 16 == 4
        _, ta, _ = run_row(row, odd=())
        assert ta["x0"].data_ptr() % 16 == 0
        assert torch.equal(t["out"], ta["out"]) and torch.equal(t["stats"], ta["stats"]), f"{row['name']}: dword and 16-byte gather differ"
