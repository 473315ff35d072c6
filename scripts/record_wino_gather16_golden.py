#!/usr/bin/env python3
"""Records the outputs and GroupNorm partials of the golden rows of tests/wino_gather16_rows.py as tests/test_wino_gather16_gpu.py
compares them: run on a build of the commit BEFORE the 16-byte gather (IDIFF_LIB=/path/to/that/libidiff_hip.so), the files are what
the dword gather gives.  usage: record_wino_gather16_golden.py [--out DIR]   (default tests/golden/wino_gather16)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_wino_gather16_gpu import input_digest, run_row  # noqa: E402
from wino_gather16_rows import GOLDEN, ROWS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wino_gather16"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    from instancediff_amd import _lib
    print("library:", _lib.LIB_PATH)
    for row in ROWS:
        if row["name"] not in GOLDEN:
            continue
        inp, t, _ = run_row(row)
        path = os.path.join(args.out, row["name"] + ".npz")
        np.savez(path, inputs=input_digest(inp), out=t["out"].cpu().numpy(), stats=t["stats"].cpu().numpy())
        print(f"{row['name']}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
