"""Geometric self-ensembles (driftSDE self_ensemble) on the clock.  Prints one JSON line.

  (a) kernel: `ops.dihedral_rows` in us per launch and TB/s of its own bytes (what it reads plus what it writes), at 256x256 with 16
      rows and 224x224 with 8 rows, separately for a code without the transposition (6, the half turn), codes with it (1, and 7 with both
      flips on top) and the expanding form of the chain's first launch (in_rep = S = 8 under the eight dihedral codes, which reads one
      row per eight it writes).  The yardstick is `ops.axpby(x, x, 1.0, 0.0)` over the same tensor in the same run: the project's plain
      copy.  HIP events around `--launches` back-to-back repetitions, the forms alternated over `--rounds` rounds.  Tensors of this size
      stay in the last-level cache between repetitions, for the yardstick as for the kernel: the rates compare the two, they are not
      HBM rates.
  (b) chain: one testUM-shaped call, `model.test()` at 224x224, `num_samples: 8`, `sample_T: 10`, with the option off and with
      `self_ensemble: dihedral`, alternated pass by pass in one process over the same nets.  Host clock around each call plus a device
      synchronise; one untimed pass of each first.  The difference of the medians is set against the off column's own spread.
  (c) bench: `bench.py`'s default line from two checkouts, `--parent-root` (the commit before) against this one, alternated, each run a
      fresh process.  The change touches nothing on that path; this is the record of it.

    python scripts/bench_self_ensemble.py [--parts kernel,chain,bench --parent-root DIR --out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_self_ensemble {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(v, nd=2):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def kernel_times(H, R, S, args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import self_ensemble_codes
    g = torch.Generator().manual_seed(0)
    x = torch.randn((R, 1, H, H), generator=g).to(dev)
    few = x[:R // S].contiguous()
    out = torch.empty_like(x)
    codes = self_ensemble_codes("dihedral")
    nbytes = x.numel() * 4
    fns = {
        "copy_axpby": (lambda: ops.axpby(x, x, 1.0, 0.0, out=out), 2 * nbytes),
        "code_6_half_turn": (lambda: ops.dihedral_rows(x, [6], out=out), 2 * nbytes),
        "code_1_transpose": (lambda: ops.dihedral_rows(x, [1], out=out), 2 * nbytes),
        "code_7_transpose_and_flips": (lambda: ops.dihedral_rows(x, [7], out=out), 2 * nbytes),
        "dihedral_in_rep_S": (lambda: ops.dihedral_rows(few, codes, S=S, in_rep=S, out=out), nbytes + nbytes // S),
    }
    # the permutation is checked here too, before it is timed
    got = ops.dihedral_rows(few, codes, S=S, in_rep=S)
    for r in range(R):
        w, k = few[r // S], codes[r % S]
        w = w.transpose(-1, -2) if k & 1 else w
        w = w.flip(-2) if k & 2 else w
        w = w.flip(-1) if k & 4 else w
        assert torch.equal(got[r], w), r
    res = {k: [] for k in fns}
    for fn, _ in fns.values():
        for _ in range(20):
            fn()
    for _ in range(args.rounds):
        for k, (fn, _) in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    row = dict(H=H, rows=R, S=S, launches=args.launches, rounds=args.rounds, tensor_MiB=round(nbytes / 2 ** 20, 2))
    for k, v in res.items():
        us = spread(v)
        row[k] = dict(us=us, bytes=fns[k][1], TB_per_s=round(fns[k][1] / (us["median"] * 1e-6) / 1e12, 3))
    copy = row["copy_axpby"]["TB_per_s"]
    for k in fns:
        row[k]["rate_over_copy"] = round(row[k]["TB_per_s"] / copy, 3)
    log(json.dumps(row))
    return row


def chain_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    from instancediff_amd.utils.synthetic import make_batch
    H, S = 224, 8
    model, base = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K))
    model.set_eval()
    sdes = {}
    for tag, kind in (("off", None), ("dihedral", "dihedral")):
        s = driftSDE(nets=model.get_nets(), T=args.T, max_sigma=base.max_sigma, eta=base.eta, drift_schedule=base.schedule_names[0],
                     noise_schedule=base.schedule_names[1], sample_T=args.K, num_samples=S, max_batch=16, self_ensemble=kind)
        s.set_gpu(dev)
        sdes[tag] = s
    images = [make_batch(1, H, seed=100 + i) for i in range(args.images)]
    per_pass = {tag: [] for tag in sdes}
    std_mean = {}
    for p in range(args.passes + 1):
        for tag, sde in sdes.items():
            model.set_sde(sde)
            sde.set_seed(7)
            ts = []
            for batch in images:
                model.feed_data(batch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.test()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert sde.last_mode == "graph" and sde.last_steps == args.K
                assert (sde.last_member_ops is None) == (tag == "off")
            std_mean[tag] = round(float(model.output_std.mean()), 6)
            if p:  # pass 0 fills the weight and text caches
                per_pass[tag].append(statistics.median(ts))
    row = dict(workload="224 num_samples 8", H=H, num_samples=S, T=args.T, K=args.K, images=args.images, passes=args.passes)
    for tag in sdes:
        row[f"{tag}_ms"] = spread(per_pass[tag])
        row[f"{tag}_mean_std_of_last_image"] = std_mean[tag]
    d = row["dihedral_ms"]["median"] - row["off_ms"]["median"]
    off_spread = row["off_ms"]["max"] - row["off_ms"]["min"]
    row["added_ms_per_image"] = round(d, 2)
    row["off_spread_ms"] = round(off_spread, 2)
    row["inside_off_spread"] = bool(abs(d) <= off_spread)
    log(json.dumps(row))
    return row


def bench_lines(args):
    """bench.py's default line from the two checkouts, alternated; every run a fresh process"""
    roots = {"parent": os.path.abspath(args.parent_root), "this": ROOT}
    vals = {k: [] for k in roots}
    metric = None
    for r in range(args.bench_rounds):
        for tag, root in roots.items():
            p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "3"],
                               cwd=root, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"bench.py of {tag} failed ({p.returncode}): {p.stderr[-2000:]}")
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            metric = line["metric"]
            vals[tag].append(float(line["value"]))
            log(f"round {r} {tag}: {line['value']} {metric}")
    row = dict(metric=metric, steps=args.bench_steps, rounds=args.bench_rounds)
    for tag in roots:
        row[tag] = dict(spread(vals[tag], 3), runs=[round(v, 3) for v in vals[tag]])
    row["this_over_parent"] = round(row["this"]["median"] / row["parent"]["median"], 4)
    row["parent_spread"] = round(row["parent"]["max"] - row["parent"]["min"], 3)
    log(json.dumps(row))
    return row


def write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--parent-root", type=str, default=None, help="a built checkout of the commit before (part `bench`)")
    ap.add_argument("--parts", type=str, default="kernel,chain")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    parts = args.parts.split(",")
    if "bench" in parts and not args.parent_root:
        ap.error("part `bench` needs --parent-root")
    res = dict(metric="driftSDE self_ensemble: dihedral_rows us and TB/s against the axpby copy; ms per model.test() image, option off vs dihedral; "
                      "bench.py parent vs this")
    if "bench" in parts:  # first: the children run before this process holds anything on the device
        res["bench"] = bench_lines(args)
        if args.out:
            write(args.out, res)
    assert torch.cuda.is_available(), "bench_self_ensemble needs a GPU"
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)
    if "kernel" in parts:
        res["kernel"] = [kernel_times(256, 16, 8, args, dev), kernel_times(224, 8, 8, args, dev)]
        if args.out:
            write(args.out, res)
    if "chain" in parts:
        res["chain"] = chain_times(args, dev)
    print(json.dumps(res), flush=True)
    if args.out:
        write(args.out, res)


if __name__ == "__main__":
    main()
