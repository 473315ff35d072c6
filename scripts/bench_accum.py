"""Gradient accumulation (accum_steps) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernels: idiff_gather_segments_acc against idiff_gather_segments on each net's real flat gradient buffer (n is reported) with the
      segment table FusedAdam._collect builds for it -- one record per parameter, the sources laid out as separate tensors; HIP events
      around `--launches` back-to-back launches, the two alternated over `--rounds` rounds.  Bytes per second of each kernel's own
      traffic: 12 n for the accumulating form (dst and src read, dst written), 8 n for the assigning one.
  (b) iteration: model.feed_data + optimize_parameters at BASELINE config c3 (256 x 256, fp32) at the SAME effective batch on ONE
      model switched round by round between accum_steps 1 x batch 32, 2 x 16 and 4 x 8; HIP events on the step's stream around
      `--steps` optimizer steps per round (host work included: the closing event follows the last step's host copy), `--passes`
      rounds of each after one untimed round.  ms per OPTIMIZER step.
  (c) launches: library launches (idiff_launch_count) per micro-step with the option off, counted as bench.py --mode train counts its
      library_launches_per_it (same model, batch and seeds): to be set against the parent commit's figure.

    python scripts/bench_accum.py [--size 256 --batch 32 --steps 3 --passes 5 --parts kernels,iteration,launches --out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_accum {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(v, nd=2):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def kernel_times(model, args):
    from instancediff_amd import _lib
    from instancediff_amd.ops import _p, _stream
    lib = _lib.load()
    rows = []
    for name, opt in (("drift", model.drift_optimizer), ("noise", model.noise_optimizer)):
        f = opt._flat[0]
        n = f['g'].numel()
        dev = f['g'].device
        dst = torch.zeros(n, device=dev)  # a buffer of the flat gradient's size and alignment: the timed launches leave the model alone
        src = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev) * 1e-3
        sizes = np.asarray([p.numel() for p in f['params']], dtype=np.int64)
        offs = np.cumsum(sizes) - sizes
        tab = np.zeros((len(sizes), 4), dtype=np.int64)
        tab[:, 0] = src.data_ptr() + 4 * offs
        tab[:, 1], tab[:, 2] = offs, sizes
        nb = (sizes + 4095) // 4096
        tab[:, 3] = np.cumsum(nb) - nb
        assert int(offs[-1] + sizes[-1]) == n
        dev_tab = torch.from_numpy(tab).to(dev)
        nseg, nblocks = len(sizes), int(nb.sum())
        fns = {"gather_segments": lambda: lib.idiff_gather_segments(dev_tab.data_ptr(), nseg, nblocks, _p(dst), _stream()),
               "gather_segments_acc": lambda: lib.idiff_gather_segments_acc(dev_tab.data_ptr(), nseg, nblocks, _p(dst), _stream())}
        res = {k: [] for k in fns}
        for fn in fns.values():
            for _ in range(10):
                assert fn() == 0
        for _ in range(args.rounds):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        row = dict(net=name, n=n, segments=nseg, workgroups=nblocks, launches=args.launches, rounds=args.rounds)
        for k, t in res.items():
            row[f"{k}_us"] = spread(t)
        row["gather_segments_TBps"] = round(8.0 * n / row["gather_segments_us"]["median"] / 1e6, 2)
        row["gather_segments_acc_TBps"] = round(12.0 * n / row["gather_segments_acc_us"]["median"] / 1e6, 2)
        row["acc_minus_assign_us"] = round(row["gather_segments_acc_us"]["median"] - row["gather_segments_us"]["median"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


def iteration_times(model, sde, args):
    from instancediff_amd.utils.synthetic import make_batch
    modes = [(k, args.batch // k) for k in (1, 2, 4)]
    batches = {k: make_batch(mb, args.size, seed=1234, mixed=True) for k, mb in modes}
    sde.set_seed(1234)
    res = {k: [] for k, _ in modes}
    for p in range(args.passes + 1):
        for k, mb in modes:
            model.set_accum_steps(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                for _ in range(k):
                    model.feed_data(batches[k])
                    model.optimize_parameters()
                assert model.stepped
            e1.record()
            torch.cuda.synchronize()
            if p:  # round 0 warms every mode up (weight packs, workspaces at each micro-batch size)
                res[k].append(e0.elapsed_time(e1) / args.steps)
    model.set_accum_steps(1)
    row = dict(size=args.size, effective_batch=args.batch, optimizer_steps_per_round=args.steps, passes=args.passes)
    for k, mb in modes:
        row[f"k{k}_x_{mb}_ms"] = spread(res[k])
    off = row[f"k1_x_{args.batch}_ms"]
    row["k1_spread_ms"] = round(off["max"] - off["min"], 2)
    for k, mb in modes[1:]:
        row[f"k{k}_minus_k1_ms"] = round(row[f"k{k}_x_{mb}_ms"]["median"] - off["median"], 2)
    log(json.dumps(row))
    return row


def launch_count(model, sde, args):
    """bench.py's train_measure, as far as the count goes: warm-up, then launches over `--count-iters` iterations"""
    from instancediff_amd import ops
    from instancediff_amd.utils.synthetic import make_batch
    assert model.accum_steps == 1
    batch = make_batch(args.batch, args.size, seed=1234, mixed=True)
    sde.set_seed(1234)
    torch.manual_seed(99)
    for _ in range(3):
        model.feed_data(batch)
        model.optimize_parameters()
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for _ in range(args.count_iters):
        model.feed_data(batch)
        model.optimize_parameters()
    torch.cuda.synchronize()
    row = dict(size=args.size, batch=args.batch, iters=args.count_iters, accum_steps=1,
               library_launches_per_micro_step=round((ops.launch_count() - n0) / args.count_iters, 1))
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32, help="the effective batch: accum_steps x micro-batch")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3, help="optimizer steps per timed round")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--count-iters", type=int, default=20)
    ap.add_argument("--parts", type=str, default="kernels,launches,iteration")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert args.batch % 4 == 0, "the effective batch is split into 2 and 4 micro-batches"
    assert torch.cuda.is_available(), "bench_accum needs a GPU"
    from instancediff_amd import pipeline
    dev = torch.device("cuda", 0)
    model, sde = pipeline.build(phase="train", device=dev, T=args.T, seed=0)
    model.set_train()
    res = dict(metric="gradient accumulation: gather kernels (us, TB/s) on the nets' flat buffers; library launches per micro-step, option "
                      "off; ms per optimizer step at one effective batch, accum_steps 1 / 2 / 4",
               device=torch.cuda.get_device_name(0))
    parts = args.parts.split(",")
    for part, fn in (("kernels", lambda: kernel_times(model, args)), ("launches", lambda: launch_count(model, sde, args)),
                     ("iteration", lambda: iteration_times(model, sde, args))):
        if part in parts:
            res[part] = fn()
            if args.out:
                write(args.out, res)
    print(json.dumps(res), flush=True)


def write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
