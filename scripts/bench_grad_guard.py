"""The gradient guard (grad_clip_norm / skip_nonfinite_steps) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernels: idiff_grad_sumsq, idiff_grad_guard, idiff_adam_step and idiff_adam_step_dev on each net's real flat buffers (n is
      reported: it is written nowhere else), HIP events around `--launches` back-to-back launches, the four alternated over
      `--rounds` rounds.  Bytes per second of each kernel's own traffic: 4 n for the sum of squares, 28 n for Adam (p, g, m, v read;
      p, m, v written).
  (b) iteration: model.feed_data + optimize_parameters at BASELINE config c3 (256 x 256, batch 32, fp32) on ONE model whose two
      optimizers are switched between options off / clip on / clip + skip on, round by round in one process; host clock plus a device
      synchronise around `--iters` iterations per round, `--passes` rounds of each after one untimed round.

    python scripts/bench_grad_guard.py [--size 256 --batch 32 --iters 5 --passes 5 --parts kernels,iteration --out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_grad_guard {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(v, nd=2):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def kernel_times(model, args):
    from instancediff_amd import _lib
    from instancediff_amd.ops import _p, _stream
    lib = _lib.load()
    P = int(lib.idiff_grad_sumsq_parts())
    rows = []
    for name, opt in (("drift", model.drift_optimizer), ("noise", model.noise_optimizer)):
        f, group = opt._flat[0], opt.param_groups[0]
        n = f['p'].numel()
        # copies: the timed Adam launches must not train the model under the iteration part
        p, m, v = f['p'].clone(), torch.zeros_like(f['p']), torch.zeros_like(f['p'])
        g = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(p.device) * 1e-3
        part = torch.zeros(P, device=p.device)
        info = torch.zeros(4, device=p.device)
        b1, b2 = group['betas']
        hyper = (group['lr'], b1, b2, group['eps'], group['weight_decay'], 1.0, 1)
        fns = {"grad_sumsq": lambda: lib.idiff_grad_sumsq(_p(g), n, _p(part), _stream()),
               "grad_guard": lambda: lib.idiff_grad_guard(_p(part), 1, 1.0, 1e30, 1, _p(info), _stream()),
               "adam_step": lambda: lib.idiff_adam_step(_p(p), _p(g), _p(m), _p(v), n, *hyper, _stream()),
               "adam_step_dev": lambda: lib.idiff_adam_step_dev(_p(p), _p(g), _p(m), _p(v), n, *hyper, _p(info), _stream())}
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
        row = dict(net=name, n=n, parts=P, launches=args.launches, rounds=args.rounds)
        for k, t in res.items():
            row[f"{k}_us"] = spread(t)
        row["grad_sumsq_GBps"] = round(4.0 * n / row["grad_sumsq_us"]["median"] / 1e3, 1)
        row["adam_step_GBps"] = round(28.0 * n / row["adam_step_us"]["median"] / 1e3, 1)
        row["adam_step_dev_GBps"] = round(28.0 * n / row["adam_step_dev_us"]["median"] / 1e3, 1)
        row["sumsq_over_adam"] = round(row["grad_sumsq_us"]["median"] / row["adam_step_us"]["median"], 3)
        row["guard_launches_us"] = round(row["grad_sumsq_us"]["median"] + row["grad_guard_us"]["median"]
                                         + row["adam_step_dev_us"]["median"] - row["adam_step_us"]["median"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


MODES = {"off": dict(), "clip": dict(max_grad_norm=1.0), "clip_skip": dict(max_grad_norm=1.0, skip_nonfinite=True)}


def iteration_times(model, sde, args):
    from instancediff_amd.utils.synthetic import make_batch
    batch = make_batch(args.batch, args.size, seed=1234, mixed=True)
    sde.set_seed(1234)
    res = {k: [] for k in MODES}
    coefs = {}
    for p in range(args.passes + 1):
        for tag, kw in MODES.items():
            for o in (model.drift_optimizer, model.noise_optimizer):
                o.set_grad_guard(**kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                model.feed_data(batch)
                model.optimize_parameters()
            torch.cuda.synchronize()
            if p:  # round 0 warms every mode up (weight packs, workspaces, the guard's buffers)
                res[tag].append((time.perf_counter() - t0) * 1e3 / args.iters)
            if tag != "off":
                coefs[tag] = {k: round(model.grad_info[k]["coef"], 4) for k in ("drift", "noise")}
    row = dict(size=args.size, batch=args.batch, iters_per_round=args.iters, passes=args.passes, last_coefs=coefs,
               skipped_steps=model.grad_info["skipped_steps"])
    for tag in MODES:
        row[f"{tag}_ms"] = spread(res[tag])
    off = row["off_ms"]
    row["off_spread_ms"] = round(off["max"] - off["min"], 2)
    for tag in ("clip", "clip_skip"):
        d = row[f"{tag}_ms"]["median"] - off["median"]
        row[f"{tag}_minus_off_ms"] = round(d, 2)
        row[f"{tag}_inside_off_spread"] = bool(abs(d) <= row["off_spread_ms"])
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernels,iteration")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grad_guard needs a GPU"
    from instancediff_amd import pipeline
    dev = torch.device("cuda", 0)
    model, sde = pipeline.build(phase="train", device=dev, T=args.T, seed=0)
    model.set_train()
    res = dict(metric="gradient guard: kernel us on the nets' flat buffers; ms per training iteration, options off / clip / clip + skip",
               device=torch.cuda.get_device_name(0))
    parts = args.parts.split(",")
    if "kernels" in parts:
        res["kernels"] = kernel_times(model, args)
        if args.out:
            write(args.out, res)
    if "iteration" in parts:
        res["iteration"] = iteration_times(model, sde, args)
    print(json.dumps(res), flush=True)
    if args.out:
        write(args.out, res)


def write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
