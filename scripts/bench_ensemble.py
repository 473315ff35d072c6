"""Posterior ensembles (driftSDE num_samples) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) calls: per-image wall time of an S-member `reverse_ddpm_ensemble` at HxH, `sample_T: K`, against S sequential `reverse_ddpm`
      calls at batch 1 in the same process (the only way to S samples without the feature): host clock around the call(s) plus a
      synchronise, the two forms alternated over `--calls` repetitions after one untimed, median and spread of the repetitions.
  (b) step kernels: per-launch time of `ops.drift_reverse_step_members_dev` against `ops.drift_reverse_step_dev` (3-row table) and
      `ops.drift_reverse_step2_dev` (5-row table, both rho non-zero), on-device noise: HIP events around `--launches` back-to-back
      launches, the kernels alternated over `--rounds` rounds, median of the rounds (the method of scripts/bench_solver_order.py).
  (c) `ops.ensemble_stats` at 256x256, S = 16 (and the second-read form at S = 17): the same event method, (S + 2)*4 bytes per pixel.

    python scripts/bench_ensemble.py [--T 100 --K 10 --H 224 --S 1,4,8,16 --calls 3 --launches 200 --rounds 5 --parts calls,kernel,stats --out FILE]
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
    print(f"[bench_ensemble {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per launch of each round]}: the kernels alternated round by round, `launches` back-to-back launches per timing"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(20):
            fn()
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return res


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K))
    model.set_eval()
    batch = make_batch(1, args.H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    rows = []
    for S in args.S:
        times = {"ensemble": [], "loop": []}
        for i in range(args.calls + 1):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sde.reverse_ddpm_ensemble(cond, batch['names'], model.text_encoder, image_context=ctx, num_samples=S)
            torch.cuda.synchronize()
            times["ensemble"].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K and sde.last_mode == "graph", (sde.last_steps, sde.last_mode)
            t0 = time.perf_counter()
            for _ in range(S):
                sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx)
            torch.cuda.synchronize()
            times["loop"].append((time.perf_counter() - t0) * 1e3)
        row = dict(H=args.H, T=args.T, K=args.K, S=S, max_batch=sde.max_batch, loop_mode=sde.last_mode)
        for k, v in times.items():
            v = v[1:]  # the first repetition fills the weight / text caches
            row[f"{k}_ms_median"] = round(statistics.median(v), 2)
            row[f"{k}_ms"] = [round(t, 2) for t in v]
        row["loop_over_ensemble"] = round(row["loop_ms_median"] / row["ensemble_ms_median"], 2)
        row["ensemble_ms_per_sample"] = round(row["ensemble_ms_median"] / S, 2)
        log(json.dumps(row))
        rows.append(row)
    del model, sde
    torch.cuda.empty_cache()
    return rows


def kernel_times(H, R, args, dev):
    from instancediff_amd import ops
    shp = (R, 1, H, H)
    n = R * H * H
    g = torch.Generator().manual_seed(0)
    x0, r, e, rp, ep, cond = (torch.randn(shp, generator=g).to(dev) for _ in range(6))
    xa = torch.empty(shp, device=dev)
    Tp1, t = 8, 5
    tb = torch.zeros(5, Tp1)
    tb[:, t] = torch.tensor([1e-3, 1e-3, 1e-3, 0.5, 0.5])  # small a, b, c: x stays finite over thousands of in-place launches
    coef5, coef3 = tb.to(dev).contiguous(), tb[:3].to(dev).contiguous()
    state = torch.tensor([t, 0, 0], dtype=torch.int32, device=dev)
    members = ops.member_ids(range(1, R + 1), dev)
    x = x0.clone()
    fns = {
        "step_dev": lambda: ops.drift_reverse_step_dev(x, r, e, None, cond, xa, coef3, state, 1, n // 4, 0),
        "members_3": lambda: ops.drift_reverse_step_members_dev(x, r, e, None, None, None, cond, xa, coef3, state, members, 1),
        "step2_dev": lambda: ops.drift_reverse_step2_dev(x, r, e, rp, ep, None, cond, xa, coef5, state, 1, n // 4, 0),
        "members_5": lambda: ops.drift_reverse_step_members_dev(x, r, e, rp, ep, None, cond, xa, coef5, state, members, 1),
    }
    res = event_time(fns, args.launches, args.rounds)
    assert torch.isfinite(x).all()
    row = dict(H=H, rows=R, launches=args.launches, rounds=args.rounds, noise="on-device Philox")
    for k, v in res.items():
        row[f"{k}_us"] = round(statistics.median(v), 2)
        row[f"{k}_us_rounds"] = [round(t, 2) for t in v]
    log(json.dumps(row))
    return row


def stats_times(args, dev):
    from instancediff_amd import ops
    rows = []
    for B, S, H in ((1, 16, 256), (16, 16, 256), (1, 17, 256), (16, 17, 256)):
        x = (0.5 * torch.randn(B, S, 1, H, H)).to(dev)
        res = event_time({"stats": lambda: ops.ensemble_stats(x)}, args.launches, args.rounds)["stats"]
        us = statistics.median(res)
        nbytes = (S + 2) * 4 * B * H * H
        row = dict(B=B, S=S, H=H, form="registers" if S <= 16 else "second read", us=round(us, 2), us_rounds=[round(t, 2) for t in res],
                   bytes=nbytes, GBps=round(nbytes / us * 1e-3, 1), note="time includes two output allocations per launch")
        log(json.dumps(row))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10, help="jumps per chain of the call-time part")
    ap.add_argument("--H", type=int, default=224)
    ap.add_argument("--S", type=str, default="1,4,8,16")
    ap.add_argument("--calls", type=int, default=3, help="timed repetitions per S (after one untimed)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="calls,kernel,stats")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    args.S = [int(v) for v in args.S.split(",")]
    assert torch.cuda.is_available(), "bench_ensemble needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE posterior ensembles: S-member batched chain vs S sequential calls, member step kernel, ensemble_stats",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["step_kernel"] = [kernel_times(224, 1, args, dev), kernel_times(256, 16, args, dev)]
    if "stats" in parts:
        res["ensemble_stats"] = stats_times(args, dev)
    if "calls" in parts:
        res["calls"] = call_times(args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
