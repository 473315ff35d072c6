"""Per-pixel order statistics of posterior ensembles (driftSDE interval) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernel: `ops.ensemble_order_stats` at 256x256, batch 16, S in {4, 8, 16, 32}, the four order statistics of a 0.9 interval (lo, hi
      and the two medians), in the auto form -- at S = 16 also the network and the rank form by name -- against `torch.sort` over the
      members of the same tensor (what a caller had to do without it) and `ops.ensemble_stats`, which reads the same bytes.  HIP events
      around `--launches` back-to-back launches, the candidates alternated over `--rounds` rounds, median of the rounds (the method of
      scripts/bench_ensemble.py; every time includes the output allocation of its call).
  (b) calls: wall time of one `reverse_ddpm_ensemble` call at HxH, `num_samples: S`, `sample_T: K`, with and without `interval`: host
      clock around the call plus a synchronise, the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_ensemble_interval.py [--T 100 --K 10 --H 224 --S 8 --calls 5 --launches 200 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_ensemble_interval {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per launch of each round]}: the candidates alternated round by round, `launches` back-to-back launches per timing"""
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


def kernel_times(args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import order_stat_indices
    rows = []
    B, H = 16, 256
    for S in (4, 8, 16, 32):
        x = (0.5 * torch.randn(B, S, 1, H, H)).to(dev)
        idx = order_stat_indices(S, 0.9)
        ks = [idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]]
        fns = {"auto": lambda: ops.ensemble_order_stats(x, ks),
               "torch_sort": lambda: torch.sort(x, dim=1),
               "ensemble_stats": lambda: ops.ensemble_stats(x)}
        if S == 16:
            fns["network"] = lambda: ops.ensemble_order_stats(x, ks, algo=ops.ORDER_NETWORK)
            fns["rank"] = lambda: ops.ensemble_order_stats(x, ks, algo=ops.ORDER_RANK)
        want = torch.sort(x, dim=1).values[:, ks]
        for name in ("auto", "network", "rank"):
            if name in fns:
                assert torch.equal(fns[name](), want), (S, name)
        res = event_time(fns, args.launches, args.rounds)
        nbytes = (S + len(ks)) * 4 * B * H * H
        row = dict(B=B, S=S, H=H, ks=ks, auto_form="network" if S <= 16 else "rank", bytes=nbytes, launches=args.launches, rounds=args.rounds)
        for k, v in res.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_rounds"] = [round(t, 2) for t in v]
        row["auto_GBps"] = round(nbytes / row["auto_us"] * 1e-3, 1)
        row["torch_sort_over_auto"] = round(row["torch_sort_us"] / row["auto_us"], 2)
        row["auto_over_ensemble_stats"] = round(row["auto_us"] / row["ensemble_stats_us"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K, num_samples=args.S))
    model.set_eval()
    batch = make_batch(1, args.H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    times = {"plain": [], "interval": []}
    for i in range(args.calls + 1):
        for name, level in (("plain", None), ("interval", 0.9)):
            sde.set_seed(100 + i)
            sde.set_interval(level)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sde.reverse_ddpm_ensemble(cond, batch['names'], model.text_encoder, image_context=ctx)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K and sde.last_mode == "graph" and (sde.last_order_stats is None) == (level is None)
    row = dict(H=args.H, T=args.T, K=args.K, S=args.S, level=0.9, calls=args.calls)
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["interval_minus_plain_ms"] = round(row["interval_ms_median"] - row["plain_ms_median"], 3)
    row["plain_spread_ms"] = round(max(row["plain_ms"]) - min(row["plain_ms"]), 3)
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10, help="jumps per chain of the call-time part")
    ap.add_argument("--H", type=int, default=224)
    ap.add_argument("--S", type=int, default=8, help="members of the call-time part")
    ap.add_argument("--calls", type=int, default=5, help="timed repetitions (after one untimed)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ensemble_interval needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE ensemble order statistics: ensemble_order_stats vs torch.sort and ensemble_stats; a call with and without interval",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["order_stats"] = kernel_times(args, dev)
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
