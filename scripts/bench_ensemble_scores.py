"""Ensemble scores (CRPS, rank histogram, spread-skill sums) of posterior ensembles on the clock.  Prints one JSON line; bench.py is not
involved.

  (a) kernel: `ops.ensemble_scores` at 256x256, batch 16, S in {4, 8, 16, 32}, with and without the CRPS map, against the two kernels
      that stream the same tensor -- `ops.ensemble_stats` and `ops.ensemble_order_stats` (the four order statistics of a 0.9 interval)
      -- and against the torch composition a caller had to write without it (`torch.sort` over the members, the absolute and signed
      sums, `var`, the rank of the truth and a `bincount` per image).  HIP events around `--launches` back-to-back calls, the candidates
      alternated over `--rounds` rounds, median with min - max of the rounds (the method of scripts/bench_ensemble_interval.py; every
      time includes the output and workspace allocations of its call and, for `ensemble_scores`, both of its launches).
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: K` -- with and
      without `model.score_ensemble(want_map=True)` and the host copy of its sums and counts: host clock around the call plus a
      synchronise, the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_ensemble_scores.py [--T 100 --K 10 --H 224 --S 8 --calls 5 --launches 200 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_ensemble_scores {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per call of each round]}: the candidates alternated round by round, `launches` back-to-back calls per timing"""
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


def torch_scores(x, y):
    """what a caller composes from ATen: (sums [B, 3], counts [B, S + 1], crps map), float32 sums"""
    B, S = x.shape[:2]
    d = x - y[:, None]
    srt = torch.sort(d, dim=1).values
    c = (2 * torch.arange(S, device=x.device, dtype=torch.float32) - S + 1).view((1, S) + (1,) * (x.dim() - 2))
    crps = d.abs().sum(dim=1) / S - (c * srt).sum(dim=1) / (S * S)
    e = d.mean(dim=1) ** 2
    v = d.var(dim=1, unbiased=True)
    k = (d < 0).sum(dim=1).flatten(1)
    counts = torch.stack([torch.bincount(k[b], minlength=S + 1) for b in range(B)])
    return torch.stack([crps.flatten(1).sum(1), e.flatten(1).sum(1), v.flatten(1).sum(1)], dim=1), counts, crps


def kernel_times(args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import order_stat_indices
    rows = []
    B, H = 16, 256
    for S in (4, 8, 16, 32):
        y = (torch.rand(B, 1, H, H) * 2 - 1).to(dev)
        x = (y.cpu()[:, None] + 0.1 * torch.randn(B, S, 1, H, H)).to(dev)
        idx = order_stat_indices(S, 0.9)
        ks = [idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]]
        fns = {"scores": lambda: ops.ensemble_scores(x, y),
               "scores_map": lambda: ops.ensemble_scores(x, y, want_map=True),
               "ensemble_stats": lambda: ops.ensemble_stats(x),
               "order_stats": lambda: ops.ensemble_order_stats(x, ks),
               "torch": lambda: torch_scores(x, y)}
        sums, counts, crps = fns["scores_map"]()
        t_sums, t_counts, t_crps = fns["torch"]()
        assert torch.equal(counts[:, :S + 1].long(), t_counts) and not counts[:, S + 1].any(), S
        assert torch.allclose(crps, t_crps, rtol=0, atol=1e-5) and torch.allclose(sums.float(), t_sums, rtol=1e-3), S
        res = event_time(fns, args.launches, args.rounds)
        pix = B * H * H
        nbytes = {"scores": (S + 1) * 4 * pix, "scores_map": (S + 2) * 4 * pix, "ensemble_stats": (S + 2) * 4 * pix,
                  "order_stats": (S + len(ks)) * 4 * pix}
        row = dict(B=B, S=S, H=H, form="register" if S <= 16 else "second-read", bytes=nbytes, launches=args.launches, rounds=args.rounds)
        for k, v in res.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            if k in nbytes:
                row[f"{k}_TBps"] = round(nbytes[k] / statistics.median(v) * 1e-6, 2)
        row["scores_over_order_stats"] = round(row["scores_us"] / row["order_stats_us"], 2)
        row["scores_over_ensemble_stats"] = round(row["scores_us"] / row["ensemble_stats_us"], 2)
        row["scores_map_over_scores"] = round(row["scores_map_us"] / row["scores_us"], 2)
        row["torch_over_scores_map"] = round(row["torch_us"] / row["scores_map_us"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import ensemble_score_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    times = {"plain": [], "scores": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "scores"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "scores":
                sums, counts, _ = model.score_ensemble(want_map=True)
                record = ensemble_score_summary(sums.cpu(), counts.cpu(), args.S)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K
    row = dict(H=args.H, T=args.T, K=args.K, S=args.S, calls=args.calls, last_record={k: record[k] for k in ("CRPS", "SSR", "RANK_DEV", "OUTLIERS")})
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["scores_minus_plain_ms"] = round(row["scores_ms_median"] - row["plain_ms_median"], 3)
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
    assert torch.cuda.is_available(), "bench_ensemble_scores needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE ensemble scores: ensemble_scores vs ensemble_stats, ensemble_order_stats and a torch composition; a call with "
                      "and without scoring",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["scores"] = kernel_times(args, dev)
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
