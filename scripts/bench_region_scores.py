"""Region-wise ensemble scores on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernel: `ops.region_scores` at 256x256, batch 16, S in {1, 4, 8, 16, 32}, over four label maps -- one region (L = 1), a shared 4x4
      grid (L = 16), three intensity bands of the truth (`ops.band_labels`, L = 3, a map per image) and, as the stated worst case, a
      per-pixel random map with L = 64 (every wave holds every label) -- against `ops.ensemble_scores` on the same tensors (the fused
      kernel does that kernel's work plus the label reductions) and against a float64 torch composition of the same numbers (the CRPS / e /
      v / m maps by a sort of the members, then `index_add_` and `bincount` by label).  HIP events around `--launches` back-to-back
      calls, the candidates alternated over `--rounds` rounds in one process, median with min - max of the rounds; every time includes the
      output and workspace allocations of its call and both of its launches.  `ops.band_labels` is timed beside them.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: J` -- with and
      without `model.region_scores` over a 4x4 grid, the host copy of its records and `region_score_summary`: host clock around the call
      plus a synchronise, the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_region_scores.py [--T 100 --sample-T 10 --H 224 --S 8 --calls 5 --launches 200 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_region_scores {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per call of each round]}: the candidates alternated round by round, `launches` back-to-back calls per timing"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(10):
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


def torch_region_scores(x, y, labels, L):
    """what a caller composes from ATen for NaN-free inputs: (sums float64 [B, L, 4], counts int64 [B, L, S + 1]) of the contract in
    include/idiff.h; labels uint8 [B, n] or [n]"""
    B, S = x.shape[:2]
    d = (x.flatten(2) - y.flatten(1)[:, None]).double()
    ds, _ = d.sort(dim=1)
    c = (2 * torch.arange(S, device=x.device, dtype=torch.float64) - S + 1)[None, :, None]
    crps = d.abs().mean(dim=1) - (c * ds).sum(dim=1) / (S * S)
    m = d.mean(dim=1)
    v = d.var(dim=1, unbiased=True) if S > 1 else torch.zeros_like(m)
    k = (d < 0).sum(dim=1)
    lab = labels.long().expand(B, -1) if labels.dim() == 1 else labels.long()
    inside = lab < L
    idx = (lab + L * torch.arange(B, device=x.device)[:, None])[inside]
    terms = torch.stack([crps, m * m, v, m], dim=2)[inside]
    sums = torch.zeros(B * L, 4, device=x.device, dtype=torch.float64).index_add_(0, idx, terms)
    counts = torch.bincount(idx * (S + 1) + k[inside], minlength=B * L * (S + 1))
    return sums.view(B, L, 4), counts.view(B, L, S + 1)


def kernel_times(args, dev):
    from instancediff_amd import ops
    rows = []
    B, H = 16, 256
    n = H * H
    y = (torch.rand(B, 1, H, H) * 2 - 1).to(dev)
    maps = {"one": (torch.zeros(n, dtype=torch.uint8, device=dev), 1),
            "grid4x4": (ops.grid_labels(H, H, 4, 4, str(dev)).reshape(-1), 16),
            "bands3": (ops.band_labels(y, [-1.0 / 3.0, 1.0 / 3.0]).view(B, n), 3),
            "random64": (torch.randint(0, 64, (B, n), dtype=torch.uint8).to(dev), 64)}
    band = event_time({"band_labels": lambda: ops.band_labels(y, [-1.0 / 3.0, 1.0 / 3.0])}, args.launches, args.rounds)["band_labels"]
    for S in (1, 4, 8, 16, 32):
        x = (y.cpu()[:, None] + 0.1 * torch.randn(B, S, 1, H, H) * torch.rand(B, 1, 1, H, H)).to(dev)
        xf, yf = x.view(B, S, n), y.view(B, n)
        row = dict(B=B, H=H, S=S, launches=args.launches, rounds=args.rounds, bytes=(S + 1) * 4 * B * n + B * n)
        fns = {"ensemble_scores": lambda: ops.ensemble_scores(xf, yf)}
        for name, (lab, L) in maps.items():
            sums, counts, outside = ops.region_scores(xf, yf, lab, L)
            t_sums, t_counts = torch_region_scores(xf, yf, lab, L)
            assert torch.equal(counts[:, :, :S + 1].long(), t_counts) and not outside.any(), ("counts differ from the torch composition", S, name)
            scale = t_sums.abs().amax(dim=(0, 1)).clamp(min=1e-30)
            worst = float(((sums - t_sums).abs() / scale).max())
            assert worst <= 1e-5, ("sums differ from the torch composition", S, name, worst)  # fp32 per-pixel terms against float64 ones
            fns[name] = (lambda lab=lab, L=L: ops.region_scores(xf, yf, lab, L))
            fns[f"torch_{name}"] = (lambda lab=lab, L=L: torch_region_scores(xf, yf, lab, L))
        res = event_time(fns, args.launches, args.rounds)
        for k, v in res.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        for name in maps:
            row[f"{name}_over_ensemble_scores"] = round(row[f"{name}_us"] / row["ensemble_scores_us"], 2)
            row[f"torch_over_{name}"] = round(row[f"torch_{name}_us"] / row[f"{name}_us"], 2)
        log(json.dumps(row))
        rows.append(row)
    return dict(rows=rows, band_labels_us=round(statistics.median(band), 2), band_labels_us_min_max=[round(min(band), 2), round(max(band), 2)])


def call_times(args, dev):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.models.SDEs.driftSDE import region_score_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.sample_T, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    grid = ops.grid_labels(args.H, args.H, 4, 4, str(dev))
    times = {"plain": [], "regions": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "regions"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "regions":
                rec = [t.cpu() for t in model.region_scores(grid, 16)]
                record = region_score_summary(*rec, args.S)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.sample_T
    row = dict(H=args.H, T=args.T, sample_T=args.sample_T, L=16, S=args.S, calls=args.calls,
               last_record=dict(N_PIX=record["N_PIX"], RMSE=[r["RMSE"] for r in record["regions"]], SSR=[r["SSR"] for r in record["regions"]]))
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["regions_minus_plain_ms"] = round(row["regions_ms_median"] - row["plain_ms_median"], 3)
    row["plain_spread_ms"] = round(max(row["plain_ms"]) - min(row["plain_ms"]), 3)
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sample-T", type=int, default=10, help="jumps per chain of the call-time part")
    ap.add_argument("--H", type=int, default=224)
    ap.add_argument("--S", type=int, default=8, help="members of the call-time part")
    ap.add_argument("--calls", type=int, default=5, help="timed repetitions (after one untimed)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_region_scores needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="region-wise ensemble scores: ops.region_scores over four label maps vs ops.ensemble_scores and a float64 torch "
                      "composition; a call with and without the regions",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["region_scores"] = kernel_times(args, dev)
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
