"""Sparsification curves of uncertainty maps on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernel: `ops.sparsification` for a map (the ensemble's std) and for the oracle (key=None) at 256x256 batch 16 and 224x224 batch 8,
      K in {20, 64}, against the float64 torch composition of the same numbers (the mapped keys, `torch.sort` descending, a gather, a
      cumulative sum, the tie groups by `searchsorted`) and against `ops.ensemble_scores` on the same ensemble, the scale of a
      neighbouring analysis.  HIP events around `--launches` back-to-back calls, the candidates alternated over `--rounds` rounds in one
      process, median with min - max of the rounds; every time includes the output and workspace allocations of its call and all of its
      launches.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: J` -- with and
      without `model.sparsification(K=20)`, the host copy of its records and `sparsification_summary`: host clock around the call plus a
      synchronise, the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_sparsification.py [--T 100 --sample-T 10 --H 224 --S 8 --calls 5 --launches 100 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_sparsification {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


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


def torch_sparsification(key, pred, target, K):
    """what a caller composes from ATen for NaN-free inputs: (sums float64 [B, K + 1, 2], counts int64 [B, K + 1, 2]) of the contract in
    include/idiff.h, by a full sort of every image"""
    B = pred.shape[0]
    d = (pred - target).flatten(1)
    e = d * d
    n = e.shape[1]
    k = e if key is None else key.flatten(1)
    b = k.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    u = torch.where(b >= 0x80000000, b ^ 0xffffffff, b | 0x80000000)
    srt, idx = torch.sort(u, dim=1, descending=True)
    cs = e.double().gather(1, idx).cumsum(1)
    cs0 = torch.cat([cs.new_zeros(B, 1), cs], dim=1)  # cs0[:, j] = the error of the first j pixels
    m = torch.tensor([(j * n) // K for j in range(K)], device=pred.device)
    live = m > 0
    tau = srt[:, (m - 1).clamp(min=0)]
    asc = srt.flip(1).contiguous()
    c = n - torch.searchsorted(asc, tau.contiguous(), right=True)
    ge = n - torch.searchsorted(asc, tau.contiguous(), right=False)
    A = cs0.gather(1, c)
    T = cs0.gather(1, ge) - A
    zero = torch.zeros_like(c)
    sums = torch.stack([torch.where(live, A, A.new_zeros(())), torch.where(live, T, T.new_zeros(()))], dim=2)
    counts = torch.stack([torch.where(live, c, zero), torch.where(live, ge - c, zero)], dim=2)
    last_s = torch.stack([cs[:, -1], cs.new_zeros(B)], dim=1)[:, None]
    last_c = torch.tensor([n, 0], device=pred.device).expand(B, 1, 2)
    return torch.cat([sums, last_s], dim=1), torch.cat([counts, last_c], dim=1)


def kernel_times(args, dev):
    from instancediff_amd import ops
    rows = []
    S = 8
    for B, H in ((16, 256), (8, 224)):
        y = (torch.rand(B, 1, H, H) * 2 - 1).to(dev)
        x = (y.cpu()[:, None] + 0.1 * torch.randn(B, S, 1, H, H) * torch.rand(B, 1, 1, H, H)).to(dev)
        mean, std = ops.ensemble_stats(x)
        for K in (20, 64):
            fns = {"map": lambda: ops.sparsification(std, mean, y, K),
                   "oracle": lambda: ops.sparsification(None, mean, y, K),
                   "torch_map": lambda: torch_sparsification(std, mean, y, K),
                   "ensemble_scores": lambda: ops.ensemble_scores(x, y)}
            for key, name in ((std, "map"), (None, "oracle")):
                sums, counts, _ = fns[name]()
                t_sums, t_counts = torch_sparsification(key, mean, y, K)
                assert torch.equal(counts.long(), t_counts), ("counts differ from the torch composition", B, H, K, name)
                # the composition's T is a difference of two cumulative sums: its error scales with the image's total, not with T
                worst = float(((sums - t_sums).abs() / sums[:, K:, :1]).max())
                assert worst <= 1e-10, ("sums differ from the torch composition", B, H, K, name, worst)
            res = event_time(fns, args.launches, args.rounds)
            pix = B * H * H
            # the selection reads key / pred / target and writes u, then reads u three times; the sums read u / pred / target per group of 8
            groups = (K + 7) // 8
            nbytes = {"map": (3 + 1 + 3 + 3 * groups) * 4 * pix, "oracle": (2 + 1 + 3 + 3 * groups) * 4 * pix}
            row = dict(B=B, H=H, K=K, S=S, bytes=nbytes, launches=args.launches, rounds=args.rounds)
            for k, v in res.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            row["torch_over_map"] = round(row["torch_map_us"] / row["map_us"], 2)
            row["map_over_ensemble_scores"] = round(row["map_us"] / row["ensemble_scores_us"], 2)
            log(json.dumps(row))
            rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import sparsification_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.sample_T, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    times = {"plain": [], "sparsification": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "sparsification"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "sparsification":
                rec = [t.cpu() for t in model.sparsification(K=20)[:4]]
                record = sparsification_summary(*rec, 20)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.sample_T
    row = dict(H=args.H, T=args.T, sample_T=args.sample_T, K=20, S=args.S, calls=args.calls, last_record={k: record[k] for k in ("AUSE", "AURG", "AUSE_RMSE", "N")})
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["sparsification_minus_plain_ms"] = round(row["sparsification_ms_median"] - row["plain_ms_median"], 3)
    row["plain_spread_ms"] = round(max(row["plain_ms"]) - min(row["plain_ms"]), 3)
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sample-T", type=int, default=10, help="jumps per chain of the call-time part (the curve has K = 20 points there)")
    ap.add_argument("--H", type=int, default=224)
    ap.add_argument("--S", type=int, default=8, help="members of the call-time part")
    ap.add_argument("--calls", type=int, default=5, help="timed repetitions (after one untimed)")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sparsification needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="sparsification curves: ops.sparsification (map, oracle) vs a float64 torch composition by torch.sort and vs "
                      "ensemble_scores; a call with and without the curves",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["sparsification"] = kernel_times(args, dev)
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
