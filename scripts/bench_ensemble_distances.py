"""Ensemble member distances (the S x S matrix of image-to-image distances, the medoid and the best member) on the clock.  Prints one JSON
line; bench.py is not involved.

  (a) kernel: `ops.ensemble_distances` at 256x256, batch 16, S in {4, 8, 16, 32}, with and without the target, against the torch
      composition of the same matrix in float64 (the finite mask over all rows, `torch.cdist` of the masked float64 rows without the
      Gram form, the counts and the two argmins), against `ops.ensemble_scores` on the same tensors, and `ops.ensemble_pick_rows`.  HIP
      events around `--launches` back-to-back calls, the candidates alternated over `--rounds` rounds, median with min - max of the
      rounds (the method of scripts/bench_ensemble_scores.py; every time includes the output and workspace allocations of its call
      and both launches of the two-launch calls).  `fp64_Tops` is the first launch's arithmetic over the whole call's time: 2 fp64
      operations (a subtraction and an fma) per element and computed pair, 64 pairs per off-diagonal 8 x 8 tile and 28 per diagonal
      one; a lower bound of the rate the kernel reaches.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: K` -- with and
      without `model.member_distances()`, both `model.pick_member` calls and the host summary: host clock around the call plus a
      synchronise, the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_ensemble_distances.py [--T 100 --K 10 --H 224 --S 8 --calls 5 --launches 50 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_ensemble_distances {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per call of each round]}: the candidates alternated round by round, `launches` back-to-back calls per timing"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
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


def torch_distances(x, y):
    """what a caller composes from ATen: (d2 [B, M, M] float64, counts [B, 2], pick [B, 2])"""
    B, S = x.shape[:2]
    rows = torch.cat([x.flatten(2), y.flatten(1)[:, None]], dim=1)
    valid = torch.isfinite(rows).all(dim=1)
    r64 = torch.where(valid[:, None], rows, torch.zeros((), device=x.device)).double()
    dist = torch.cdist(r64, r64, compute_mode="donot_use_mm_for_euclid_dist")
    nv = valid.sum(dim=1)
    counts = torch.stack([nv, valid.shape[1] - nv], dim=1)
    pick = torch.stack([dist[:, :S, :S].sum(dim=2).argmin(dim=1), dist[:, :S, S].argmin(dim=1)], dim=1)
    return dist * dist, counts, pick


def computed_pairs(M):
    nt = (M + 7) // 8
    return 28 * nt + 64 * nt * (nt - 1) // 2


def kernel_times(args, dev):
    from instancediff_amd import ops
    rows = []
    B, H = 16, 256
    for S in (4, 8, 16, 32):
        y = (torch.rand(B, 1, H, H) * 2 - 1).to(dev)
        x = (y.cpu()[:, None] + 0.1 * torch.randn(B, S, 1, H, H)).to(dev)
        pick = ops.ensemble_distances(x, y)[2]
        fns = {"distances": lambda: ops.ensemble_distances(x, y),
               "distances_no_target": lambda: ops.ensemble_distances(x),
               "pick_rows": lambda: ops.ensemble_pick_rows(x, pick, 0),
               "scores": lambda: ops.ensemble_scores(x, y),
               "torch": lambda: torch_distances(x, y)}
        d2, counts, _ = fns["distances"]()
        t_d2, t_counts, t_pick = fns["torch"]()
        assert torch.equal(counts.long(), t_counts) and torch.equal(pick.long(), t_pick), S
        assert torch.allclose(d2, t_d2, rtol=1e-9, atol=0), S
        res = event_time(fns, args.launches, args.rounds)
        pix = B * H * H
        row = dict(B=B, S=S, H=H, tile_pairs=((S + 8) // 8) * ((S + 8) // 8 + 1) // 2, launches=args.launches, rounds=args.rounds)
        for k, v in res.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        row["fp64_Tops"] = round(2 * computed_pairs(S + 1) * pix / row["distances_us"] * 1e-6, 2)
        row["pick_rows_TBps"] = round(2 * 4 * pix / row["pick_rows_us"] * 1e-6, 2)
        row["torch_over_distances"] = round(row["torch_us"] / row["distances_us"], 2)
        row["distances_over_scores"] = round(row["distances_us"] / row["scores_us"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import ensemble_distance_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    times = {"plain": [], "distances": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "distances"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "distances":
                d2, counts, _ = model.member_distances()
                model.pick_member("medoid"), model.pick_member("best")
                record = ensemble_distance_summary(d2, counts, args.S, True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K
    row = dict(H=args.H, T=args.T, K=args.K, S=args.S, calls=args.calls,
               last_record={k: record[k][0] for k in ("ES", "ES_FAIR", "DIVERSITY", "RMS_best", "RMS_medoid", "medoid", "best")})
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["distances_minus_plain_ms"] = round(row["distances_ms_median"] - row["plain_ms_median"], 3)
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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ensemble_distances needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE ensemble member distances: ensemble_distances vs a float64 torch composition and ensemble_scores; a call with "
                      "and without the distances and picks",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["distances"] = kernel_times(args, dev)
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
