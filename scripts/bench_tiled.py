"""Tiled sampling (driftSDE tile / tile_overlap) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) calls: per-image time of a tiled `reverse_ddpm` at HxH (`tile`, `tile_overlap`, `sample_T: K`, batch 1) against the whole-image
      chain of the same size in the same process, the same seed: HIP events around each call plus a synchronise, the two forms
      alternated over `--calls` repetitions after one untimed, median and spread of the repetitions; the PSNR between the two results
      (ops.image_metrics, the tiled result against the whole-image one).
  (b) step kernel: per-launch time of `ops.drift_reverse_step_tiled_dev` against `ops.drift_reverse_step_dev` on the same full image,
      on-device noise: HIP events around `--launches` back-to-back launches, the kernels alternated over `--rounds` rounds, median of the
      rounds (the method of scripts/bench_ensemble.py).  Effective bytes: the plain step reads x, r, e, cond and writes x, xa: 24 bytes per
      pixel; the tiled step reads x, cond and one prediction pair per weighted window, writes x and one input pair per covering window:
      counted from the plan's tables.

    python scripts/bench_tiled.py [--T 100 --K 10 --cases 512:256:32,448:224:28 --calls 3 --launches 200 --rounds 5 --parts calls,kernel --out FILE]
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
    print(f"[bench_tiled {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


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


def call_times(H, tile, overlap, args, dev):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K))
    model.set_eval()
    batch = make_batch(1, H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    times, outs, grid = {"tiled": [], "whole": []}, {}, None
    for i in range(args.calls + 1):
        for form in ("tiled", "whole"):
            sde.set_tiling(tile if form == "tiled" else None, overlap if form == "tiled" else None)
            sde.set_seed(100)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx)
            e1.record()
            torch.cuda.synchronize()
            times[form].append(e0.elapsed_time(e1))
            assert sde.last_steps == args.K and sde.last_mode == "graph", (sde.last_steps, sde.last_mode)
            assert (sde.last_tiles is not None) == (form == "tiled")
            outs[form] = out.clone()
            if form == "tiled":
                grid = sde.last_tiles
    met = ops.image_metrics(outs["tiled"][:, 0].contiguous(), outs["whole"][:, 0].contiguous()).cpu().tolist()[0]
    row = dict(H=H, T=args.T, K=args.K, tile=tile, tile_overlap=overlap, windows=list(grid), max_batch=sde.max_batch,
               psnr_tiled_vs_whole_dB=round(met[1], 2), weights="random init (no checkpoint): the PSNR compares two chains of untrained nets")
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 2)
        row[f"{k}_ms"] = [round(t, 2) for t in v]
    row["whole_over_tiled"] = round(row["whole_ms_median"] / row["tiled_ms_median"], 2)
    log(json.dumps(row))
    del model, sde
    torch.cuda.empty_cache()
    return row


def kernel_times(H, tile, overlap, args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import TilePlan, _tile_overlap
    plan = TilePlan(H, H, (tile, tile), (_tile_overlap(overlap, tile),) * 2).to(dev)
    ny, nx, Ph, Pw = plan.grid
    shp, tshp = (1, 1, H, H), (ny * nx, 1, Ph, Pw)
    n = H * H
    g = torch.Generator().manual_seed(0)
    x0, r, e, cond = (torch.randn(shp, generator=g).to(dev) for _ in range(4))
    xa = torch.empty(shp, device=dev)
    r_t, e_t = ops.tile_gather(r, plan), ops.tile_gather(e, plan)
    x_t, xa_t = torch.empty(tshp, device=dev), torch.empty(tshp, device=dev)
    Tp1, t = 8, 5
    tb = torch.zeros(3, Tp1)
    tb[:, t] = torch.tensor([1e-3, 1e-3, 1e-3])  # small a, b, c: x stays finite over thousands of in-place launches
    coef3 = tb.to(dev).contiguous()
    state = torch.tensor([t, 0, 0], dtype=torch.int32, device=dev)
    x = x0.clone()
    fns = {
        "step_dev": lambda: ops.drift_reverse_step_dev(x, r, e, None, cond, xa, coef3, state, 1, n // 4, 0),
        "tiled": lambda: ops.drift_reverse_step_tiled_dev(x, r_t, e_t, None, None, None, cond, x_t, xa_t, plan, coef3, state, 1, n // 4, 0),
    }
    res = event_time(fns, args.launches, args.rounds)
    assert torch.isfinite(x).all()
    # per pixel: weighted windows (reads of r and e) and covering windows (writes of x and xa), from the tables
    wts = [(ax["w1"] != 0).astype(int) + 1 for ax in (plan.y, plan.x)]
    cov = [ax["cov_hi"] - ax["cov_lo"] for ax in (plan.y, plan.x)]
    reads, writes = int(wts[0].sum()) * int(wts[1].sum()), int(cov[0].sum()) * int(cov[1].sum())
    bytes_plain, bytes_tiled = 24 * n, 4 * (3 * n + 2 * reads + 2 * writes)
    row = dict(H=H, tile=tile, tile_overlap=overlap, windows=[ny, nx, Ph, Pw], launches=args.launches, rounds=args.rounds,
               noise="on-device Philox", bytes_plain=bytes_plain, bytes_tiled=bytes_tiled)
    for k, v in res.items():
        row[f"{k}_us"] = round(statistics.median(v), 2)
        row[f"{k}_us_rounds"] = [round(t, 2) for t in v]
    row["step_dev_GBps"] = round(bytes_plain / row["step_dev_us"] * 1e-3, 1)
    row["tiled_GBps"] = round(bytes_tiled / row["tiled_us"] * 1e-3, 1)
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10, help="jumps per chain of the call-time part")
    ap.add_argument("--cases", type=str, default="512:256:32,448:224:28", help="H:tile:overlap, comma separated")
    ap.add_argument("--calls", type=int, default=3, help="timed repetitions per case (after one untimed)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="calls,kernel")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in args.cases.split(",")]
    assert torch.cuda.is_available(), "bench_tiled needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE tiled sampling: tiled chain vs whole-image chain at batch 1, tiled step kernel vs plain step kernel",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["step_kernel"] = [kernel_times(*c, args, dev) for c in cases]
    if "calls" in parts:
        res["calls"] = [call_times(*c, args, dev) for c in cases]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
