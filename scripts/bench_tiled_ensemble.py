"""Posterior ensembles of tiled chains (driftSDE tiled_ensemble) on the clock.  One process, prints one JSON line; bench.py is not involved.

  (a) step kernel: per-launch time of `ops.drift_reverse_step_tiled_members_dev` on R full-resolution rows against
      `ops.drift_reverse_step_tiled_dev` at B = R on the same operands (the same bytes, the kernel the tiled chain already had),
      on-device noise: HIP events around `--launches` back-to-back launches, the two alternated over `--rounds` rounds, median and
      min - max of the rounds.
  (b) calls: per-image time of `reverse_ddpm_ensemble` at HxH (`tile`, `tile_overlap`, `sample_T: K`, S members) with
      `max_chain_rows` = nwin (one member per chain), 128 (the default) and all rows (one chain), against S sequential
      `reverse_ddpm_tiled` calls: HIP events around each form plus a synchronise, the forms alternated over `--calls` repetitions after
      one untimed, median and min - max.

    python scripts/bench_tiled_ensemble.py [--T 100 --K 10 --case 512:256:32 --rows 4,8,16 --members 4,8 --calls 3 --launches 200
                                            --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_tiled_ensemble {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(v, nd=2):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd), all=[round(t, nd) for t in v])


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


def kernel_times(H, tile, overlap, R, args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import TilePlan, _tile_overlap
    plan = TilePlan(H, H, (tile, tile), (_tile_overlap(overlap, tile),) * 2).to(dev)
    ny, nx, Ph, Pw = plan.grid
    shp, tshp = (R, 1, H, H), (R * ny * nx, 1, Ph, Pw)
    n = R * H * H
    g = torch.Generator().manual_seed(0)
    x0, r, e, cond = (torch.randn(shp, generator=g).to(dev) for _ in range(4))
    r_t, e_t = ops.tile_gather(r, plan), ops.tile_gather(e, plan)
    x_t, xa_t = torch.empty(tshp, device=dev), torch.empty(tshp, device=dev)
    Tp1, t = 8, 5
    tb = torch.zeros(3, Tp1)
    tb[:, t] = torch.tensor([1e-3, 1e-3, 1e-3])  # small a, b, c: x stays finite over thousands of in-place launches
    coef3 = tb.to(dev).contiguous()
    state = torch.tensor([t, 0, 0], dtype=torch.int32, device=dev)
    mdev = ops.member_ids(range(1, R + 1), dev)
    x = x0.clone()
    fns = {
        "tiled": lambda: ops.drift_reverse_step_tiled_dev(x, r_t, e_t, None, None, None, cond, x_t, xa_t, plan, coef3, state, 1, n // 4, 0),
        "tiled_members": lambda: ops.drift_reverse_step_tiled_members_dev(x, r_t, e_t, None, None, None, cond, x_t, xa_t, plan, coef3, state,
                                                                          mdev, 1),
    }
    res = event_time(fns, args.launches, args.rounds)
    assert torch.isfinite(x).all()
    # per pixel: weighted windows (reads of r and e) and covering windows (writes of x and xa), from the tables
    wts = [(ax["w1"] != 0).astype(int) + 1 for ax in (plan.y, plan.x)]
    cov = [ax["cov_hi"] - ax["cov_lo"] for ax in (plan.y, plan.x)]
    reads, writes = int(wts[0].sum()) * int(wts[1].sum()), int(cov[0].sum()) * int(cov[1].sum())
    nbytes = R * 4 * (3 * H * H + 2 * reads + 2 * writes)
    row = dict(H=H, tile=tile, tile_overlap=overlap, windows=[ny, nx, Ph, Pw], R=R, launches=args.launches, rounds=args.rounds,
               noise="on-device Philox", bytes=nbytes)
    for k, v in res.items():
        row[f"{k}_us"] = spread(v)
        row[f"{k}_GBps"] = round(nbytes / statistics.median(v) * 1e-3, 1)
    row["members_over_tiled"] = round(row["tiled_members_us"]["median"] / row["tiled_us"]["median"], 3)
    log(json.dumps(row))
    return row


def call_times(H, tile, overlap, args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0,
                                sde_overrides=dict(sample_T=args.K, tile=tile, tile_overlap=overlap, tiled_ensemble=True))
    model.set_eval()
    batch = make_batch(1, H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    plan = sde._tile_plan(H, H, dev)
    nwin = plan.ny * plan.nx
    rows = []
    for S in args.members:
        forms = {"sequential_tiled_calls": None, "chain_rows_nwin": nwin, "chain_rows_128": 128, "chain_rows_all": S * nwin}
        times = {k: [] for k in forms}
        for i in range(args.calls + 1):
            for form, mcr in forms.items():
                sde.set_seed(100)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if mcr is None:
                    for _ in range(S):
                        sde.reverse_ddpm_tiled(cond, batch['names'], model.text_encoder, image_context=ctx)
                else:
                    sde.set_num_samples(S, max_chain_rows=mcr)
                    sde.reverse_ddpm_ensemble(cond, batch['names'], model.text_encoder, image_context=ctx)
                    sde.set_num_samples(None)
                e1.record()
                torch.cuda.synchronize()
                times[form].append(e0.elapsed_time(e1))
                assert sde.last_steps == args.K and sde.last_mode == "graph" and sde.last_tiles == plan.grid, (sde.last_steps, sde.last_mode)
        row = dict(H=H, T=args.T, K=args.K, S=S, tile=tile, tile_overlap=overlap, windows=list(plan.grid), max_batch=sde.max_batch,
                   chains={k: (S if v is None else len(range(0, S, max(1, v // nwin)))) for k, v in forms.items()},
                   weights="random init (no checkpoint)")
        for k, v in times.items():
            row[f"{k}_ms"] = spread(v[1:])  # the first repetition fills the weight / text caches
        base = row["sequential_tiled_calls_ms"]["median"]
        for k in forms:
            row[f"{k}_over_sequential"] = round(row[f"{k}_ms"]["median"] / base, 3)
        log(json.dumps(row))
        rows.append(row)
    del model, sde
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10, help="jumps per chain of the call-time part")
    ap.add_argument("--case", type=str, default="512:256:32", help="H:tile:overlap")
    ap.add_argument("--rows", type=str, default="4,8,16", help="R of the step-kernel part, comma separated")
    ap.add_argument("--members", type=str, default="4,8", help="S of the call-time part, comma separated")
    ap.add_argument("--calls", type=int, default=3, help="timed repetitions per form (after one untimed)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    H, tile, overlap = (int(v) for v in args.case.split(":"))
    args.members = [int(v) for v in args.members.split(",")]
    assert torch.cuda.is_available(), "bench_tiled_ensemble needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE ensembles of tiled chains: member step kernel vs tiled step kernel at B = R; ensemble call vs S sequential "
                      "tiled calls and vs max_chain_rows",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["step_kernel"] = [kernel_times(H, tile, overlap, int(R), args, dev) for R in args.rows.split(",")]
    if "calls" in parts:
        res["calls"] = call_times(H, tile, overlap, args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
