"""No-reference despeckling statistics on the clock.  Prints one JSON line; bench.py is not involved.

  (a) kernel: `ops.despeckle_stats` at 256x256, batch 16 and 224x224, batch 8, S in {1, 8, 16}, over three label maps -- one region
      (L = 1), a shared 8x8 grid (L = 64) and three intensity bands of the reference (`ops.band_labels`, L = 3, a map per image) --
      against `ops.region_scores` at S = 1 on the same tensors in the same process (that call streams the image once and runs 4 shuffle
      trees per label present; this one adds the stencil's loads and runs 12) and against a float64 torch composition of the same
      numbers (`F.conv2d` Laplacians, the three masks, `index_add_` by label).  HIP events around `--launches` back-to-back calls
      (`--torch-launches` for the composition), the candidates alternated over `--rounds` rounds in one process, median with min - max
      of the rounds; every time includes the output and workspace allocations of its call and both of its launches.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: J` -- with and
      without what `testUM --speckle` adds (the mean image against the input and the target, the members against the input, over an 8x8
      grid, the host copies, `despeckle_summary` and `homogeneous_cells`): host clock around the call plus a synchronise, the two
      alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_despeckle_stats.py [--T 100 --sample-T 10 --H 224 --S 8 --calls 5 --launches 200 --rounds 5 --parts kernel,calls --out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_despeckle_stats {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per call of each round]}: the candidates alternated round by round, launches[name] back-to-back calls per timing"""
    res = {k: [] for k in fns}
    for name, fn in fns.items():
        for _ in range(min(10, launches[name])):
            fn()
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(launches[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / launches[name])
    return res


def torch_despeckle_stats(x, ref, labels, L, scale=0.5, shift=0.5, floor=2.0 ** -8):
    """what a caller composes from ATen: (sums float64 [B, S, L, 12], counts int64 [B, S, L, 3]) of the contract in include/idiff.h with
    float64 per-pixel terms; x [B, S, 1, H, W], ref [B, 1, H, W], labels uint8 [B, 1, H, W] or [1, H, W]"""
    B, S, _, H, W = x.shape
    a = (x.double() * scale + shift).view(B * S, 1, H, W)
    y = (ref.double() * scale + shift)[:, None].expand(B, S, 1, H, W).reshape(B * S, 1, H, W)
    valid = torch.isfinite(a) & torch.isfinite(y)
    ratio = valid & (a >= floor)
    rho = torch.where(ratio, y / torch.where(ratio, a, torch.ones_like(a)), torch.zeros_like(a))
    lap = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], device=x.device, dtype=torch.float64)[None, None]
    la = F.pad(F.conv2d(torch.where(valid, a, torch.zeros_like(a)), lap), (1, 1, 1, 1))
    ly = F.pad(F.conv2d(torch.where(valid, y, torch.zeros_like(y)), lap), (1, 1, 1, 1))
    sten = F.pad(F.conv2d(valid.double(), lap.abs().clamp(max=1.0)), (1, 1, 1, 1)) == 5.0
    masks = [valid] * 5 + [ratio] * 2 + [sten] * 5
    terms = [a, a * a, y, y * y, a * y, rho, rho * rho, la, ly, la * la, ly * ly, la * ly]
    terms = torch.stack([torch.where(m, t, torch.zeros_like(t)).flatten() for m, t in zip(masks, terms)], dim=1)
    lab = (labels.long().expand(B, 1, H, W) if labels.dim() == 3 else labels.long())[:, None].expand(B, S, 1, H, W).reshape(B * S, -1)
    inside = (lab < L).flatten()
    idx = (lab + L * torch.arange(B * S, device=x.device)[:, None]).flatten()[inside]
    sums = torch.zeros(B * S * L, 12, device=x.device, dtype=torch.float64).index_add_(0, idx, terms[inside])
    flags = torch.stack([valid.flatten(), ratio.flatten(), sten.flatten()], dim=1)[inside].long()
    counts = torch.zeros(B * S * L, 3, device=x.device, dtype=torch.int64).index_add_(0, idx, flags)
    return sums.view(B, S, L, 12), counts.view(B, S, L, 3)


def kernel_times(args, dev):
    from instancediff_amd import ops
    rows = []
    for B, H in ((16, 256), (8, 224)):
        n = H * H
        g = torch.Generator().manual_seed(H)
        scene = 0.5 + 0.3 * torch.sin(torch.arange(H)[:, None] * 0.05) * torch.cos(torch.arange(H)[None] * 0.03)
        noisy01 = (scene * torch.distributions.Gamma(4.0, 4.0).sample((B, 1, H, H))).clamp(0.0, 1.0)
        ref = (noisy01 * 2 - 1).to(dev)
        maps = {"one": (torch.zeros(1, H, H, dtype=torch.uint8, device=dev), 1),
                "grid8x8": (ops.grid_labels(H, H, 8, 8, str(dev))[None].contiguous(), 64),
                "bands3": (ops.band_labels(ref, [-1.0 / 3.0, 1.0 / 3.0]), 3)}
        for S in (1, 8, 16):
            x = ((scene * (1 + 0.05 * torch.randn(B, S, 1, H, H, generator=g))).clamp(0.0, 1.0) * 2 - 1).to(dev)
            row = dict(B=B, H=H, S=S, launches=args.launches, torch_launches=args.torch_launches, rounds=args.rounds,
                       bytes=(S + 1) * 4 * B * n + B * n)
            x1, reff = x[:, 0].reshape(B, n).contiguous(), ref.view(B, n)
            fns = {"region_scores_S1": lambda: ops.region_scores(x1, reff, maps["one"][0].view(n), 1)}
            launches = {"region_scores_S1": args.launches}
            for name, (lab, L) in maps.items():
                sums, counts, outside = ops.despeckle_stats(x, ref, lab, L)
                t_sums, t_counts = torch_despeckle_stats(x, ref, lab, L)
                assert torch.equal(counts[..., :3].long(), t_counts) and not outside.any() and not counts[..., 3].any(), ("counts", S, name)
                # fp32 per-pixel terms against float64 ones: relative to the largest sum of the quantity (1e-4: an a near the floor 2^-8
                # carries 2^-16 of relative rounding, its rho^2 twice that, and such terms dominate sum rho^2), plus 4e-6 per pixel for
                # the signed stencil sums, which cancel (a Laplacian carries about 2^-19 of fp32 rounding)
                tol = 1e-4 * t_sums.abs().amax(dim=(0, 1, 2)) + 4e-6 * float(t_counts.max())
                worst = float(((sums - t_sums).abs() / tol).max())
                assert worst <= 1.0, ("sums differ from the torch composition", S, name, worst)
                fns[name] = (lambda lab=lab, L=L: ops.despeckle_stats(x, ref, lab, L))
                fns[f"torch_{name}"] = (lambda lab=lab, L=L: torch_despeckle_stats(x, ref, lab, L))
                launches[name], launches[f"torch_{name}"] = args.launches, args.torch_launches
            res = event_time(fns, launches, args.rounds)
            for k, v in res.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            for name in maps:
                row[f"{name}_over_region_scores_S1"] = round(row[f"{name}_us"] / row["region_scores_S1_us"], 2)
                row[f"torch_over_{name}"] = round(row[f"torch_{name}_us"] / row[f"{name}_us"], 2)
            log(json.dumps(row))
            rows.append(row)
    return dict(rows=rows)


def call_times(args, dev):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.models.SDEs.driftSDE import despeckle_summary, homogeneous_cells
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.sample_T, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    grid = ops.grid_labels(args.H, args.H, 8, 8, str(dev))
    times = {"plain": [], "speckle": []}
    record = auto = None
    for i in range(args.calls + 1):
        for name in ("plain", "speckle"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "speckle":
                for what, against in (("output", "input"), ("output", "target"), ("ensemble", "input")):
                    rec = [t.cpu() for t in model.despeckle_stats(grid, 64, what=what, against=against)]
                    record = despeckle_summary(*rec)
                    auto = homogeneous_cells(*rec[:2])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.sample_T
    enl = [q["ENL"] for r in record["rows"] for q in r if q["ENL"] is not None]
    row = dict(H=args.H, T=args.T, sample_T=args.sample_T, L=64, S=args.S, calls=args.calls,
               last_record=dict(ENL_member=sum(enl) / max(len(enl), 1), ENL_AUTO_member=auto["ENL_AUTO"]))
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["speckle_minus_plain_ms"] = round(row["speckle_ms_median"] - row["plain_ms_median"], 3)
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
    ap.add_argument("--torch-launches", type=int, default=3, help="back-to-back calls per timing of the torch composition")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_despeckle_stats needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="no-reference despeckling statistics: ops.despeckle_stats over three label maps vs ops.region_scores at S = 1 and a "
                      "float64 torch composition; a call with and without the statistics",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["despeckle_stats"] = kernel_times(args, dev)
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
