"""Principal modes of a posterior ensemble (the eigen-decomposition of the members' centred Gram matrix and the mode images) on the clock.
Prints one JSON line; bench.py is not involved.

  (a) kernel: at 256x256, batch 16 and 224x224, batch 8, S in {4, 8, 16, 32}, K = 4: `ops.ensemble_modes` on a finished distance matrix
      (one launch, one block per image), `ops.ensemble_project` of the K leading coefficient rows (one launch), the whole
      `driftSDE.principal_modes` call (the distances' two launches and those two), `ops.ensemble_distances` alone, and the torch
      composition of the same result in float64: centred members, the Gram matrix by `matmul`, `torch.linalg.eigh`, the mode images and
      the target's coordinates by `matmul`.  Before timing, the two spectra, the mode images up to their sign and the coordinates are
      compared (`torch_agrees`).  HIP events
      around `--launches` back-to-back calls, the candidates alternated over `--rounds` rounds, median with min - max of the rounds (the
      method of scripts/bench_ensemble_distances.py; every time includes the output allocations of its call).  `project_TBps` counts
      (S + K) * 4 bytes per pixel.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: K` -- with and
      without `model.principal_modes(K=4)`, the host copy of its records and the summary: host clock around the call plus a synchronise,
      the two alternated over `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_ensemble_modes.py [--T 100 --K 10 --H 224 --S 8 --calls 5 --launches 50 --rounds 5 --parts kernel,calls --out FILE]
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

MODES = 4


def log(msg):
    print(f"[bench_ensemble_modes {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


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


def torch_modes(x, y, K):
    """what a caller composes from ATen in float64: (lam [B, S] descending, modes [B, K, n] float32, tcoord [B, K])"""
    X = x.flatten(2).double()
    c = X.mean(dim=1, keepdim=True)
    R = X - c
    lam, V = torch.linalg.eigh(R @ R.transpose(1, 2))
    lam, V = lam.flip(1), V.flip(2)
    coef = V[:, :, :K].transpose(1, 2) / lam[:, :K, None].sqrt()
    modes = coef @ R
    t = (modes @ (y.flatten(1).double() - c[:, 0])[:, :, None])[:, :, 0]
    return lam, modes.float(), t


def kernel_times(args, dev):
    from instancediff_amd import ops
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    rows = []
    for B, H in ((16, 256), (8, 224)):
        for S in (4, 8, 16, 32):
            K = min(MODES, S)
            y = (torch.rand(B, 1, H, H) * 2 - 1).to(dev)
            x = (y.cpu()[:, None] + 0.1 * torch.randn(B, S, 1, H, H)).to(dev)
            d2 = ops.ensemble_distances(x, y)[0]
            lam, vec, coef, tcoord, tnorm2, info = ops.ensemble_modes(d2, S, True)
            fns = {"modes": lambda: ops.ensemble_modes(d2, S, True),
                   "project": lambda: ops.ensemble_project(x, coef[:, :K]),
                   "principal_modes": lambda: driftSDE.principal_modes(x, y, K=K),
                   "distances": lambda: ops.ensemble_distances(x, y)}
            row = dict(B=B, S=S, H=H, K=K, launches=args.launches, rounds=args.rounds, sweeps=info[:, 1].tolist(), rank=info[:, 0].tolist())
            try:
                t_lam, t_modes, t_t = torch_modes(x, y, K)
                mine = fns["project"]().flatten(2)
                sign = (mine * t_modes).sum(dim=2, keepdim=True).sign()
                row["torch_agrees"] = bool(torch.allclose(lam[:, :S - 1], t_lam[:, :S - 1], rtol=1e-9, atol=0)
                                           and (mine - sign * t_modes).abs().max().item() <= 1e-6
                                           and torch.allclose(tcoord[:, :K], sign[:, :, 0].double() * t_t, rtol=0,
                                                              atol=1e-7 * float(tnorm2.max().sqrt())))
                fns["torch"] = lambda: torch_modes(x, y, K)
            except RuntimeError as e:  # an ATen build without a batched symmetric eigensolver: the row then has no torch column
                row["torch_error"] = str(e).splitlines()[0][:200]
            res = event_time(fns, args.launches, args.rounds)
            pix = B * H * H
            for k, v in res.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            row["project_TBps"] = round((S + K) * 4 * pix / row["project_us"] * 1e-6, 2)
            if "torch_us" in row:
                row["torch_over_principal_modes"] = round(row["torch_us"] / row["principal_modes_us"], 2)
            row["principal_modes_over_distances"] = round(row["principal_modes_us"] / row["distances_us"], 2)
            log(json.dumps(row))
            rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import ensemble_mode_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    times = {"plain": [], "modes": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "modes"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "modes":
                rec = model.principal_modes(K=MODES)
                record = ensemble_mode_summary(*(rec[q].cpu() for q in ("lam", "tcoord", "tnorm2", "info", "counts")), args.S, True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K
    row = dict(H=args.H, T=args.T, K=args.K, S=args.S, calls=args.calls,
               last_record={k: record[k][0] for k in ("EFF_MODES", "SPAN_SHARE", "MODE_Z_RMS", "rank", "sweeps")})
    row["last_record"]["EXPLAINED_1"] = record["EXPLAINED"][0][0]
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["modes_minus_plain_ms"] = round(row["modes_ms_median"] - row["plain_ms_median"], 3)
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
    assert torch.cuda.is_available(), "bench_ensemble_modes needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="driftSDE principal modes: ensemble_modes, ensemble_project and the whole principal_modes call vs ensemble_distances and a "
                      "float64 torch composition (matmul, linalg.eigh, matmul); a call with and without the modes",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["modes"] = kernel_times(args, dev)
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
