"""Graph reuse across driftSDE sampling calls (reuse_graph) on the clock.  Prints one JSON line; bench.py is not involved.

  (a) streams: 8 distinct images through `model.test()`, `sample_T: K`, with the option off (every call captures and frees its own step
      graph: the path of the commit before the option) and on, the two alternated pass by pass in one process over the same nets.
      Host clock around each `model.test()` plus a device synchronise; one untimed pass of each first, then `--passes` timed ones.
      Every timed pass with the option on starts from `close_sessions()`, so its first image captures and the other seven replay:
      the first image and the later ones are reported separately, as medians over the passes with their min and max.
      Workloads: 224x224 batch 1; 256x256 batch 16; 224x224 ensembles of 8, 16 (one chunk) and 24 members (two chunks, max_batch 16).
  (b) memory: `torch.cuda.memory_reserved()` after `empty_cache()` with the sessions of a pass open, and again after `close_sessions()`.
  (c) launch: `ops.chain_begin` against what it replaces (randn + axpby + clone + axpby and the two host-built state tensors), HIP
      events around `--launches` back-to-back repetitions, alternated over `--rounds` rounds.

    python scripts/bench_reuse_graph.py [--T 100 --K 10 --images 8 --passes 5 --parts streams,launch --out FILE]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_reuse_graph {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def reserved():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.memory_reserved()


def stream_times(name, H, B, S, args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    from instancediff_amd.utils.synthetic import make_batch
    model, base = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K))
    model.set_eval()
    sdes = {}
    for tag in ("off", "on"):
        s = driftSDE(nets=model.get_nets(), T=args.T, max_sigma=base.max_sigma, eta=base.eta, drift_schedule=base.schedule_names[0],
                     noise_schedule=base.schedule_names[1], sample_T=args.K, num_samples=S if S > 1 else None, max_batch=16,
                     reuse_graph=tag == "on")
        s.set_gpu(dev)
        sdes[tag] = s
    images = [make_batch(B, H, seed=100 + i) for i in range(args.images)]
    first = {"off": [], "on": []}
    later = {"off": [], "on": []}
    held = []
    for p in range(args.passes + 1):
        for tag in ("off", "on"):
            sde = sdes[tag]
            model.set_sde(sde)
            sde.close_sessions()
            ts = []
            for i, batch in enumerate(images):
                model.feed_data(batch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.test()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                want = None if tag == "off" else ("captured" if i == 0 else "replayed")
                assert sde.last_mode == "graph" and sde.last_steps == args.K and sde.last_session == want, (sde.last_mode, sde.last_session)
            if p:  # pass 0 fills the weight and text caches
                first[tag].append(ts[0])
                later[tag].append(statistics.median(ts[1:]))
            if tag == "on" and p:
                m_open = reserved()
                sde.close_sessions()
                held.append(m_open - reserved())
    row = dict(workload=name, H=H, batch=B, num_samples=S, T=args.T, K=args.K, images=args.images, passes=args.passes, sessions=-(-B * S // 16) if S > 1 else 1)
    for tag in ("off", "on"):
        row[f"{tag}_later_ms"] = spread(later[tag])
        row[f"{tag}_first_ms"] = spread(first[tag])
    d = row["off_later_ms"]["median"] - row["on_later_ms"]["median"]
    off_spread = row["off_later_ms"]["max"] - row["off_later_ms"]["min"]
    row["saved_ms_per_image"] = round(d, 2)
    row["off_spread_ms"] = round(off_spread, 2)
    row["inside_off_spread"] = bool(abs(d) <= off_spread)
    row["held_MiB"] = spread([h / 2 ** 20 for h in held])
    log(json.dumps(row))
    del model, sdes
    gc.collect()
    torch.cuda.empty_cache()
    return row


def launch_times(H, R, args, dev):
    from instancediff_amd import ops
    shp = (R, 1, H, H)
    cond_in = torch.randn(shp, generator=torch.Generator().manual_seed(0)).to(dev)
    cond, x, xa = (torch.empty(shp, device=dev) for _ in range(3))
    state = torch.zeros(3, dtype=torch.int32, device=dev)
    tdev = torch.zeros(R, device=dev)

    def replaced():
        z = ops.randn(shp, dev, 1, 0)
        x_T = ops.axpby(cond_in, z, 1.0, 0.4).contiguous().clone()
        ops.axpby(x_T, cond_in, 1.0, -1.0)
        torch.full((R,), 100.0, dtype=torch.float32, device=dev)
        torch.tensor([100, 0, 0], dtype=torch.int32, device=dev)

    def library_only():
        z = ops.randn(shp, dev, 1, 0)
        x_T = ops.axpby(cond_in, z, 1.0, 0.4)
        ops.axpby(x_T, cond_in, 1.0, -1.0)

    fns = {"chain_begin": lambda: ops.chain_begin(cond_in, cond, x, xa, state, tdev, 0.4, 1, offset=0, t0=100),
           "replaced": replaced, "replaced_library_launches_only": library_only}
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(20):
            fn()
    for _ in range(args.rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    row = dict(H=H, rows=R, launches=args.launches, rounds=args.rounds)
    for k, v in res.items():
        row[f"{k}_us"] = spread(v)
    log(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="streams,launch")
    ap.add_argument("--workloads", type=str, default="a,b,c8,c16,d")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reuse_graph needs a GPU"
    dev = torch.device("cuda", 0)
    res = dict(metric="driftSDE reuse_graph: ms per model.test() image, option off vs on, later images and the first; held memory; chain_begin launch",
               device=torch.cuda.get_device_name(0))
    table = dict(a=("224 batch 1", 224, 1, 1), b=("256 batch 16", 256, 16, 1), c8=("224 num_samples 8", 224, 1, 8),
                 c16=("224 num_samples 16", 224, 1, 16), d=("224 num_samples 24 (two chunks)", 224, 1, 24))
    parts = args.parts.split(",")
    if "launch" in parts:
        res["launch"] = [launch_times(224, 1, args, dev), launch_times(256, 16, args, dev)]
    if "streams" in parts:
        res["streams"] = []
        for w in args.workloads.split(","):
            res["streams"].append(stream_times(*table[w], args, dev))
            if args.out:  # keep what is measured so far
                write(args.out, res)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        write(args.out, res)


def write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
