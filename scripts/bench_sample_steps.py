"""Few-step sampling (driftSDE sample_T) on the clock: for K in {T, 50, 20, 10} jumps per chain, the wall time of one
`driftSDE.reverse_ddpm` call (host clock around the call plus a synchronise, median of several calls), the time per step of a long
`Stepper.run` on the same schedule, and the fixed per-call cost = call time - K x step time (the eager warm step and the graph capture
that every call pays, plus the x_T draw and the table uploads).  K = T runs the plain T-step path, the others the schedule path.
Shapes: 224x224 batch 1 (the reference's testUM case) and 256x256 batch 16 (bench.py's), T = 100.  Prints one JSON line; bench.py
is not involved.

    python scripts/bench_sample_steps.py [--T 100 --ks 100,50,20,10 --calls 5 --steps 40 --out FILE]
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
    print(f"[bench_sample_steps {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def measure_shape(H, B, args, dev):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0)
    model.set_eval()
    batch = make_batch(B, H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    rows = []
    for K in args.ks:
        sde.set_sample_steps(sample_T=None if K == args.T else K)
        # wall time of whole calls: the first one fills the weight / text caches and is not counted
        calls = []
        for i in range(args.calls + 1):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e3)
        assert sde.last_steps == K, (sde.last_steps, K)
        mode = sde.last_mode
        calls = calls[1:]
        # per step: one long replay loop on the same schedule (the table advance wraps back to t_0)
        sde.set_seed(7)
        x = ops.axpby(cond, sde._randn_like(cond), 1.0, sde.max_sigma)
        st = driftSDE.Stepper(sde, x, cond, batch['names'], model.text_encoder, ctx,
                              timesteps=None if K == args.T else sde.timesteps)
        st.prepare()
        st.run(3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        st.run(args.steps)
        e1.record()
        torch.cuda.synchronize()
        step_ms = e0.elapsed_time(e1) / args.steps
        call_ms = statistics.median(calls)
        row = dict(H=H, B=B, T=args.T, K=K, path="plain" if K == args.T else "schedule", loop=mode,
                   call_ms_median=round(call_ms, 2), call_ms=[round(c, 2) for c in calls], step_ms=round(step_ms, 3),
                   fixed_ms=round(call_ms - K * step_ms, 2), images_per_s=round(B * 1e3 / call_ms, 3))
        log(json.dumps(row))
        rows.append(row)
    base = rows[0]["call_ms_median"]
    for r in rows:
        r["speedup_vs_first"] = round(base / r["call_ms_median"], 2)
    del model, sde
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--ks", type=str, default="100,50,20,10", help="jumps per chain; the first is the reference for speedup_vs_first")
    ap.add_argument("--shapes", type=str, default="224x1,256x16", help="HxB pairs")
    ap.add_argument("--calls", type=int, default=5, help="timed reverse_ddpm calls per K (after one untimed)")
    ap.add_argument("--steps", type=int, default=40, help="replayed steps of the per-step measurement")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    args.ks = [int(k) for k in args.ks.split(",")]
    assert torch.cuda.is_available(), "bench_sample_steps needs a GPU"
    dev = torch.device("cuda", 0)
    rows = []
    for shape in args.shapes.split(","):
        H, B = (int(v) for v in shape.split("x"))
        log(f"{H}x{H} batch {B}, T={args.T}, K in {args.ks}")
        rows += measure_shape(H, B, args, dev)
    res = dict(metric="driftSDE reverse_ddpm wall time per call vs sample_T", unit="ms", device=torch.cuda.get_device_name(0),
               calls_per_point=args.calls, replay_steps=args.steps,
               note="call_ms: host clock around reverse_ddpm + synchronize, median; step_ms: long Stepper.run on the same schedule; "
                    "fixed_ms = call_ms - K * step_ms (warm step + graph capture + x_T draw + table uploads)",
               rows=rows)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
