"""A/B of the opt-in bf16-operand 3x3 convs (model option conv_dtype: bf16, csrc/conv_bf16.hip) against the fp32 path, in ONE process,
the two modes alternated: the c2 sampling step (256^2, batch 16: one captured HIP graph per step, as bench.py times it) and the c3
training iteration (256^2, batch 32).  Prints one JSON line labelled as the REDUCED-PRECISION VARIANT it measures, with per-layer
TFLOP/s of the bf16 kernels (against the 2.5 PFLOP/s dense bf16 peak) and max / mean |dx| of a sampled chain between the two modes
on identical inputs and injected noise.  bench.py's headline line is the fp32 path and never reports this mode.

    python scripts/bench_conv_bf16.py [--size 256 --batch 16 --train-batch 32 --steps 10 --rounds 2]
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

BF16_PEAK_TFLOPS = 2500.0
LABEL = "REDUCED-PRECISION VARIANT: bf16 3x3 conv operands"


def log(msg):
    print(f"[bench_conv_bf16 {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def sampling_runner(kind, args, dev, batch):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, conv_dtype=kind)
    model.set_eval()
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    sde.set_seed(4321)
    x = ops.axpby(cond, sde._randn_like(cond), 1.0, sde.max_sigma)
    st = driftSDE.Stepper(sde, x, cond, batch['names'], model.text_encoder, ctx)
    st.prepare()
    return model, st


def time_steps(st, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    st.run(n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def layer_times(st, kind):
    """one EAGER step with every conv launch timed by events on its stream: {(Cin, Cout, Hout, Wout, mode): [flops, seconds, algos]} of
    the 3x3 convs.  Per-launch events in an eager step include launch gaps the captured graph does not have: use them to compare the
    two modes layer by layer, not as the step's kernel time."""
    from instancediff_amd import ops
    ops.PROFILE = []
    try:
        with ops.conv_operands(kind):
            torch.cuda.synchronize()
            st._body()
            torch.cuda.synchronize()
        recs = ops.PROFILE
    finally:
        ops.PROFILE = None
    agg = {}
    for r in recs:
        if r.get("ks") != 3 or "Cin" not in r:
            continue
        k = (r["Cin"], r["Cout"], r["Hout"], r["Wout"], r["mode"])
        a = agg.setdefault(k, [0.0, 0.0, set()])
        a[0] += r["flops"]
        a[1] += r["e0"].elapsed_time(r["e1"]) * 1e-3
        a[2].add(r["algo"])
    return agg


def layer_ab(runners):
    """per 3x3 level: the fp32 kernel's time (and which kernel) against the bf16 kernel's, same eager methodology"""
    from instancediff_amd import ops
    names = {0: "direct", 1: "F(2x2,3x3)", 3: "F(4x4,3x3)", 4: "F(4x4,3x3) half", 6: "bf16"}
    f32, bf = layer_times(runners["f32"][1], "f32"), layer_times(runners["bf16"][1], "bf16")
    rows, tot = [], {"f32_ms": 0.0, "bf16_ms": 0.0}
    for k in sorted(bf, key=lambda k: -bf[k][0]):
        if ops.CONV_ALGO_BF16 not in bf[k][2] or k not in f32:
            continue
        cin, cout, h, w, mode = k
        fl, sb, _ = bf[k]
        sf = f32[k][1]
        tf = fl / sb / 1e12
        tot["f32_ms"] += sf * 1e3
        tot["bf16_ms"] += sb * 1e3
        rows.append({"layer": f"{cin}->{cout} @{h}x{w}" + (" up2" if mode == ops.CONV_UPSAMPLE2 else ""),
                     "f32_kernel": "/".join(names.get(x, str(x)) for x in sorted(f32[k][2])), "f32_ms": round(sf * 1e3, 3),
                     "bf16_ms": round(sb * 1e3, 3), "bf16_tflops": round(tf, 1), "bf16_of_peak": round(tf / BF16_PEAK_TFLOPS, 3),
                     "bf16_faster": sb < sf})
    return rows, {k: round(v, 3) for k, v in tot.items()}


def chain_delta(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    batch = make_batch(args.chain_batch, args.size, seed=99, mixed=True)
    g = torch.Generator().manual_seed(7)
    x_T = batch['input'] + 0.4 * torch.randn(batch['input'].shape, generator=g)
    noises = torch.randn((args.chain_steps,) + tuple(batch['input'].shape), generator=g)
    outs = []
    for kind in ("f32", "bf16"):
        model, sde = pipeline.build(phase="test", device=dev, T=args.chain_steps, seed=0, conv_dtype=kind)
        model.set_eval()
        model.feed_data(batch)
        model.test(x_T=x_T.to(dev), noises=noises.to(dev))
        outs.append(torch.from_numpy(model.get_visuals()).clone())
        del model, sde
    d = (outs[0] - outs[1]).abs()
    return {"max_abs": float("%.4g" % float(d.max())), "mean_abs": float("%.4g" % float(d.mean())),
            "measured_on": f"{args.chain_steps}-step chain, batch {args.chain_batch}, {args.size}x{args.size}, same weights / inputs / injected noise"}


def train_runner(kind, args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="train", device=dev, T=100, seed=0, conv_dtype=kind)
    model.set_train()
    sde.set_seed(1234)
    batch = make_batch(args.train_batch, args.size, seed=1234, mixed=True)

    def it():
        model.feed_data(batch)
        return model.optimize_parameters()[0]
    return it


def time_iters(it, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = it()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10, help="timed sampling steps per round and mode")
    ap.add_argument("--train-steps", type=int, default=4, help="timed training iterations per round and mode")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="f32 / bf16 alternations")
    ap.add_argument("--chain-steps", type=int, default=50)
    ap.add_argument("--chain-batch", type=int, default=4)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    from instancediff_amd.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    res = {"label": LABEL, "variant": "3x3 conv operands and weights rounded once to bf16 after the fp32 gather, fp32 sums, fp32 epilogue; "
           "every other op as the fp32 path", "metric_sampling": f"ms per denoising step, {args.size}^2, batch {args.batch} (c2 shape)"}

    log("sampling: building both models")
    batch = make_batch(args.batch, args.size, seed=1234, mixed=True)
    runners = {k: sampling_runner(k, args, dev, batch) for k in ("f32", "bf16")}
    for k in ("f32", "bf16"):
        runners[k][1].run(args.warmup)
    ms = {"f32": [], "bf16": []}
    for _ in range(args.rounds):
        for k in ("f32", "bf16"):
            ms[k].append(time_steps(runners[k][1], args.steps))
    res["sampling_ms_per_step"] = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    res["sampling_ms_per_step_all"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
    res["sampling_speedup"] = round(res["sampling_ms_per_step"]["f32"] / res["sampling_ms_per_step"]["bf16"], 3)
    res["sampling_stepper_mode"] = {k: runners[k][1].mode for k in runners}  # 'graph' = the timed steps replayed a captured graph
    log(f"sampling: {res['sampling_ms_per_step']} {res['sampling_stepper_mode']}")
    res["layers_eager_ab"], res["layers_eager_ab_total"] = layer_ab(runners)
    del runners
    torch.cuda.empty_cache()

    if not args.no_train:
        log("training: building both models")
        its = {k: train_runner(k, args, dev) for k in ("f32", "bf16")}
        for k in ("f32", "bf16"):
            for _ in range(2):
                its[k]()
        tms, losses = {"f32": [], "bf16": []}, {}
        for _ in range(args.rounds):
            for k in ("f32", "bf16"):
                t, losses[k] = time_iters(its[k], args.train_steps)
                tms[k].append(t)
        res["metric_training"] = f"ms per training iteration, {args.size}^2, batch {args.train_batch} (c3 shape, one GPU)"
        res["training_ms_per_iter"] = {k: round(statistics.median(v), 2) for k, v in tms.items()}
        res["training_ms_per_iter_all"] = {k: [round(x, 2) for x in v] for k, v in tms.items()}
        res["training_speedup"] = round(res["training_ms_per_iter"]["f32"] / res["training_ms_per_iter"]["bf16"], 3)
        res["training_last_loss"] = {k: round(v, 5) for k, v in losses.items()}
        log(f"training: {res['training_ms_per_iter']}")
        del its
        torch.cuda.empty_cache()

    log("accuracy: chain in both modes")
    res["sampled_x_delta_vs_f32"] = chain_delta(args, dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
