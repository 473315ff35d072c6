"""driftSDE solver_order 1 against 2 on the clock and on accuracy.  Prints one JSON line; bench.py is not involved.

  (a) step kernels: per-launch time of `ops.drift_reverse_step_dev` (order 1) and `ops.drift_reverse_step2_dev` (order 2, both rho
      non-zero: every read and write happens) at 224x224 batch 1 and 256x256 batch 16: HIP events around `--launches` back-to-back
      launches, the two kernels alternated over `--rounds` rounds, median of the rounds.
  (b) whole calls: wall time of `driftSDE.reverse_ddpm` at K = `--K` jumps for both orders (host clock around the call plus a
      synchronise, median of `--calls` calls after one untimed, the two orders alternated), measured as
      scripts/bench_sample_steps.py does.
  (c) accuracy at eta = 0, graph replay: max |x - x_ref| and the root mean square of x - x_ref for the K-jump result of each order,
      x_ref = the K = T chain (run at both orders: at T = 100 the order-1 one carries a first-order error of its own), on the analytic
      Gaussian-posterior nets of tests/test_solver_order_gpu.py and on the random-init pipeline nets at 64x64 and 224x224.

    python scripts/bench_solver_order.py [--T 100 --K 10 --calls 5 --launches 200 --rounds 5 --parts kernel,calls,accuracy --out FILE]
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
    print(f"[bench_solver_order {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def kernel_times(H, B, args, dev):
    from instancediff_amd import ops
    n = B * H * H
    g = torch.Generator().manual_seed(0)
    x0, r, e, rp, ep, cond = (torch.randn(n, generator=g).to(dev) for _ in range(6))
    xa = torch.empty(n, device=dev)
    Tp1, t = 8, 5
    tb = torch.zeros(5, Tp1)
    tb[:, t] = torch.tensor([1e-3, 1e-3, 1e-3, 0.5, 0.5])  # small a, b, c: x stays finite over thousands of in-place launches
    coef5 = tb.to(dev).contiguous()
    coef3 = tb[:3].to(dev).contiguous()
    state = torch.tensor([t, 0, 0], dtype=torch.int32, device=dev)
    nper = (n + 3) // 4
    x = x0.clone()

    def k1():
        ops.drift_reverse_step_dev(x, r, e, None, cond, xa, coef3, state, 1, nper, 0)

    def k2():
        ops.drift_reverse_step2_dev(x, r, e, rp, ep, None, cond, xa, coef5, state, 1, nper, 0)
    res = {1: [], 2: []}
    for fn in (k1, k2):
        for _ in range(20):
            fn()
    for _ in range(args.rounds):
        for order, fn in ((1, k1), (2, k2)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[order].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    assert torch.isfinite(x).all()
    row = dict(H=H, B=B, pixels=n, launches=args.launches, rounds=args.rounds, noise="on-device Philox",
               order1_us=round(statistics.median(res[1]), 2), order2_us=round(statistics.median(res[2]), 2),
               order1_us_rounds=[round(v, 2) for v in res[1]], order2_us_rounds=[round(v, 2) for v in res[2]],
               order1_bytes_per_pixel=24, order2_bytes_per_pixel=40)
    log(json.dumps(row))
    return row


def call_times(H, B, args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0)
    model.set_eval()
    batch = make_batch(B, H, seed=1)
    cond = batch['input'].to(dev).contiguous()
    ctx = batch['A_emb'].to(dev).contiguous()
    sde.set_sample_steps(sample_T=args.K)
    calls = {1: [], 2: []}
    for i in range(args.calls + 1):
        for order in (1, 2):
            sde.set_solver_order(order)
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx)
            torch.cuda.synchronize()
            calls[order].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K and sde.last_solver_order == order, (sde.last_steps, sde.last_solver_order)
    mode = sde.last_mode
    row = dict(H=H, B=B, T=args.T, K=args.K, loop=mode)
    for order in (1, 2):
        c = calls[order][1:]  # the first call fills the weight / text caches
        row[f"order{order}_call_ms_median"] = round(statistics.median(c), 2)
        row[f"order{order}_call_ms"] = [round(v, 2) for v in c]
    row["order2_minus_order1_ms"] = round(row["order2_call_ms_median"] - row["order1_call_ms_median"], 2)
    row["order1_spread_ms"] = round(max(calls[1][1:]) - min(calls[1][1:]), 2)
    log(json.dumps(row))
    del model, sde
    torch.cuda.empty_cache()
    return row


def gaussian_device_nets(sde, cond, m, v):
    """posterior means of R ~ N(m, v), eps ~ N(0, 1) given y = x_t - cond = g R + s_t eps, g = -(1 - d_t)"""
    d = sde.drift_schedule
    sg = sde.max_sigma * torch.sqrt(sde.noise_schedule)

    def u_of(y, t):
        ti = t.long()
        g = -(1 - torch.index_select(d, 0, ti).view(-1, 1, 1, 1))
        s = torch.index_select(sg, 0, ti).view(-1, 1, 1, 1)
        return g, s, (y - g * m) / (g * g * v + s * s)

    def drift_net(xa, c, t, *a, **kw):
        g, s, u = u_of(xa, t)
        return m + v * g * u

    def noise_net(xa, x, t, *a, **kw):
        g, s, u = u_of(xa, t)
        return s * u
    return drift_net, noise_net


def accuracy_row(label, sde, run, args, extra):
    res = {}
    for k in (args.K, args.T):
        for order in (1, 2):
            sde.set_sample_steps(sample_T=k)
            sde.set_solver_order(order)
            res[(k, order)] = run().double()
            torch.cuda.synchronize()
            assert sde.last_steps == k and sde.last_solver_order == order
    row = dict(nets=label, T=args.T, K=args.K, eta=0.0, loop=sde.last_mode, **extra)
    for ref_order in (1, 2):
        ref = res[(args.T, ref_order)]
        for order in (1, 2):
            diff = res[(args.K, order)] - ref
            row[f"order{order}_max_vs_full_order{ref_order}"] = float(f"{float(diff.abs().max()):.4e}")
            row[f"order{order}_rms_vs_full_order{ref_order}"] = float(f"{float(diff.pow(2).mean().sqrt()):.4e}")
    row["full_chains_max_diff"] = float(f"{float((res[(args.T, 1)] - res[(args.T, 2)]).abs().max()):.4e}")
    row["finite"] = bool(all(torch.isfinite(v).all() for v in res.values()))
    log(json.dumps(row))
    return row


def accuracy(args, dev):
    from instancediff_amd import pipeline
    from instancediff_amd.models.SDEs.driftSDE import driftSDE
    from instancediff_amd.utils.synthetic import make_batch
    rows = []
    for kind in ("linear", "sigmoid"):
        g = torch.Generator().manual_seed(0)
        cond = (torch.rand(2, 1, 32, 32, generator=g) * 2 - 1).to(dev)
        m = (0.3 * torch.randn(cond.shape, generator=g)).to(dev)
        v = (0.05 + 0.2 * torch.rand(cond.shape, generator=g)).to(dev)
        sde = driftSDE(T=args.T, eta=0.0, drift_schedule=kind, noise_schedule=kind)
        sde.set_gpu(dev)
        sde.drift_net, sde.noise_net = gaussian_device_nets(sde, cond, m, v)
        x_T = cond + sde.max_sigma * torch.randn(cond.shape, generator=g).to(dev)
        rows.append(accuracy_row("analytic Gaussian posterior", sde, lambda: sde.reverse_ddpm(cond, ["x"] * 2, None, x_T=x_T).clone(), args,
                                 dict(H=32, B=2, schedule=kind)))
    for H, B in ((64, 4), (224, 1)):
        model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(eta=0.0))
        model.set_eval()
        batch = make_batch(B, H, seed=1)
        cond = batch['input'].to(dev).contiguous()
        ctx = batch['A_emb'].to(dev).contiguous()
        g = torch.Generator().manual_seed(5)
        x_T = cond + sde.max_sigma * torch.randn(cond.shape, generator=g).to(dev)
        rows.append(accuracy_row("random-init pipeline nets", sde,
                                 lambda: sde.reverse_ddpm(cond, batch['names'], model.text_encoder, image_context=ctx, x_T=x_T).clone(), args,
                                 dict(H=H, B=B, schedule="sigmoid")))
        del model, sde
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, default=10, help="jumps per chain of the call-time and accuracy parts")
    ap.add_argument("--shapes", type=str, default="224x1,256x16", help="HxB pairs of the kernel and call-time parts")
    ap.add_argument("--calls", type=int, default=5, help="timed reverse_ddpm calls per order (after one untimed)")
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per timed round")
    ap.add_argument("--rounds", type=int, default=5, help="alternated rounds per kernel")
    ap.add_argument("--parts", type=str, default="kernel,calls,accuracy")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solver_order needs a GPU"
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    parts = args.parts.split(",")
    res = dict(metric="driftSDE solver_order 1 vs 2: step kernel time, reverse_ddpm call time, distance to the K = T chain",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["step_kernel"] = [kernel_times(H, B, args, dev) for H, B in shapes]
    if "calls" in parts:
        res["calls"] = [call_times(H, B, args, dev) for H, B in shapes]
    if "accuracy" in parts:
        res["accuracy"] = accuracy(args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
