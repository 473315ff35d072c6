"""Radial power spectra (ops.radial_power_spectrum: a direct 2-D DFT in fp64 on the matrix cores, then the radial bins) on the clock.
Prints one JSON line; bench.py is not involved.

  (a) kernel: `ops.radial_power_spectrum` at 256x256 with R = 16 (S + 1) planes for S in {1, 4, 8, 16}, and at 224x224 with R = 9,
      against the torch composition of the same numbers -- `torch.fft.rfft2` of the float64 planes (rocFFT), |X|^2 / (H W) with the
      Hermitian weights, an `index_add_` over the same bin table -- and against `ops.ensemble_distances` on the same tensors in the same
      run.  HIP events around `--launches` back-to-back calls, the candidates alternated over `--rounds` rounds, median with min - max
      of the rounds (the method of scripts/bench_ensemble_distances.py; every time includes the output and workspace allocations of
      its call and all three launches).  `mfma_Tflops` is the arithmetic the matrix cores execute (2 x 16 x 16 x 4 per
      v_mfma_f64_16x16x4_f64: per plane and strip of 16 columns, ceil(H/16) tiles x (2 x W/4 rounded up to 16-column chunks + 4 x H/4)
      instructions) over the whole call's time: a lower bound of the rate the DFT launch reaches.
  (b) calls: wall time of one testUM-shaped step -- `model.test(return_samples=True)` at HxH, `num_samples: S`, `sample_T: K` -- with and
      without `model.power_spectra()` and the host summary: host clock around the call plus a synchronise, the two alternated over
      `--calls` repetitions after one untimed, median and spread.

    python scripts/bench_spectra.py [--T 100 --K 10 --H 224 --S 8 --calls 5 --launches 20 --rounds 5 --parts kernel,calls --out FILE]
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
    print(f"[bench_spectra {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def event_time(fns, launches, rounds):
    """{name: [us per call of each round]}: the candidates alternated round by round, `launches` back-to-back calls per timing"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
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


def torch_spectrum(x, bins, weights, nb):
    """what a caller composes from ATen: float64 [R, nb]"""
    H, W = x.shape[-2:]
    X = torch.fft.rfft2(x.double())
    P = (X.real * X.real + X.imag * X.imag) * (weights / (H * W))
    out = torch.zeros((nb, x.shape[0]), dtype=torch.float64, device=x.device)
    out.index_add_(0, bins, P.flatten(1).t())
    return out.t()


def mfma_flops(R, H, W):
    sv = 16 if H <= 512 else 8
    strips = -(-(W // 2 + 1) // sv)
    tiles = -(-H // 16)
    per_strip = tiles * (2 * 4 * -(-W // 16) + 4 * -(-H // 4))
    return R * strips * per_strip * 2 * 16 * 16 * 4


def kernel_times(args, dev):
    from instancediff_amd import ops
    rows = []
    for H, R, S in [(256, 32, 1), (256, 80, 4), (256, 144, 8), (256, 272, 16), (224, 9, 8)]:
        x = torch.randn(R, H, H, device=dev)
        table, counts, _ = ops.radial_bins(H, H)
        nb = counts.numel()
        bins = table.to(dev).flatten().long()
        v = torch.arange(H // 2 + 1, device=dev)
        weights = torch.where((v == 0) | (2 * v == H), 1.0, 2.0).double()
        fns = {"spectrum": lambda: ops.radial_power_spectrum(x), "torch": lambda: torch_spectrum(x, bins, weights, nb)}
        if H == 256:  # the last merged reducer on the same tensors: B = 16 images of S members and a target
            xs, y = x[:16 * S].view(16, S, 1, H, H), x[16 * S:].view(16, 1, H, H)
            fns["distances"] = lambda: ops.ensemble_distances(xs, y)
        got, want = fns["spectrum"](), fns["torch"]()
        assert torch.allclose(got, want, rtol=1e-9, atol=0), (H, R)
        res = event_time(fns, args.launches, args.rounds)
        row = dict(H=H, R=R, S=S, nb=nb, launches=args.launches, rounds=args.rounds)
        for k, t in res.items():
            row[f"{k}_us"] = round(statistics.median(t), 2)
            row[f"{k}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        row["mfma_Tflops"] = round(mfma_flops(R, H, H) / row["spectrum_us"] * 1e-6, 2)
        row["spectrum_over_torch"] = round(row["spectrum_us"] / row["torch_us"], 2)
        log(json.dumps(row))
        rows.append(row)
    return rows


def call_times(args, dev):
    from instancediff_amd import ops, pipeline
    from instancediff_amd.models.SDEs.driftSDE import spectrum_summary
    from instancediff_amd.utils.synthetic import make_batch
    model, sde = pipeline.build(phase="test", device=dev, T=args.T, seed=0, sde_overrides=dict(sample_T=args.K, num_samples=args.S))
    model.set_eval()
    model.feed_data(make_batch(1, args.H, seed=1))
    counts = ops.radial_bins(args.H, args.H)[1]
    times = {"plain": [], "spectra": []}
    record = None
    for i in range(args.calls + 1):
        for name in ("plain", "spectra"):
            sde.set_seed(100 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.test(return_samples=True)
            if name == "spectra":
                record = spectrum_summary(model.power_spectra(), counts, args.S, L=args.H)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert sde.last_steps == args.K
    row = dict(H=args.H, T=args.T, K=args.K, S=args.S, calls=args.calls,
               last_record={k: record[k] for k in ("HF_RATIO_output", "HF_RATIO_member", "LSD_output", "LSD_member", "SSR_HF")})
    for k, v in times.items():
        v = v[1:]  # the first repetition fills the weight / text caches
        row[f"{k}_ms_median"] = round(statistics.median(v), 3)
        row[f"{k}_ms"] = [round(t, 3) for t in v]
    row["spectra_minus_plain_ms"] = round(row["spectra_ms_median"] - row["plain_ms_median"], 3)
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", type=str, default="kernel,calls")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spectra needs a GPU"
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    res = dict(metric="radial power spectra: radial_power_spectrum vs a float64 torch.fft.rfft2 + index_add_ composition and "
                      "ensemble_distances; a call with and without power_spectra()",
               device=torch.cuda.get_device_name(0))
    if "kernel" in parts:
        res["spectra"] = kernel_times(args, dev)
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
