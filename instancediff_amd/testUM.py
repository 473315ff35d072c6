#!/usr/bin/env python3
"""Inference driver with the reference's option surface (testUM.py:43-186):

    python -m instancediff_amd.testUM -opt <yaml>

Reads `test: {iter, pth_dir, use_ema, which_model, which_sde, result_root}` (testUM.py:71-100), restores every
image of the test sets with `model.test()` (timed like :141-144), computes RMSE / PSNR / SSIM per image on the
device (:151-164) and writes the LQ|pred|GT `.raw` triptychs (:170-173).  With `--num-samples S` (driftSDE) each image is restored as
an S-member posterior ensemble: the metrics and the triptych are the mean's, `PSNR_member` / `STD` and a `<i>_std_WxHx1.raw` map are added.
With `--interval L` on top of that the per-pixel median and the level-L credible interval of the members are written as `<i>_median_` / `<i>_lo_` /
`<i>_hi_WxHx1.raw` maps, and `PSNR_median`, `COVER` (the share of ground-truth pixels inside the interval) and `WIDTH` (its mean width) are listed.
With `--scores` on top of `--num-samples S` the ensemble is verified against the ground truth on the device: `CRPS`, `SSR` (spread-skill ratio) and
`RANK_DEV` (the rank histogram's distance from flat) are listed per image, a `<i>_crps_WxHx1.raw` map is written, and per artifact type the
pooled scores are printed and the pooled rank histogram goes to `rank_hist.json`.
With `--distances` on top of `--num-samples S` the members are compared as whole images on the device: the energy score `ES`, its fair form
`ES_FAIR` and the mean pairwise member distance `DIVERSITY` are listed per image with `PSNR_best` (the member nearest to the ground truth) and
`PSNR_medoid` (the most central member), and the medoid is written as `<i>_medoid_WxHx1.raw`.
With `--spectra` (with or without `--num-samples`) the restoration is compared with the ground truth scale by scale on the device: per image
`HF_RATIO` (the restored power above half Nyquist over the truth's: below 1 is over-smoothing) and `LSD` (the log-spectral distance in dB), with
`--num-samples S` also `HF_RATIO_member`, `LSD_member` and `SSR_HF` (the spread-skill ratio of the frequencies above half Nyquist); the radial
power spectra go to `<i>_spectra.json`, the pooled ones per artifact type to `spectra.json` (`spectra_WxH.json` per size if a type's images differ in size).
With `--sparsification [K]` on top of `--num-samples S` the std map is tested as a ranking of the pixels by their error, on the device and without a
sort: per image `AUSE` (the area between the map's sparsification curve and the oracle's: 0 is a perfect ranking), `AURG` (the area gained over
removal in random order: <= 0 is no better than chance) and `AUSE_RMSE` are listed for K points (default 20), per artifact type the pooled values
are printed and the pooled curves (mean squared errors on RMSE's x/2 + 0.5 scale) go to `sparsification.json`.
With `--modes [K]` on top of `--num-samples S` the members' joint variation is decomposed into principal modes on the device: per image `EFF_MODES`
(the participation ratio of the spectrum: how many degrees of freedom the ensemble has), `EXPLAINED_1` (the leading mode's share of the variance),
`SPAN_SHARE` (the share of the mean's squared error inside the members' span) and `MODE_Z_RMS` (error over spread along the modes: above 1 is
under-dispersed) are listed, the K leading unit-norm mode images (default 4) go to `<i>_modes_WxHxK.raw`, the pooled values per artifact type to `modes.json`.
With `--tile P [P]` / `--tile-overlap O` (driftSDE) an image larger than the window is restored as a batch of overlapping windows of one
full-resolution chain; `--tiled-ensemble` lets that meet `--num-samples` (an ensemble of tiled chains).  With `--reuse-graph` (driftSDE) the captured step graph is kept and replayed for every later image of the same shape.
With `--self-ensemble {flips,dihedral}` on top of `--num-samples S` (driftSDE) the members also differ in orientation: each runs on a flipped /
transposed copy of the image and is turned back before the mean, the maps and the scores (a geometric self-ensemble).
With `--random-init` the checkpoint load
is skipped (synthetic smoke runs).
With `--regions SPEC` the scores are also taken per region of a label map, on the device, with or without `--num-samples` (S = 1 scores the
restoration itself): `bands:e1,e2,...` labels every pixel by the intensity band of its ground truth (edges on the x/2 + 0.5 scale),
`grid:GYxGX` by the cell of a GY x GX grid, `file` by the raw uint8 map the dataset item's optional `"label"` key names (`--regions-L L`
regions; any label >= L, 255 by convention, is outside).  Per image `RMSE_r`, `CRPS_r` (the MAE at S = 1), `BIAS_r` (x/2 + 0.5 scale) and
`SSR_r` are listed region by region; the pooled record per artifact type goes to `regions.json`.
With `--speckle [SPEC]` (the `--regions` grammar, default `grid:8x8`; `--speckle-L L` with `file`, `--speckle-background l` for the CNR) the
restoration is judged without a ground truth, on the device and on the x/2 + 0.5 scale, from the restored image and the noisy input alone:
per image `ENL` (the equivalent number of looks, the mean over the regions), `ENL_AUTO` (over the quarter of the regions in which the input
is most homogeneous), `SSI`, `MEAN_RATIO` / `VAR_RATIO` of the ratio image input / restored, and the edge-preservation index against the input
(`EPI_in`) and the ground truth (`EPI_gt`); with `--num-samples S` also `ENL_member` / `LAP_RATIO_member` beside the mean image's `ENL` /
`LAP_RATIO` (how much smoother the mean is than a draw); the means over a type's images go to `speckle.json`.  Sampling shards by image across ranks when launched with torchrun.
"""
import argparse
import json
import math
import os
import time
from collections import OrderedDict

import torch
import yaml

from . import ops, parallel
from .data import create_dataset, dump_raw, iterate_batches
from .models import create_model
from .models.SDEs import create_sde
from .models.SDEs.driftSDE import (despeckle_summary, ensemble_distance_summary, ensemble_mode_summary, ensemble_score_summary,
                                   homogeneous_cells, region_score_summary, sparsification_summary, spectrum_summary)


def pool_spectra(entries, S):
    """entries: (H, W, spectra dict of host tensors) per image -> {(H, W): spectrum_summary of the images of that size pooled}.  Bins of
    different image sizes are different frequencies, so a type whose images differ in size gets a record per size."""
    out = {}
    for Hs, Ws in sorted({(h, w) for h, w, _ in entries}):
        group = [sp for h, w, sp in entries if (h, w) == (Hs, Ws)]
        out[(Hs, Ws)] = spectrum_summary({key: torch.cat([sp[key] for sp in group]) for key in group[0]}, ops.radial_bins(Hs, Ws)[1], S,
                                         L=max(Hs, Ws))
    return out


def yaml_num_samples(args, opt):
    """num_samples as the sde will get it: --num-samples, else the YAML's; known before the model is built"""
    return args.num_samples if args.num_samples is not None else opt['sdes'][opt['test']['which_sde']].get('num_samples')


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-opt", type=str, required=True, help="Path to options YAML file.")
    parser.add_argument("--random-init", action="store_true", help="skip model.load (no checkpoint; synthetic smoke run)")
    parser.add_argument("--limit", type=int, default=0, help="stop after N images")
    parser.add_argument("--sample-T", type=int, default=None, metavar="K",
                        help="reverse-chain steps per image (driftSDE sample_T: K uniform jumps over the T-step schedule)")
    parser.add_argument("--solver-order", type=int, default=None, metavar="N", choices=(1, 2),
                        help="driftSDE solver_order: 1 = first-order jumps, 2 = second-order multistep jumps (overrides the YAML)")
    parser.add_argument("--num-samples", type=int, default=None, metavar="S",
                        help="driftSDE num_samples: S posterior samples per image as one batched chain; the mean is the restored image, "
                             "the per-pixel standard deviation is written next to it (overrides the YAML)")
    parser.add_argument("--max-batch", type=int, default=None, metavar="M",
                        help="driftSDE max_batch: rows per chain of an ensemble (overrides the YAML)")
    parser.add_argument("--interval", type=float, default=None, metavar="L",
                        help="driftSDE interval: credible level L in (0, 1) of the per-pixel interval and median maps of an ensemble, written "
                             "next to the std map with PSNR_median / COVER / WIDTH (needs num_samples > 1; overrides the YAML)")
    parser.add_argument("--scores", action="store_true",
                        help="ensemble scores against the ground truth (needs num_samples > 1): CRPS / SSR / RANK_DEV per image and a CRPS "
                             "map, the pooled scores and rank_hist.json per artifact type")
    parser.add_argument("--distances", action="store_true",
                        help="image-level member distances (needs num_samples > 1): the energy score ES / ES_FAIR, DIVERSITY, PSNR_best and "
                             "PSNR_medoid per image and the medoid member as a map, the averages per artifact type")
    parser.add_argument("--spectra", action="store_true",
                        help="radial power spectra of the restoration, the ground truth and their difference (of the members too with "
                             "num_samples > 1): HF_RATIO and LSD per image, <i>_spectra.json, the pooled spectra in spectra.json per artifact type")
    parser.add_argument("--tile", type=int, nargs="+", default=None, metavar="P",
                        help="driftSDE tile: window size P, or Ph Pw, of tiled sampling for images larger than the window (overrides the YAML)")
    parser.add_argument("--tile-overlap", type=int, default=None, metavar="O",
                        help="driftSDE tile_overlap: pixels shared by adjacent windows (default tile // 8; overrides the YAML)")
    parser.add_argument("--tiled-ensemble", action="store_true",
                        help="driftSDE tiled_ensemble: let --num-samples and --tile meet: an image larger than the window is restored as an "
                             "ensemble of tiled chains (without it the two options refuse each other; overrides the YAML)")
    parser.add_argument("--max-chain-rows", type=int, default=None, metavar="N",
                        help="driftSDE max_chain_rows: window rows per chain of a tiled ensemble (default 128; overrides the YAML)")
    parser.add_argument("--reuse-graph", action="store_true",
                        help="driftSDE reuse_graph: keep the captured step graph and replay it for every later image of the same shape "
                             "(same bits; overrides the YAML)")
    parser.add_argument("--self-ensemble", type=str, default=None, choices=("flips", "dihedral"),
                        help="driftSDE self_ensemble: member s of an ensemble runs on the image flipped (flips: any H x W) or flipped / "
                             "transposed (dihedral: square images) and is turned back before the reduction (needs num_samples > 1; "
                             "overrides the YAML)")
    # absent from the namespace without the flag (argparse.SUPPRESS): tests/test_spectrum_cpu.py compares the whole namespace of a run
    # without it against a literal dict
    parser.add_argument("--sparsification", type=int, nargs="?", const=20, default=argparse.SUPPRESS, metavar="K",
                        help="sparsification curves of the std map over K points, default 20 (needs num_samples > 1): AUSE / AURG / AUSE_RMSE "
                             "per image, the pooled values and sparsification.json per artifact type; an image whose C*H*W is not a "
                             "multiple of 4 is left out of the curves, with a note on its line")
    # absent from the namespace without the flag, like --sparsification
    parser.add_argument("--modes", type=int, nargs="?", const=4, default=argparse.SUPPRESS, metavar="K",
                        help="principal modes of the ensemble, the K leading ones as images, default 4 (needs num_samples > 1): EFF_MODES / "
                             "EXPLAINED_1 / SPAN_SHARE / MODE_Z_RMS per image, the pooled values and modes.json per artifact type; an image "
                             "whose C*H*W is not a multiple of 4 is left out, with a note on its line")
    # absent from the namespace without the flags, like --sparsification
    parser.add_argument("--regions", type=str, default=argparse.SUPPRESS, metavar="SPEC",
                        help="per-region scores over a label map, with or without num_samples (S = 1 scores the restoration itself): "
                             "bands:e1,e2,... (intensity bands of the ground truth, edges on the x/2 + 0.5 scale), grid:GYxGX (a grid of "
                             "GY x GX cells, at most 64) or file (the raw uint8 map named by the dataset item's \"label\" key, with "
                             "--regions-L); RMSE_r / CRPS_r / BIAS_r / SSR_r per image and regions.json per artifact type")
    parser.add_argument("--regions-L", type=int, default=argparse.SUPPRESS, metavar="L", dest="regions_L",
                        help="the number of regions of --regions file: labels 0 .. L-1 count, any other label (255 by convention) is outside")
    parser.add_argument("--speckle", type=str, nargs="?", const="grid:8x8", default=argparse.SUPPRESS, metavar="SPEC",
                        help="no-reference despeckling statistics per region of a label map (the --regions grammar, default grid:8x8), with or "
                             "without num_samples: ENL / ENL_AUTO / SSI / MEAN_RATIO / VAR_RATIO / EPI_in / EPI_gt per image (with num_samples "
                             "also ENL_member / LAP_RATIO_member) and speckle.json per artifact type; an image whose width is not a multiple "
                             "of 4 is left out, with a note on its line")
    parser.add_argument("--speckle-L", type=int, default=argparse.SUPPRESS, metavar="L", dest="speckle_L",
                        help="the number of regions of --speckle file")
    parser.add_argument("--speckle-background", type=int, default=argparse.SUPPRESS, metavar="l", dest="speckle_background",
                        help="the background region of the contrast-to-noise ratio (default 0)")
    return parser


MODES_MAX_K = 64  # the members of the largest ensemble the kernels take


def parse_regions(spec, regions_L=None):
    """--regions SPEC (and --regions-L) -> dict(kind, L, names, spec and, by kind, edges: the band edges on the tensors' [-1, 1] scale
    as float32 values | gy, gx).  Raises ValueError with the message parser.error prints."""
    kind, _, rest = str(spec).partition(":")
    if kind != "file" and regions_L is not None:
        raise ValueError("--regions-L goes with --regions file: bands and grids know their number of regions")
    if kind == "bands":
        try:
            shown = [float(t) for t in rest.split(",")]
        except ValueError:
            raise ValueError(f"--regions bands: takes comma-separated numbers, got {rest!r}") from None
        if not 1 <= len(shown) <= ops.BAND_MAX_EDGES:
            raise ValueError(f"--regions bands: takes 1 to {ops.BAND_MAX_EDGES} edges, got {len(shown)}")
        if not all(math.isfinite(e) for e in shown):
            raise ValueError("--regions bands: the edges must be finite")
        edges = torch.tensor([2.0 * e - 1.0 for e in shown], dtype=torch.float64).to(torch.float32).tolist()  # x/2 + 0.5 -> [-1, 1]
        if any(b <= a for a, b in zip(edges, edges[1:])):
            raise ValueError("--regions bands: the edges must be strictly ascending")
        names = [f"<{shown[0]:g}"] + [f"{a:g}..{b:g}" for a, b in zip(shown, shown[1:])] + [f">={shown[-1]:g}"]
        return dict(kind="bands", spec=str(spec), L=len(edges) + 1, names=names, edges=edges)
    if kind == "grid":
        parts = rest.lower().split("x")
        if len(parts) != 2 or not all(p.isdigit() for p in parts):
            raise ValueError(f"--regions grid: takes GYxGX, got {rest!r}")
        gy, gx = int(parts[0]), int(parts[1])
        if gy < 1 or gx < 1 or gy * gx > ops.REGION_MAX_L:
            raise ValueError(f"--regions grid: GY and GX must be >= 1 with GY*GX <= {ops.REGION_MAX_L}, got {gy}x{gx}")
        return dict(kind="grid", spec=str(spec), L=gy * gx, names=[f"r{y}c{x}" for y in range(gy) for x in range(gx)], gy=gy, gx=gx)
    if kind == "file" and not rest:
        if isinstance(regions_L, bool) or not isinstance(regions_L, int) or not 1 <= regions_L <= ops.REGION_MAX_L:
            raise ValueError(f"--regions file: needs --regions-L L with L in [1, {ops.REGION_MAX_L}]")
        return dict(kind="file", spec=str(spec), L=regions_L, names=[str(l) for l in range(regions_L)])
    raise ValueError(f"--regions takes bands:e1,e2,..., grid:GYxGX or file, got {spec!r}")


def region_labels(regions, model, item):
    """the uint8 label map of one image for model.region_scores, by the kind of --regions"""
    if regions["kind"] == "bands":
        return ops.band_labels(model.target, regions["edges"])
    if regions["kind"] == "grid":
        H, W = (int(n) for n in model.target.shape[-2:])
        return ops.grid_labels(H, W, regions["gy"], regions["gx"], str(model.target.device))
    if "LABEL" not in item:
        raise ValueError(f"--regions file: the dataset item of {item['GT_path']} has no \"label\" key")
    return item["LABEL"]


def _scaled(v, scale):
    return None if v is None else scale * v


def parse_speckle(spec, speckle_L=None, background=None):
    """--speckle SPEC (and --speckle-L, --speckle-background) -> parse_regions' dict plus background.  Raises ValueError with the message
    parser.error prints."""
    try:
        speckle = parse_regions(spec, speckle_L)
    except ValueError as e:
        raise ValueError(str(e).replace("--regions", "--speckle")) from None
    background = 0 if background is None else background
    if isinstance(background, bool) or not isinstance(background, int) or not 0 <= background < speckle["L"]:
        raise ValueError(f"--speckle-background takes a region index in [0, {speckle['L']}), got {background!r}")
    speckle["background"] = background
    return speckle


def _region_mean(rows, metric):
    """the mean of a metric over every row and region of a despeckle_summary where it is defined, else None"""
    have = [q[metric] for row in rows for q in row if q[metric] is not None]
    return math.fsum(have) / len(have) if have else None


def speckle_record(recs, speckle):
    """the speckle.json record of a type: recs = per image dict(input, target[, members]) of ops.despeckle_stats' host tensors"""
    out = dict(spec=speckle["spec"], L=speckle["L"], names=speckle["names"], background=speckle["background"], images=len(recs))
    for key in ("input", "target", "members"):
        if not all(key in rec for rec in recs):
            continue
        one = despeckle_summary(*(torch.cat([rec[key][q] for rec in recs]) for q in range(3)), speckle["names"], speckle["background"])
        auto = [a for a in homogeneous_cells(*(torch.cat([rec[key][q] for rec in recs]) for q in range(2)))["ENL_AUTO"] if a is not None]
        out[key] = dict(regions=one["regions"], outside=one["outside"], ENL_AUTO=math.fsum(auto) / len(auto) if auto else None,
                        **{m: _region_mean(one["rows"], m) for m in ("ENL", "SSI", "MEAN_RATIO", "VAR_RATIO", "EPI", "LAP_RATIO")})
    return out


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.tile is not None and len(args.tile) > 2:
        parser.error("--tile takes one size P or two, Ph Pw")
    with open(args.opt, "r") as f:
        opt = yaml.load(f.read(), yaml.FullLoader)  # raw dict: missing keys raise, as in the reference (:50-54)
    if args.self_ensemble is not None:  # refused before the model is built: the option only turns the members of an ensemble
        num = yaml_num_samples(args, opt)
        if not isinstance(num, int) or num <= 1:
            parser.error("--self-ensemble turns the members of an ensemble: it needs num_samples > 1 (--num-samples S or the YAML's num_samples)")
    K_sp = getattr(args, "sparsification", None)
    if K_sp is not None:  # refused before the model is built, like --self-ensemble
        if not 1 <= K_sp <= ops.SPARSIFICATION_MAX_K:
            parser.error(f"--sparsification takes K in [1, {ops.SPARSIFICATION_MAX_K}]")
        num = yaml_num_samples(args, opt)
        if not isinstance(num, int) or num <= 1:
            parser.error("--sparsification ranks the pixels by an ensemble's spread: it needs num_samples > 1 (--num-samples S or the YAML's "
                         "num_samples)")
    K_modes = getattr(args, "modes", None)
    if K_modes is not None:  # refused before the model is built, like --sparsification
        if not 1 <= K_modes <= MODES_MAX_K:
            parser.error(f"--modes takes K in [1, {MODES_MAX_K}]")
        num = yaml_num_samples(args, opt)
        if not isinstance(num, int) or num <= 1:
            parser.error("--modes decomposes the spread of an ensemble: it needs num_samples > 1 (--num-samples S or the YAML's num_samples)")
    regions = None
    if hasattr(args, "regions") or hasattr(args, "regions_L"):  # refused before the model is built, like --sparsification
        if not hasattr(args, "regions"):
            parser.error("--regions-L goes with --regions file")
        try:
            regions = parse_regions(args.regions, getattr(args, "regions_L", None))
        except ValueError as e:
            parser.error(str(e))
    speckle = None
    if any(hasattr(args, a) for a in ("speckle", "speckle_L", "speckle_background")):  # refused before the model is built, like --regions
        if not hasattr(args, "speckle"):
            parser.error("--speckle-L and --speckle-background go with --speckle")
        try:
            speckle = parse_speckle(args.speckle, getattr(args, "speckle_L", None), getattr(args, "speckle_background", None))
        except ValueError as e:
            parser.error(str(e))
    rank, world, local = parallel.init_distributed()
    if torch.cuda.is_available():
        torch.cuda.set_device(local if world > 1 else opt['gpu_ids'][0])
    train_opt, test_opt = dict(opt['train']), opt['test']
    train_opt['dist'] = False
    model = create_model(train_opt, opt['models'][test_opt['which_model']], phase='test')
    if not args.random_init:
        model.load(test_opt['iter'], test_opt['pth_dir'])
    sde_opt = dict(opt['sdes'][test_opt['which_sde']])
    if args.sample_T is not None:
        sde_opt.pop('sample_timesteps', None)
        sde_opt['sample_T'] = args.sample_T
    if args.solver_order is not None:
        sde_opt['solver_order'] = args.solver_order
    if args.num_samples is not None:
        sde_opt['num_samples'] = args.num_samples
    if args.max_batch is not None:
        sde_opt['max_batch'] = args.max_batch
    if args.interval is not None:
        sde_opt['interval'] = args.interval
    if args.tile is not None:
        sde_opt['tile'] = args.tile[0] if len(args.tile) == 1 else list(args.tile)
    if args.tile_overlap is not None:
        sde_opt['tile_overlap'] = args.tile_overlap
    if args.tiled_ensemble:
        sde_opt['tiled_ensemble'] = True
    if args.max_chain_rows is not None:
        sde_opt['max_chain_rows'] = args.max_chain_rows
    if args.reuse_graph:
        sde_opt['reuse_graph'] = True
    if args.self_ensemble is not None:
        sde_opt['self_ensemble'] = args.self_ensemble
    sde = create_sde(model.get_nets(use_ema=test_opt['use_ema']), sde_opt)
    sde.set_gpu(model.device)
    model.set_sde(sde)
    model.set_eval()
    S = getattr(sde, 'num_samples', 1)
    if args.scores and S <= 1:
        parser.error("--scores verifies an ensemble: it needs num_samples > 1 (--num-samples S or the YAML's num_samples)")
    if args.distances and S <= 1:
        parser.error("--distances compares the members of an ensemble: it needs num_samples > 1 (--num-samples S or the YAML's num_samples)")
    kind = getattr(sde, 'self_ensemble', None) if S > 1 else None
    result_root = os.path.join(test_opt['result_root'], opt['name'])
    results = OrderedDict((a, {'num': 0, 'RMSE': [], 'SSIM': [], 'PSNR': []}) for a in opt['artifact_type'])
    if S > 1:
        for r in results.values():
            r['PSNR_member'], r['STD'] = [], []
    level = getattr(sde, 'interval', None) if S > 1 else None  # the interval maps are an ensemble's: the plain chain has none
    if level is not None:
        for r in results.values():
            r['PSNR_median'], r['COVER'], r['WIDTH'] = [], [], []
    if args.scores:
        for r in results.values():
            r['CRPS'], r['SSR'], r['RANK_DEV'], r['scores'] = [], [], [], []
    if args.distances:
        for r in results.values():
            r['ES'], r['ES_FAIR'], r['DIVERSITY'], r['PSNR_best'], r['PSNR_medoid'] = [], [], [], [], []
    if args.spectra:
        for r in results.values():
            r['HF_RATIO'], r['LSD'], r['spectra'] = [], [], []
            if S > 1:
                r['HF_RATIO_member'], r['LSD_member'], r['SSR_HF'] = [], [], []
    if K_sp is not None:
        for r in results.values():
            r['AUSE'], r['AURG'], r['AUSE_RMSE'], r['sparsification'] = [], [], [], []
    if K_modes is not None:
        for r in results.values():
            r['EFF_MODES'], r['EXPLAINED_1'], r['SPAN_SHARE'], r['MODE_Z_RMS'], r['modes'] = [], [], [], [], []
    if regions is not None:
        for r in results.values():
            r['regions'] = []
    if speckle is not None:
        for r in results.values():
            r['speckle'] = []
    times = []
    n_done = n_replayed = 0
    for phase, dataset_opt in sorted(opt["datasets"].items()):
        if args.limit and n_done >= args.limit:
            break
        dataset_opt = dict(dataset_opt)
        dataset_opt.setdefault("phase", phase.split("_")[0])
        test_set = create_dataset(dataset_opt)
        ids = parallel.shard_indices(len(test_set), rank, world)
        print("Testing [{:s}]: {:d} images ({:d} on this rank)".format(dataset_opt["name"], len(test_set), len(ids)))
        with torch.no_grad():
            for i in ids:
                it = test_set[i]
                if it["name"] not in opt['artifact_type']:
                    continue
                data = {'input': it["LQ"][None], 'target': it["GT"][None], 'names': [it["name"]], 'A_emb': it["A_emb"][None]}
                model.feed_data(data)
                torch.cuda.synchronize()
                tic = time.time()
                model.test(**({'return_samples': True} if S > 1 else {}))
                times.append(time.time() - tic)
                n_replayed += getattr(sde, 'last_session', None) == 'replayed'
                rmse, psnr, ssim = ops.image_metrics(model.output[:, 0], model.target[:, 0]).cpu().tolist()[0]
                r = results[it["name"]]
                r['RMSE'].append(rmse), r['SSIM'].append(ssim), r['PSNR'].append(psnr)
                r['num'] += 1
                shape = dump_raw(os.path.join(result_root, it["name"], f"{i}.raw"), it["LQ"].numpy(), model.get_visuals(), it["GT"].numpy())
                os.replace(os.path.join(result_root, it["name"], f"{i}.raw"),
                           os.path.join(result_root, it["name"], f"{i}_{shape[-1]}x{shape[-2]}x1.raw"))
                extra = ""
                if S > 1:  # the listed metrics are the mean's; the members' own PSNR and the spread go beside them
                    member = ops.image_metrics(model.samples[0, :, 0], model.target[:, 0].expand(S, -1, -1).contiguous()).cpu()
                    r['PSNR_member'].append(float(member[:, 1].mean()))
                    std_map = model.output_std[0, 0].cpu()
                    r['STD'].append(float(std_map.mean()))
                    std_map.numpy().tofile(os.path.join(result_root, it["name"], f"{i}_std_{std_map.shape[-1]}x{std_map.shape[-2]}x1.raw"))
                    extra = f", PSNR_member={r['PSNR_member'][-1]}, STD={r['STD'][-1]}"
                if level is not None:
                    lo, hi, med = model.output_lo, model.output_hi, model.output_median
                    npix = lo[0].numel()
                    r['PSNR_median'].append(ops.image_metrics(med[:, 0], model.target[:, 0]).cpu().tolist()[0][1])
                    r['COVER'].append(ops.interval_coverage(lo, hi, model.target).cpu().tolist()[0][1] / npix)
                    r['WIDTH'].append(float(ops.plane_sum(ops.axpby(hi, lo, 1.0, -1.0)).cpu()[0, 0]) / npix)
                    for tag, m in (("lo", lo), ("hi", hi), ("median", med)):
                        m = m[0, 0].cpu()
                        m.numpy().tofile(os.path.join(result_root, it["name"], f"{i}_{tag}_{m.shape[-1]}x{m.shape[-2]}x1.raw"))
                    extra += f", PSNR_median={r['PSNR_median'][-1]}, COVER={r['COVER'][-1]}, WIDTH={r['WIDTH'][-1]}"
                if args.scores:  # CRPS and the spreads on RMSE's x/2 + 0.5 scale: half of what the [-1, 1] tensors give
                    sums, counts, crps_map = model.score_ensemble(want_map=True)
                    sums, counts = sums.cpu(), counts.cpu()
                    one = ensemble_score_summary(sums, counts, S)
                    r['scores'].append((sums, counts))
                    r['CRPS'].append(0.5 * one['CRPS']), r['SSR'].append(one['SSR']), r['RANK_DEV'].append(one['RANK_DEV'])
                    m = crps_map[0, 0].cpu() * 0.5
                    m.numpy().tofile(os.path.join(result_root, it["name"], f"{i}_crps_{m.shape[-1]}x{m.shape[-2]}x1.raw"))
                    extra += f", CRPS={r['CRPS'][-1]}, SSR={r['SSR'][-1]}, RANK_DEV={r['RANK_DEV'][-1]}"
                if args.distances:  # the distances on RMSE's x/2 + 0.5 scale, like the CRPS; the PSNRs from the picked members themselves
                    d2, dcounts, _ = model.member_distances()
                    one = ensemble_distance_summary(d2, dcounts, S, True)
                    medoid, best = model.pick_member("medoid"), model.pick_member("best")
                    for tag in ('ES', 'ES_FAIR', 'DIVERSITY'):
                        r[tag].append(0.5 * one[tag][0])
                    r['PSNR_best'].append(ops.image_metrics(best[:, 0], model.target[:, 0]).cpu().tolist()[0][1])
                    r['PSNR_medoid'].append(ops.image_metrics(medoid[:, 0], model.target[:, 0]).cpu().tolist()[0][1])
                    m = medoid[0, 0].cpu()
                    m.numpy().tofile(os.path.join(result_root, it["name"], f"{i}_medoid_{m.shape[-1]}x{m.shape[-2]}x1.raw"))
                    extra += (f", ES={r['ES'][-1]}, ES_FAIR={r['ES_FAIR'][-1]}, DIVERSITY={r['DIVERSITY'][-1]}, PSNR_best={r['PSNR_best'][-1]}, "
                              f"PSNR_medoid={r['PSNR_medoid'][-1]}")
                if args.spectra:  # the power of the [-1, 1] tensors times 0.25: RMSE's x/2 + 0.5 scale but for bin 0, which no ratio uses
                    spectra = {key: 0.25 * v.cpu() for key, v in model.power_spectra().items()}
                    Hs, Ws = model.output.shape[-2:]
                    _, bin_counts, freq = ops.radial_bins(int(Hs), int(Ws))
                    one = spectrum_summary(spectra, bin_counts, S, L=max(int(Hs), int(Ws)))
                    r['spectra'].append((int(Hs), int(Ws), spectra))
                    r['HF_RATIO'].append(one['HF_RATIO_output']), r['LSD'].append(one['LSD_output'])
                    extra += f", HF_RATIO={r['HF_RATIO'][-1]}, LSD={r['LSD'][-1]}"
                    if S > 1:
                        r['HF_RATIO_member'].append(one['HF_RATIO_member']), r['LSD_member'].append(one['LSD_member'])
                        r['SSR_HF'].append(one['SSR_HF'])
                        extra += f", HF_RATIO_member={r['HF_RATIO_member'][-1]}, LSD_member={r['LSD_member'][-1]}, SSR_HF={r['SSR_HF'][-1]}"
                    with open(os.path.join(result_root, it["name"], f"{i}_spectra.json"), "w") as f:
                        json.dump(dict(S=S, freq=freq.tolist(), counts=bin_counts.tolist(),
                                       **{key: v for key, v in one.items() if key.startswith("PSD_")}), f)
                if K_sp is not None and model.output[0].numel() % 4:  # the kernel reads 16-byte pieces
                    extra += ", AUSE=left out (C*H*W is not a multiple of 4)"
                elif K_sp is not None:  # ratios of normalised curves: no scale to carry
                    rec = [t.cpu() for t in model.sparsification(K=K_sp, key="std")[:4]]
                    one = sparsification_summary(*rec, K_sp)
                    r['sparsification'].append(rec)
                    r['AUSE'].append(one['AUSE']), r['AURG'].append(one['AURG']), r['AUSE_RMSE'].append(one['AUSE_RMSE'])
                    extra += f", AUSE={r['AUSE'][-1]}, AURG={r['AURG'][-1]}, AUSE_RMSE={r['AUSE_RMSE'][-1]}"
                if K_modes is not None and model.output[0].numel() % 4:  # the kernels read 16-byte pieces
                    extra += ", EFF_MODES=left out (C*H*W is not a multiple of 4)"
                elif K_modes is not None:  # ratios and unit-norm images: no scale to carry
                    rec = model.principal_modes(K=K_modes)
                    host = [rec[q].cpu() for q in ('lam', 'tcoord', 'tnorm2', 'info', 'counts')]
                    one = ensemble_mode_summary(*host, S, True)
                    r['modes'].append(host)
                    r['EFF_MODES'].append(one['EFF_MODES'][0]), r['EXPLAINED_1'].append(one['EXPLAINED'][0][0])
                    r['SPAN_SHARE'].append(one['SPAN_SHARE'][0]), r['MODE_Z_RMS'].append(one['MODE_Z_RMS'][0])
                    m = rec['modes'][0, :, 0].cpu()
                    m.numpy().tofile(os.path.join(result_root, it["name"], f"{i}_modes_{m.shape[-1]}x{m.shape[-2]}x{m.shape[0]}.raw"))
                    extra += (f", EFF_MODES={r['EFF_MODES'][-1]}, EXPLAINED_1={r['EXPLAINED_1'][-1]}, SPAN_SHARE={r['SPAN_SHARE'][-1]}, "
                              f"MODE_Z_RMS={r['MODE_Z_RMS'][-1]}")
                if regions is not None and model.output[0].numel() % 4:  # the kernel reads 16-byte pieces
                    extra += ", RMSE_r=left out (C*H*W is not a multiple of 4)"
                elif regions is not None:  # errors on RMSE's x/2 + 0.5 scale: half of what the [-1, 1] tensors give; SSR is a ratio
                    rec = [t.cpu() for t in model.region_scores(region_labels(regions, model, it), regions["L"],
                                                                what="ensemble" if S > 1 else "output")]
                    one = region_score_summary(*rec, S, regions["names"])["regions"]
                    r['regions'].append(rec)
                    extra += (f", RMSE_r={[_scaled(q['RMSE'], 0.5) for q in one]}, CRPS_r={[_scaled(q['CRPS'], 0.5) for q in one]}, "
                              f"BIAS_r={[_scaled(q['BIAS'], 0.5) for q in one]}, SSR_r={[q['SSR'] for q in one]}")
                if speckle is not None and model.output.shape[-1] % 4:  # the kernel reads aligned 16-byte pieces of an image line
                    extra += ", ENL=left out (W is not a multiple of 4)"
                elif speckle is not None:  # a = x/2 + 0.5 inside the kernel: RMSE's scale, on which speckle is multiplicative
                    labels = region_labels(speckle, model, it)
                    rec = {key: [t.cpu() for t in model.despeckle_stats(labels, speckle["L"], what="output", against=key)]
                           for key in ("input", "target")}
                    if S > 1:
                        rec["members"] = [t.cpu() for t in model.despeckle_stats(labels, speckle["L"], what="ensemble", against="input")]
                    r['speckle'].append(rec)
                    one = speckle_record([rec], speckle)
                    extra += (f", ENL={one['input']['ENL']}, ENL_AUTO={one['input']['ENL_AUTO']}, SSI={one['input']['SSI']}, "
                              f"MEAN_RATIO={one['input']['MEAN_RATIO']}, VAR_RATIO={one['input']['VAR_RATIO']}, EPI_in={one['input']['EPI']}, "
                              f"EPI_gt={one['target']['EPI']}")
                    if S > 1:
                        extra += (f", ENL_member={one['members']['ENL']}, LAP_RATIO={one['input']['LAP_RATIO']}, "
                                  f"LAP_RATIO_member={one['members']['LAP_RATIO']}")
                print(f' Testing {i}, {it["GT_path"]}: RMSE={rmse}, SSIM={ssim}, PSNR={psnr}' + extra)
                n_done += 1
                if args.limit and n_done >= args.limit:
                    break
    for k, v in results.items():
        if v['num']:
            print(k + "".join(f", AVG {m}: {sum(v[m]) / v['num']}" for m in ('RMSE', 'SSIM', 'PSNR') + (('PSNR_member', 'STD') if S > 1 else ())
                                  + (('PSNR_median', 'COVER', 'WIDTH') if level is not None else ()) + (('CRPS',) if args.scores else ())
                                  + (('ES', 'ES_FAIR', 'DIVERSITY', 'PSNR_best', 'PSNR_medoid') if args.distances else ())))
            if args.scores:  # the type's record: sums and histograms pooled over its images, not the mean of the per-image ratios
                pooled = ensemble_score_summary(torch.cat([s for s, _ in v['scores']]), torch.cat([c for _, c in v['scores']]), S)
                v['pooled'] = pooled
                print(f"{k}, pooled over {v['num']} images: CRPS: {0.5 * pooled['CRPS']}, SSR: {pooled['SSR']} (SPREAD {0.5 * pooled['SPREAD']} / SKILL "
                      f"{0.5 * pooled['SKILL']}), RANK_DEV: {pooled['RANK_DEV']}, OUTLIERS: {pooled['OUTLIERS']} (nominal {pooled['OUTLIERS_nominal']}), "
                      f"invalid: {pooled['invalid']}")
                with open(os.path.join(result_root, k, "rank_hist.json"), "w") as f:
                    json.dump(dict(S=S, hist=pooled['hist'], N=pooled['N'], nominal=1.0 / (S + 1), invalid=pooled['invalid']), f)
    if K_sp is not None:  # the type's record: removed errors, ranks and totals pooled over its images, not the mean of the per-image areas
        for k, v in results.items():
            if not v['num'] or not v['sparsification']:
                continue
            pooled = sparsification_summary(*(torch.cat([rec[q] for rec in v['sparsification']]) for q in range(4)), K_sp)
            v['pooled_sparsification'] = pooled
            print(f"{k}, sparsification pooled over {len(v['sparsification'])} images: AUSE: {pooled['AUSE']}, AURG: {pooled['AURG']}, AUSE_RMSE: "
                  f"{pooled['AUSE_RMSE']}, AURG_RMSE: {pooled['AURG_RMSE']}, invalid: {pooled['invalid']}")
            with open(os.path.join(result_root, k, "sparsification.json"), "w") as f:  # curves of the [-1, 1] tensors times 0.25: RMSE's scale
                json.dump(dict(S=S, K=K_sp, fractions=pooled['fractions'], curve=[0.25 * c for c in pooled['curve']],
                               oracle=[0.25 * c for c in pooled['oracle']], random=[0.25 * c for c in pooled['random']], AUSE=pooled['AUSE'],
                               AURG=pooled['AURG'], N=pooled['N'], invalid=pooled['invalid']), f)
    if regions is not None:  # the type's record: sums and histograms pooled over its images region by region, then divided
        for k, v in results.items():
            if not v['num'] or not v['regions']:
                continue
            pooled = region_score_summary(*(torch.cat([rec[q] for rec in v['regions']]) for q in range(3)), S, regions["names"])
            v['pooled_regions'] = pooled
            for q in pooled["regions"]:
                for tag in ("CRPS", "RMSE", "BIAS"):
                    q[tag] = _scaled(q[tag], 0.5)
            print(f"{k}, regions ({regions['spec']}) pooled over {len(v['regions'])} images: "
                  + "; ".join(f"{q['name']}: N_PIX {q['N_PIX']}, RMSE {q['RMSE']}, CRPS {q['CRPS']}, BIAS {q['BIAS']}, SSR {q['SSR']}, ERR_SHARE "
                              f"{q['ERR_SHARE']}, PIX_SHARE {q['PIX_SHARE']}" for q in pooled["regions"])
                  + f"; invalid: {pooled['invalid']}, outside: {pooled['outside']}")
            with open(os.path.join(result_root, k, "regions.json"), "w") as f:  # CRPS / RMSE / BIAS on RMSE's x/2 + 0.5 scale
                json.dump(dict(spec=regions["spec"], S=S, L=pooled["L"], names=pooled["names"], images=len(v['regions']),
                               regions=pooled["regions"], N_PIX=pooled["N_PIX"], invalid=pooled["invalid"], outside=pooled["outside"]), f)
    if speckle is not None:  # the type's record: the mean of each metric over its images (not pooled sums: the images' means differ)
        for k, v in results.items():
            if not v['num'] or not v['speckle']:
                continue
            pooled = speckle_record(v['speckle'], speckle)
            v['pooled_speckle'] = pooled
            print(f"{k}, speckle ({speckle['spec']}) over {len(v['speckle'])} images: "
                  + ", ".join(f"{m}: {pooled['input'][m]}" for m in ("ENL", "ENL_AUTO", "SSI", "MEAN_RATIO", "VAR_RATIO", "LAP_RATIO"))
                  + f", EPI_in: {pooled['input']['EPI']}, EPI_gt: {pooled['target']['EPI']}"
                  + (f", ENL_member: {pooled['members']['ENL']}, LAP_RATIO_member: {pooled['members']['LAP_RATIO']}" if S > 1 else ""))
            with open(os.path.join(result_root, k, "speckle.json"), "w") as f:
                json.dump(dict(S=S, **pooled), f)
    if K_modes is not None:  # the type's record: the spectra added mode by mode over its images, not the mean of the per-image ratios
        for k, v in results.items():
            if not v['num'] or not v['modes']:
                continue
            pooled = ensemble_mode_summary(*(torch.cat([rec[q].reshape(1, -1) for rec in v['modes']]) for q in range(5)), S, True)['pooled']
            v['pooled_modes'] = pooled
            print(f"{k}, modes pooled over {len(v['modes'])} images: EFF_MODES: {pooled['EFF_MODES']}, EXPLAINED_1: {pooled['EXPLAINED'][0]}, "
                  f"SPAN_SHARE: {pooled['SPAN_SHARE']}, MODE_Z_RMS: {pooled['MODE_Z_RMS']}, refused: {pooled['refused']}")
            with open(os.path.join(result_root, k, "modes.json"), "w") as f:
                json.dump(dict(S=S, K=min(K_modes, S), **pooled), f)
    if args.spectra:  # the type's record: the power sums pooled over its images, not the mean of the per-image ratios; per image size
        for k, v in results.items():
            v['pooled_spectra'] = pool_spectra(v.get('spectra', []), S)
            sizes = sorted(v['pooled_spectra'])
            for Hs, Ws in sizes:
                pooled = v['pooled_spectra'][(Hs, Ws)]
                group = [sp for h, w, sp in v['spectra'] if (h, w) == (Hs, Ws)]
                _, bin_counts, freq = ops.radial_bins(Hs, Ws)
                of_size = "" if len(sizes) == 1 else f" of {Ws}x{Hs}"
                print(f"{k}, spectra pooled over {len(group)} images{of_size}: HF_RATIO: {pooled['HF_RATIO_output']}, LSD: {pooled['LSD_output']}"
                      + (f", HF_RATIO_member: {pooled['HF_RATIO_member']}, LSD_member: {pooled['LSD_member']}, SSR_HF: {pooled['SSR_HF']}"
                         if S > 1 else ""))
                with open(os.path.join(result_root, k, "spectra.json" if len(sizes) == 1 else f"spectra_{Ws}x{Hs}.json"), "w") as f:
                    json.dump(dict(S=S, H=Hs, W=Ws, images=len(group), freq=freq.tolist(), counts=bin_counts.tolist(), **pooled), f)
    if times:
        print(f"mean sampling time per image: {sum(times) / len(times):.3f} s ({getattr(sde, 'last_steps', sde.T)} steps)"
              + (f", solver order {sde.last_solver_order}" if hasattr(sde, 'last_solver_order') else "")
              + (f", {S} samples per image" if S > 1 else "")
              + ("" if kind is None else f", self-ensemble {kind}")
              + ("" if level is None else f", interval {level} (nominal {sde.last_order_stats['nominal']})")
              + ("" if getattr(sde, 'last_tiles', None) is None else ", {}x{} windows of {}x{}".format(*sde.last_tiles))
              + (f", graph reused for {n_replayed} of {len(times)} images" if getattr(sde, 'reuse_graph', False) else ""))
    if world > 1 and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return results


if __name__ == "__main__":
    main()
