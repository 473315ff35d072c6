"""`driftSDE` -- the instance-wise-drift diffusion of InstanceDiff on fused gfx950 kernels.

models/SDEs/driftSDE.py is absent from the reference snapshot; this class
implements the contract recoverable from its call sites:
  * forward_diffusion(x0, cond) -> (t, x_t, drift, std_noise, noise)      models/drift_noise_model.py:190
      x_t = x0 + drift_schedule[t]*(cond - x0) + max_sigma*sqrt(noise_schedule[t])*eps   (:492, :585)
  * reverse_ddpm(cond, names, text_encoder, reverse_type=, optimize_type=, image_context=) -> x0_hat   (:650)
  * indexable drift_schedule / noise_schedule, attrs T, max_sigma, set_gpu(device)   (:357,:490,:543; testUM.py:96)
  * ctor from `create_sde(nets, opt['sdes'][name])` with T, max_sigma, drift_schedule, noise_schedule
    (Configurations/config.yml:169-175; schedules 'sigmoid' | 'cosine' (drift_noise_model.py:10-16) | 'linear').
The reverse update is the build's frozen spec ("parity unpinned"):
    x_{t-1} = x_t - a_t*R_hat - b_t*eps_hat + c_t*z,   R_hat = drift_net(x_t-cond, cond, t), eps_hat = noise_net(x_t-cond, x_t, t)
with (a_t, b_t, c_t) from oracle-identical fp64 host arithmetic; ONE kernel per step does the update, draws z
(Philox) and emits the next step's `x_t - cond` network input.

Few-step sampling (`sample_T` / `sample_timesteps`): the same update evaluated as a jump between schedule points
t_0 = T > t_1 > ... > t_K = 0 instead of t -> t-1.  The nets get t_k itself: the tables stay on the training grid, so unlike IRSDE's
t*sample_scale no timestep rescaling is needed.  Training (forward_diffusion) is untouched and still draws t in [1, T].

Second-order multistep solver (`solver_order: 2`): the deterministic reverse path is the quadrature dx = R_hat dd + eps_hat dsigma,
so each jump extrapolates the two predictions linearly from the previous jump's, each in its own clock (two-step Adams-Bashforth with
variable steps), at no extra network evaluation.  It always runs the schedule path; order 1 (the default) is the update above, unchanged.

Posterior ensembles (`num_samples: S`): reverse_ddpm_ensemble draws S samples per input as rows of one batched chain and
reduces them on the device to a per-pixel mean and standard deviation.  Each row is a *member* whose noise comes from a Philox stream
of its own, a function of (seed, member id, draw index) only, so a member's image does not depend on the batch it was computed in.

Geometric self-ensembles (`self_ensemble: flips | dihedral`): with it the S members of reverse_ddpm_ensemble also differ in
orientation -- member s runs on the input flipped / transposed by code self_ensemble_codes(kind)[s % len(codes)] and is turned back before
the reduction: one permutation launch before the chain and one after it, no extra network cost.

Tiled sampling (`tile` / `tile_overlap`): an image larger than the window the nets are built for runs as a batch of
overlapping windows.  The state stays ONE full-resolution image: every step blends the windows' two predictions into full-image R_hat and
eps_hat, updates and draws the noise once per pixel on the full image (the plain chain's Philox counters, whatever the tiling), and cuts the
next step's window inputs out again -- one fused kernel per step beside the nets.

Ensembles of tiled chains (`tiled_ensemble: true`): off, num_samples > 1 and a tiling refuse each other.  On,
reverse_ddpm_ensemble runs an image larger than the window as tiled member chains: full-resolution member rows, grouped into chains of at
most max_chain_rows window rows, one fused kernel per step that blends, draws each row's z from its member's stream and scatters.

Credible intervals (`interval: L`): with it reverse_ddpm_ensemble also selects, per pixel, the order statistics of the S
members that bracket the central level-L interval and the median (one launch, values selected and never rounded) into
self.last_order_stats.  order_stat_indices states which order statistics those are and the coverage they nominally give.

Calibrating those intervals: with few members that nominal coverage lies below L.  conformal_scale finds, from per-image
counts of held-out images over calibration_grid's table of scale factors, the factor by which the interval must be widened about the
median (conformal risk control); its docstring states what the factor guarantees.  Both are pure host functions; the device side that
produces the counts and applies the factor is not part of the package yet (DESIGN.md §3 says why).

Graph reuse (`reuse_graph: true`): with it the sde keeps the captured step graph, the buffers it is baked on and the cache
values it reads in a Session per configuration, and a later image of the same shape only refills the buffers (one ops.chain_begin
launch) and replays.  The bits are those of the per-call path; what changes is who owns the graph's memory: the sde, until
close_sessions().
"""
import collections
import fractions
import itertools
import math
import numbers
import os
import weakref

import torch

from ... import ops


def _level_table(T, kind):
    t = torch.arange(T + 1, dtype=torch.float64)
    if kind == "cosine":
        lv = (1 - torch.cos(t * math.pi / T)) / 2
    elif kind == "sigmoid":
        k = 6.0
        s = torch.sigmoid(k * (2 * t / T - 1))
        s0, s1 = torch.sigmoid(torch.tensor(-k, dtype=torch.float64)), torch.sigmoid(torch.tensor(k, dtype=torch.float64))
        lv = (s - s0) / (s1 - s0)
    elif kind == "linear":
        lv = t / T
    else:
        raise ValueError(f"unknown schedule '{kind}'")
    lv[0] = 0.0
    lv[-1] = 1.0
    return lv.to(torch.float32)


def _step_coeffs(d, n, max_sigma, T, eta):
    d = d.to(torch.float64)
    s = max_sigma * torch.sqrt(n.to(torch.float64))
    a = torch.zeros(T + 1, dtype=torch.float64)
    b = torch.zeros(T + 1, dtype=torch.float64)
    c = torch.zeros(T + 1, dtype=torch.float64)
    for t in range(1, T + 1):
        a[t] = d[t] - d[t - 1]
        ratio = (s[t - 1] / s[t]) ** 2 if s[t] > 0 else 0.0
        et = eta * s[t - 1] * math.sqrt(max(1.0 - float(ratio), 0.0))
        keep = math.sqrt(max(float(s[t - 1]) ** 2 - et ** 2, 0.0))
        b[t] = s[t] - keep
        c[t] = et
    return a.to(torch.float32), b.to(torch.float32), c.to(torch.float32)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _sample_schedule(T, sample_T=None, sample_timesteps=None):
    """-> [t_0, ..., t_K = 0] for the reverse chain, or None when neither option is set (the plain T-step chain).
    sample_T = K (1 <= K <= T): t_k = ((K - k) * T) // K, so t_0 = T, t_K = 0 and every gap is >= T // K.
    sample_timesteps: a strictly decreasing list of ints in [1, T]; 0 is appended."""
    if sample_T is not None and _is_int(sample_T) and sample_T == -1:
        sample_T = None
    if sample_T is not None and sample_timesteps is not None:
        raise ValueError("driftSDE: set sample_T or sample_timesteps, not both")
    if sample_T is not None:
        if not _is_int(sample_T) or not 1 <= sample_T <= T:
            raise ValueError(f"driftSDE: sample_T must be an int in [1, T={T}] (or -1 / None: unset), got {sample_T!r}")
        K = int(sample_T)
        return [((K - k) * T) // K for k in range(K + 1)]
    if sample_timesteps is not None:
        ts = list(sample_timesteps)
        if not ts or not all(_is_int(t) and 1 <= t <= T for t in ts) or any(a <= b for a, b in zip(ts, ts[1:])):
            raise ValueError(f"driftSDE: sample_timesteps must be a non-empty, strictly decreasing list of ints in [1, T={T}], got {sample_timesteps!r}")
        return [int(t) for t in ts] + [0]
    return None


def _solver_order(order):
    """1 (None: unset) or 2, as an int; anything else -- bools, floats and strings included -- is refused"""
    if order is None:
        return 1
    if not _is_int(order) or order not in (1, 2):
        raise ValueError(f"driftSDE: solver_order must be the int 1 or 2, got {order!r}")
    return int(order)


def _num_samples(num):
    """ensemble size as an int >= 1 (None: 1, off); bools, floats and strings are refused like solver_order's"""
    if num is None:
        return 1
    if not _is_int(num) or num < 1:
        raise ValueError(f"driftSDE: num_samples must be an int >= 1 (or None: off), got {num!r}")
    return int(num)


def _interval(level):
    """credible level of the ensemble's interval maps as a float in (0, 1) (None: off); bools, ints and strings are refused like
    solver_order's"""
    if level is None:
        return None
    if not isinstance(level, float) or not 0.0 < level < 1.0:
        raise ValueError(f"driftSDE: interval must be a float in (0, 1) (or None: off), got {level!r}")
    return level


def order_stat_indices(S, level):
    """The order statistics (0-based, of S members sorted ascending) behind a central interval of credible level L, in exact rational
    arithmetic on the decimal the caller wrote (Fraction(str(level)): 0.9 is 9/10, not the double next to it):
        k_lo = floor((1 - L) / 2 * (S - 1)),  k_hi = S - 1 - k_lo      the interval [x_(k_lo), x_(k_hi)]
        k_m0 = (S - 1) // 2,  k_m1 = S // 2                            the median, 0.5 * (x_(k_m0) + x_(k_m1))
        nominal = (k_hi - k_lo) / (S + 1)                              the coverage S exchangeable draws give that pair
    With few members nominal lies below L (S = 4: min / max, 0.6)."""
    S = _num_samples(S)
    L = fractions.Fraction(str(_interval(level)))
    k_lo = math.floor((1 - L) / 2 * (S - 1))
    k_hi = S - 1 - k_lo
    return dict(k_lo=k_lo, k_hi=k_hi, k_m0=(S - 1) // 2, k_m1=S // 2, nominal=(k_hi - k_lo) / (S + 1))


def ensemble_score_summary(sums, counts, S):
    """The verification scores of an S-member ensemble from what ops.ensemble_scores returns, on the host:
        sums [..., 3] = sum crps, sum e, sum v;  counts [..., S + 2] = the rank histogram hist[0..S], then the invalid pixels.
    Rows (images) are pooled first, sums with sums and bins with bins: that is the aggregate over several images, the mean of
    per-image ratios is not.  ->  dict(
        N         sum hist: the valid pixels
        CRPS      sum crps / N
        SKILL     sqrt(sum e / N): the RMSE of the ensemble mean
        SPREAD    sqrt((S + 1)/S * sum v / N): the finite-ensemble correction under which a perfectly reliable ensemble has SSR 1
        SSR       SPREAD / SKILL;  NaN for S = 1 (no spread) or SKILL = 0
        RANK_DEV  sum_k |hist_k/N - 1/(S + 1)|: 0 for a flat histogram, 2S/(S + 1) when the truth always falls in one bin
        OUTLIERS  (hist_0 + hist_S)/N, the truth outside every member;  OUTLIERS_nominal = 2/(S + 1)
        hist      the pooled histogram, ints;  invalid  the pooled invalid count)
    Every ratio is NaN when N = 0.  Takes tensors, arrays or nested lists."""
    S = _num_samples(S)
    sums = torch.as_tensor(sums, dtype=torch.float64).detach().cpu().reshape(-1, 3)
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, S + 2)
    if sums.shape[0] != counts.shape[0]:
        raise ValueError(f"ensemble_score_summary: {sums.shape[0]} rows of sums, {counts.shape[0]} rows of counts")
    tot = [float(t) for t in sums.sum(dim=0)]
    pooled = [int(c) for c in counts.sum(dim=0)]
    hist, invalid = pooled[:S + 1], pooled[S + 1]
    N = sum(hist)
    nan = float("nan")
    if N == 0:
        return dict(N=0, CRPS=nan, SKILL=nan, SPREAD=nan, SSR=nan, RANK_DEV=nan, OUTLIERS=nan, OUTLIERS_nominal=2.0 / (S + 1), hist=hist,
                    invalid=invalid)
    skill = math.sqrt(tot[1] / N)
    spread = math.sqrt((S + 1) / S * tot[2] / N)
    return dict(N=N, CRPS=tot[0] / N, SKILL=skill, SPREAD=spread, SSR=spread / skill if S > 1 and skill > 0 else nan,
                RANK_DEV=sum(abs(h / N - 1.0 / (S + 1)) for h in hist), OUTLIERS=(hist[0] + hist[S]) / N, OUTLIERS_nominal=2.0 / (S + 1),
                hist=hist, invalid=invalid)


def _region_record(tot, pooled, S, err_total, pix_total, data_range):
    """one region's scores from its (pooled) four sums and S + 2 counts; every quotient is None without a valid pixel"""
    hist, invalid = pooled[:S + 1], pooled[S + 1]
    N = sum(hist)
    rec = dict(N_PIX=N, CRPS=None, RMSE=None, PSNR=None, BIAS=None, SSR=None, RANK_DEV=None, OUTLIERS=None, ERR_SHARE=None,
               PIX_SHARE=N / pix_total if pix_total else None, hist=hist, invalid=invalid)
    if N == 0:
        return rec
    skill = math.sqrt(tot[1] / N) if tot[1] >= 0 else float("nan")
    rec.update(CRPS=tot[0] / N, RMSE=skill, BIAS=tot[3] / N, PSNR=20.0 * math.log10(data_range / skill) if skill > 0 and math.isfinite(skill) else None,
               ERR_SHARE=tot[1] / err_total if err_total > 0 and math.isfinite(err_total) else None)
    if S > 1:
        spread = math.sqrt((S + 1) / S * tot[2] / N) if tot[2] >= 0 else float("nan")
        rec.update(SSR=spread / skill if skill > 0 else None, RANK_DEV=sum(abs(h / N - 1.0 / (S + 1)) for h in hist),
                   OUTLIERS=(hist[0] + hist[S]) / N)
    return rec


def region_score_summary(sums, counts, outside, S, names=None, data_range=2.0):
    """The per-region scores of N images from what ops.region_scores returns, on the host:
        sums [N, L, 4] = sum crps, sum e, sum v, sum m per region;  counts [N, L, S + 2] = the region's rank histogram hist[0..S], then
        its invalid pixels;  outside [N] = the pixels of no region.
    Images are pooled before dividing, sums with sums and bins with bins, as in ensemble_score_summary.  ->  dict(S, L, names,
        regions   one dict per region, pooled over the images:
            N_PIX      sum hist: the region's valid pixels
            CRPS       sum crps / N_PIX (the MAE for S = 1)
            RMSE       sqrt(sum e / N_PIX), of the ensemble mean;  PSNR = 20 log10(data_range / RMSE), None for RMSE = 0
            BIAS       sum m / N_PIX: the signed mean error
            SSR, RANK_DEV, OUTLIERS   exactly ensemble_score_summary's; None for S = 1
            ERR_SHARE  the region's sum e over all regions' sum e;  PIX_SHARE  its N_PIX over all regions' N_PIX
            hist, invalid
        images    the same list per image
        N_PIX, invalid, outside   the totals)
    A region without a valid pixel has None in every quotient: nothing divides by zero.  data_range is that of the tensors scored
    ([-1, 1]: 2).  names: L strings for the regions, default "0" .. "L-1".  Takes tensors, arrays or nested lists."""
    S = _num_samples(S)
    sums = torch.as_tensor(sums, dtype=torch.float64).detach().cpu()
    if sums.dim() < 2 or sums.shape[-1] != 4:
        raise ValueError(f"region_score_summary: sums must be [N, L, 4] or [L, 4], got {tuple(sums.shape)}")
    L = int(sums.shape[-2])
    sums = sums.reshape(-1, L, 4)
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, L, S + 2)
    outside = torch.as_tensor(outside).detach().cpu().to(torch.int64).reshape(-1)
    if not sums.shape[0] == counts.shape[0] == outside.shape[0]:
        raise ValueError(f"region_score_summary: {sums.shape[0]} rows of sums, {counts.shape[0]} of counts, {outside.shape[0]} of outside")
    names = [str(i) for i in range(L)] if names is None else [str(n) for n in names]
    if len(names) != L:
        raise ValueError(f"region_score_summary: {len(names)} names for L = {L} regions")
    if not data_range > 0:
        raise ValueError(f"region_score_summary: data_range must be > 0, got {data_range!r}")

    def table(s, c):  # s [L][4], c [L][S + 2] as lists
        err_total = sum(s[l][1] for l in range(L) if sum(c[l][:S + 1]) > 0)
        pix_total = sum(sum(c[l][:S + 1]) for l in range(L))
        return [dict(name=names[l], **_region_record(s[l], c[l], S, err_total, pix_total, data_range)) for l in range(L)]

    regions = table(sums.sum(dim=0).tolist(), counts.sum(dim=0).tolist())
    images = [table(s, c) for s, c in zip(sums.tolist(), counts.tolist())]
    return dict(S=S, L=L, names=names, regions=regions, images=images, N_PIX=sum(r["N_PIX"] for r in regions),
                invalid=sum(r["invalid"] for r in regions), outside=int(outside.sum()))


DESPECKLE_METRICS = ("MEAN", "STD", "ENL", "MEAN_REF", "ENL_REF", "SSI", "SMPI", "MEAN_RATIO", "VAR_RATIO", "ENL_RATIO", "EPI", "LAP_RATIO",
                     "CNR")
_FLAT_EPS = 8 * 2.0 ** -53  # despeckle_summary: a variance at or below this share of the sum of squares is rounding, not signal


def _moments(n, s1, s2):
    """n terms with fp64 sums s1 = sum t, s2 = sum t^2 -> (mean, population variance, flat) as exact Fractions of the rounded sums, or None
    for n = 0 or a non-finite sum.  flat: variance <= 8 * 2^-53 * s2.  Each sum carries at most 2 (n - 1) 2^-53 sum |t| of rounding, which
    is at most 6 n 2^-53 (s2 / n) on the variance; the factor 8 leaves a margin over that, so a constant region is always flat."""
    if n <= 0 or not (math.isfinite(s1) and math.isfinite(s2)):
        return None
    mean = fractions.Fraction(s1) / n
    var = fractions.Fraction(s2) / n - mean * mean
    return mean, var, var <= fractions.Fraction(_FLAT_EPS) * fractions.Fraction(s2)


def _root(q):
    """sqrt of a non-negative Fraction as a float; the quotient is formed exactly first"""
    return math.sqrt(float(q)) if q > 0 else 0.0


def _despeckle_region(s, c):
    """one region of one row from its 12 sums and 4 counts; CNR is filled in by the caller, which knows the background"""
    n, n_ratio, n_sten, invalid = (int(v) for v in c)
    rec = dict(N_PIX=n, N_RATIO=n_ratio, N_STENCIL=n_sten, invalid=invalid, FLAT=None, **{m: None for m in DESPECKLE_METRICS})
    ma, my = _moments(n, s[0], s[1]), _moments(n, s[2], s[3])
    if ma is not None:
        rec.update(MEAN=float(ma[0]), STD=_root(ma[1]), FLAT=bool(ma[2]))
        if not ma[2]:
            rec["ENL"] = float(ma[0] * ma[0] / ma[1])
    if my is not None:
        rec["MEAN_REF"] = float(my[0])
        if not my[2]:
            rec["ENL_REF"] = float(my[0] * my[0] / my[1])
    if ma is not None and my is not None and not my[2] and ma[1] >= 0:  # zero variance of the reference: no SSI / SMPI
        if ma[0] != 0 and my[0] != 0:
            rec["SSI"] = _root((ma[1] / (ma[0] * ma[0])) / (my[1] / (my[0] * my[0]))) * (1.0 if (ma[0] > 0) == (my[0] > 0) else -1.0)
        rec["SMPI"] = (1.0 + abs(float(my[0] - ma[0]))) * _root(ma[1] / my[1])
    mr = _moments(n_ratio, s[5], s[6])
    if mr is not None:
        rec.update(MEAN_RATIO=float(mr[0]), VAR_RATIO=max(float(mr[1]), 0.0))
        if not mr[2]:
            rec["ENL_RATIO"] = float(mr[0] * mr[0] / mr[1])
    la, ly = _moments(n_sten, s[7], s[9]), _moments(n_sten, s[8], s[10])
    if la is not None and ly is not None and math.isfinite(s[11]):
        if not la[2] and not ly[2]:
            cov = fractions.Fraction(s[11]) / n_sten - la[0] * ly[0]
            rec["EPI"] = math.copysign(_root(cov * cov / (la[1] * ly[1])), 1.0 if cov >= 0 else -1.0)
        if s[10] > 0:
            rec["LAP_RATIO"] = float(fractions.Fraction(s[9]) / fractions.Fraction(s[10]))
    return rec


def _despeckle_rows(sums, counts, who):
    sums = torch.as_tensor(sums, dtype=torch.float64).detach().cpu()
    if sums.dim() < 2 or sums.shape[-1] != ops.DESPECKLE_NQ:
        raise ValueError(f"{who}: sums must be [..., L, {ops.DESPECKLE_NQ}], got {tuple(sums.shape)}")
    L = int(sums.shape[-2])
    lead = tuple(sums.shape[:-2])
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64)
    if tuple(counts.shape) != lead + (L, ops.DESPECKLE_NC):
        raise ValueError(f"{who}: counts must be {lead + (L, ops.DESPECKLE_NC)} for sums {tuple(sums.shape)}, got {tuple(counts.shape)}")
    return sums.reshape(-1, L, ops.DESPECKLE_NQ).tolist(), counts.reshape(-1, L, ops.DESPECKLE_NC).tolist(), L, lead


def despeckle_summary(sums, counts, outside, names=None, background=0):
    """The no-reference despeckling statistics from what ops.despeckle_stats returns, on the host:
        sums [..., L, 12], counts [..., L, 4] (the leading axes, [B, S] from the device, are flattened into rows), outside [B].
    ->  dict(L, names, background, shape (the leading axes), outside (total),
        rows      per row a list of one dict per region:
            N_PIX, N_RATIO, N_STENCIL, invalid   the region's valid / ratio / stencil / invalid pixels
            MEAN, STD     of a over the valid pixels (population variance);  MEAN_REF  of y
            FLAT          variance <= 8 * 2^-53 * sum a^2: what is left is the rounding of the sums (see _moments);  ENL is None then
            ENL           MEAN^2 / variance, the equivalent number of looks;  ENL_REF  that of y
            SSI           (STD / MEAN) / (STD_ref / MEAN_ref);  SMPI = (1 + |MEAN_ref - MEAN|) STD / STD_ref
            MEAN_RATIO, VAR_RATIO   of the ratio image rho = y / a over the ratio pixels;  ENL_RATIO = MEAN_RATIO^2 / VAR_RATIO, the
                          looks of the input when only speckle was removed
            EPI           the Pearson correlation of La and Ly over the stencil pixels;  LAP_RATIO = sum La^2 / sum Ly^2
            CNR           |MEAN - MEAN_bg| / sqrt(var + var_bg) against region `background` of the same row
        regions   per region the mean of each metric over the rows where it is defined and, under "defined", the number of those rows)
    Rows are not pooled sum with sum: that would carry the images' different means into the variance.  Variances and the EPI's numerator
    and denominators are combined from the fp64 sums in exact rational arithmetic.  An empty region, a reference of zero variance or a
    region without a stencil pixel gives None, never a division by zero.  Takes tensors, arrays or nested lists."""
    s_rows, c_rows, L, lead = _despeckle_rows(sums, counts, "despeckle_summary")
    outside = torch.as_tensor(outside).detach().cpu().to(torch.int64).reshape(-1)
    names = [str(i) for i in range(L)] if names is None else [str(n) for n in names]
    if len(names) != L:
        raise ValueError(f"despeckle_summary: {len(names)} names for L = {L} regions")
    if isinstance(background, bool) or not isinstance(background, int) or not 0 <= background < L:
        raise ValueError(f"despeckle_summary: background must be a region index in [0, {L}), got {background!r}")
    rows = []
    for s, c in zip(s_rows, c_rows):
        recs = [dict(name=names[l], **_despeckle_region(s[l], c[l])) for l in range(L)]
        mom = [_moments(c[l][0], s[l][0], s[l][1]) for l in range(L)]
        bg = mom[background]
        for l in range(L):
            if mom[l] is not None and bg is not None:
                den = max(mom[l][1], 0) + max(bg[1], 0)
                if den > 0:
                    d = mom[l][0] - bg[0]
                    recs[l]["CNR"] = _root(d * d / den)
        rows.append(recs)
    regions = []
    for l in range(L):
        rec = dict(name=names[l], N_PIX=sum(r[l]["N_PIX"] for r in rows), invalid=sum(r[l]["invalid"] for r in rows), defined={})
        for m in DESPECKLE_METRICS:
            have = [r[l][m] for r in rows if r[l][m] is not None]
            rec[m] = math.fsum(have) / len(have) if have else None
            rec["defined"][m] = len(have)
        regions.append(rec)
    return dict(L=L, names=names, background=background, shape=list(lead), rows=rows, regions=regions, outside=int(outside.sum()))


def homogeneous_cells(sums, counts, share=0.25):
    """The customary "ENL in homogeneous regions" without a hand-drawn map: per row of ops.despeckle_stats' record (over a grid of cells,
    ops.grid_labels) the ceil(share * non-empty cells) cells with the lowest coefficient of variation of the *reference* (compared as
    exact rationals; ties go to the lower index; a cell whose reference mean is 0 ranks last) -> dict(cells: per row the chosen region
    indices in rank order, ENL_AUTO: per row the mean ENL of the restored rows over the chosen cells where it is defined, else None)."""
    if isinstance(share, bool) or not isinstance(share, numbers.Real) or not 0 < share <= 1:
        raise ValueError(f"homogeneous_cells: share must be in (0, 1], got {share!r}")
    s_rows, c_rows, L, _ = _despeckle_rows(sums, counts, "homogeneous_cells")
    cells, auto = [], []
    for s, c in zip(s_rows, c_rows):
        ranked = []
        for l in range(L):
            my = _moments(c[l][0], s[l][2], s[l][3])
            if my is None:
                continue
            cv2 = max(my[1], 0) / (my[0] * my[0]) if my[0] != 0 else None
            ranked.append((cv2 is None, cv2 if cv2 is not None else 0, l))
        ranked.sort()
        k = max(1, math.ceil(share * len(ranked) - 1e-9)) if ranked else 0  # 0.1 * 10 is one cell, whatever the product's last bit
        chosen = [l for _, _, l in ranked[:k]]
        enl = [e for e in (_despeckle_region(s[l], c[l])["ENL"] for l in chosen) if e is not None]
        cells.append(chosen)
        auto.append(math.fsum(enl) / len(enl) if enl else None)
    return dict(cells=cells, ENL_AUTO=auto)


def _sparsification_K(K):
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= ops.SPARSIFICATION_MAX_K:
        raise ValueError(f"sparsification: K must be an int in [1, {ops.SPARSIFICATION_MAX_K}], got {K!r}")
    return K


def _pooled_removal(sums, counts, K, who):
    """rows of ops.sparsification's (sums, counts) -> the pooled (R[k], m[k], total, N, invalid): per row m_k = floor(k N / K) and
    R_k = A_k + (m_k - c_k) T_k / t_k, the expected error of the m_k pixels removed under a random order inside the tie group"""
    sums = torch.as_tensor(sums, dtype=torch.float64).detach().cpu().reshape(-1, K + 1, 2).tolist()
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, K + 1, 2).tolist()
    if len(sums) != len(counts):
        raise ValueError(f"sparsification_summary: {len(sums)} rows of {who} sums, {len(counts)} rows of counts")
    R, m, total, N, invalid = [0.0] * K, [0] * K, 0.0, 0, 0
    for s, c in zip(sums, counts):
        n = c[K][0]
        invalid += c[K][1]
        if n == 0:
            continue
        N += n
        total += s[K][0]
        for k in range(K):
            mk = k * n // K
            if mk == 0:
                continue
            ck, tk = c[k]
            m[k] += mk
            R[k] += s[k][0] + ((mk - ck) * s[k][1] / tk if tk else 0.0)
    return R, m, total, N, invalid


def sparsification_summary(sums, counts, sums_oracle, counts_oracle, K):
    """The sparsification curves of an uncertainty map from what ops.sparsification returns for the map (sums, counts) and for the
    oracle (key=None: sums_oracle, counts_oracle), on the host in float64.  Rows (images) are pooled first: R_k, m_k, the totals and N
    are summed over the rows before any division (a row with N = 0 adds nothing), which is the aggregate over several images; the
    mean of per-image ratios is not.  ->  dict(
        fractions   k/K, k = 0 .. K-1: the share of pixels removed
        curve       (total - R_k)/(N - m_k): the mean squared error of the pixels that remain after the m_k most uncertain are removed
        oracle      the same with the pixels removed by their error: the lowest curve any map can reach
        random      total/N at every k: removal in random order
        curve_norm, oracle_norm, random_norm    each divided by its k = 0 value
        AUSE        the area between curve_norm and oracle_norm (trapezoid rule over fractions): 0 for a perfect ranking
        AURG        the area between random_norm and curve_norm: <= 0 for a map no better than chance
        AUSE_RMSE, AURG_RMSE    the same on the square roots of the curves
        N, invalid  the map's pooled valid and invalid pixels)
    K = 1 (one point, no area) or no valid pixel gives NaN areas.  Takes tensors, arrays or nested lists."""
    K = _sparsification_K(K)
    R, m, total, N, invalid = _pooled_removal(sums, counts, K, "the map's")
    Ro, mo, total_o, No, _ = _pooled_removal(sums_oracle, counts_oracle, K, "the oracle's")
    nan = float("nan")
    frac = [k / K for k in range(K)]
    curve = [(total - R[k]) / (N - m[k]) for k in range(K)] if N else [nan] * K
    oracle = [(total_o - Ro[k]) / (No - mo[k]) for k in range(K)] if No else [nan] * K
    random = [total / N if N else nan] * K

    def norm(c):
        return [v / c[0] if c[0] > 0 else nan for v in c]

    def area(a, b):  # the trapezoid rule on a - b over the fractions
        d = [x - y for x, y in zip(a, b)]
        return sum(0.5 * (d[k] + d[k + 1]) * (frac[k + 1] - frac[k]) for k in range(K - 1)) if K > 1 else nan

    def root(c):
        return [math.sqrt(v) if v >= 0 else nan for v in c]

    cn, on, rn = norm(curve), norm(oracle), norm(random)
    cr, orr, rr = norm(root(curve)), norm(root(oracle)), norm(root(random))
    return dict(fractions=frac, curve=curve, oracle=oracle, random=random, curve_norm=cn, oracle_norm=on, random_norm=rn,
                AUSE=area(cn, on), AURG=area(rn, cn), AUSE_RMSE=area(cr, orr), AURG_RMSE=area(rr, cr), N=N, invalid=invalid)


def spectrum_summary(spectra, counts, S, L=None):
    """The scale-by-scale scores of a restoration or an S-member ensemble from what driftSDE.power_spectra returns, on the host in
    float64.  spectra: a dict of per-bin power sums (ops.radial_power_spectrum) with the keys output, target, residual [..., nb] and
    for S > 1 also members and member_residuals [..., S, nb]; counts [nb]: ops.radial_bins' points per bin; L = max(H, W), the bins'
    scale (bin k is k / L cycles per pixel; it may be left out for a square image only, whose counts name it: others are refused).  Rows (images) are
    pooled first, sums with sums, as in ensemble_score_summary; n rows of a bin hold n * counts[k] points.  -> dict(
        n                   the rows pooled
        PSD_output, PSD_target, PSD_residual [nb]   pooled sum / (n counts): the mean power per frequency point of the bin
        PSD_member, PSD_member_residual [nb]        the same, averaged over the S members (S > 1)
        RATIO_output [nb]   PSD_output / PSD_target: below 1 where the restoration lacks the truth's power (over-smoothing), above 1
                            where it adds power;  RATIO_member [nb] the same for the members' mean power
        HF_RATIO_output, HF_RATIO_member   the same ratios of the power summed over the bins k > L/4 (above half Nyquist)
        LSD_output, LSD_member             the log-spectral distance sqrt(mean_k (10 log10 ratio_k)^2) in dB over 1 <= k <= L/2, the
                                           bins with both powers > 0
        SPREAD_PSD [nb]     S/(S - 1) (mean_s PSD_member_s - PSD_output): the members' variance about their mean, per frequency
        SKILL_PSD [nb]      PSD_residual: the squared error of the mean, per frequency
        SSR_k [nb]          sqrt((S + 1)/S SPREAD_PSD / SKILL_PSD), ensemble_score_summary's spread-skill ratio separated per
                            frequency: 1 at every k for a reliable ensemble, below 1 where it is under-dispersive
        SSR_HF              the same from the sums over k > L/4)
    A value is NaN where its denominator is 0 (or negative from rounding), and the spread entries are NaN for S = 1."""
    S = _num_samples(S)
    counts = [int(c) for c in torch.as_tensor(counts).detach().cpu().reshape(-1).tolist()]
    nb = len(counts)
    if L is None:  # only a square image's scale can be read off its counts: they must be radial_bins(L, L)'s own
        L = math.isqrt(sum(counts))
        if L < 1 or L * L != sum(counts) or ops.radial_bins(L, L)[1].tolist() != counts:
            raise ValueError("spectrum_summary: counts are not those of a square image; pass L = max(H, W)")
    nan = float("nan")
    keys = ("output", "target", "residual") + (("members", "member_residuals") if S > 1 else ())
    pooled, n = {}, None
    for key in keys:
        t = torch.as_tensor(spectra[key], dtype=torch.float64).detach().cpu()
        t = t.reshape(-1, S, nb) if key.startswith("member") else t.reshape(-1, nb)
        if n is not None and t.shape[0] != n:
            raise ValueError(f"spectrum_summary: {t.shape[0]} rows of {key}, {n} of output")
        n = t.shape[0]
        pooled[key] = t.sum(dim=0).tolist()

    def div(a, b):
        return a / b if b > 0 else nan

    def root(a):
        return math.sqrt(a) if a >= 0 else nan

    psd = {key: [div(v, n * c) for v, c in zip(pooled[key], counts)] for key in ("output", "target", "residual")}
    out = dict(n=n, PSD_output=psd["output"], PSD_target=psd["target"], PSD_residual=psd["residual"])
    tot = {"output": pooled["output"], "target": pooled["target"], "residual": pooled["residual"]}
    if S > 1:
        tot["member"] = [sum(pooled["members"][s][k] for s in range(S)) / S for k in range(nb)]
        tot["member_residual"] = [sum(pooled["member_residuals"][s][k] for s in range(S)) / S for k in range(nb)]
        out["PSD_member"] = [div(v, n * c) for v, c in zip(tot["member"], counts)]
        out["PSD_member_residual"] = [div(v, n * c) for v, c in zip(tot["member_residual"], counts)]
    hf = [k for k in range(nb) if 4 * k > L]
    for tag in ("output",) + (("member",) if S > 1 else ()):
        ratio = [div(a, b) for a, b in zip(tot[tag], tot["target"])]
        out["RATIO_" + tag] = ratio
        out["HF_RATIO_" + tag] = div(sum(tot[tag][k] for k in hf), sum(tot["target"][k] for k in hf))
        db = [10.0 * math.log10(tot[tag][k] / tot["target"][k]) for k in range(1, nb) if 2 * k <= L and tot[tag][k] > 0 and tot["target"][k] > 0]
        out["LSD_" + tag] = math.sqrt(sum(d * d for d in db) / len(db)) if db else nan
    if S > 1:
        spread = [S / (S - 1) * (a - b) for a, b in zip(tot["member"], tot["output"])]  # power sums; the PSDs divide both by n counts
        out["SPREAD_PSD"] = [div(v, n * c) for v, c in zip(spread, counts)]
        out["SSR_k"] = [root(div((S + 1) / S * a, b)) for a, b in zip(spread, tot["residual"])]
        out["SSR_HF"] = root(div((S + 1) / S * sum(spread[k] for k in hf), sum(tot["residual"][k] for k in hf)))
    else:
        out["SPREAD_PSD"], out["SSR_k"], out["SSR_HF"] = [nan] * nb, [nan] * nb, nan
    out["SKILL_PSD"] = psd["residual"]
    return out


def ensemble_distance_summary(d2, counts, S, has_target):
    """The image-level scores of an S-member ensemble from what ops.ensemble_distances returns, on the host in float64:
        d2 [..., M, M] squared distances between an image's M = S + has_target rows (members, then the target); counts [..., 2] =
        (valid, invalid) pixels.  Per image, with dist = sqrt(d2), a = sum_i dist[i][S] / S, p = sum_{i != j < S} dist[i][j] (both
        orders, added in index order) and r = sqrt(valid), so that every distance is a root-mean-square over the valid pixels:
        ES          (a - p / (2 S^2)) / r      the energy score of the members' empirical distribution, the image-level counterpart
                                               of the per-pixel CRPS of ensemble_score_summary (same form: the truth sits in no pair)
        ES_FAIR     (a - p / (2 S (S - 1))) / r   the unbiased ("fair") estimate of the underlying distribution's score; NaN for S = 1
        DIVERSITY   p / (S (S - 1)) / r        the mean pairwise member distance; NaN for S = 1
        RMS_member  a / r ;  RMS_best = min_i dist[i][S] / r ;  RMS_medoid = dist[medoid][S] / r
        medoid      the first i that minimises sum_{j < S, j != i} dist[i][j] (the scan of idiff_ensemble_distances);  best  the first i
                    that minimises d2[i][S], -1 without a target
        valid, invalid
    ES, ES_FAIR, RMS_member, RMS_best and RMS_medoid are NaN without a target; every score is NaN for an image with no valid pixel
    (medoid 0, best 0 or -1).  Both scores are proper only in expectation over ensembles; ES carries a bias of p / (2 S^2 (S - 1)) / r
    that rewards a small spread at small S, so to compare ensembles of different spread (or different S) use ES_FAIR.
    -> dict(key -> the list over images, 'mean' -> dict(key -> the mean of that list over the images): these are per-image scores, so
    pooling is the mean, unlike the sums of ensemble_score_summary).  Takes tensors, arrays or nested lists."""
    S = _num_samples(S)
    M = S + (1 if has_target else 0)
    d2 = torch.as_tensor(d2, dtype=torch.float64).detach().cpu().reshape(-1, M, M).tolist()
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, 2).tolist()
    if len(d2) != len(counts):
        raise ValueError(f"ensemble_distance_summary: {len(d2)} matrices, {len(counts)} rows of counts")
    nan = float("nan")
    keys = ("ES", "ES_FAIR", "DIVERSITY", "RMS_member", "RMS_best", "RMS_medoid", "medoid", "best", "valid", "invalid")
    out = {k: [] for k in keys}
    for mat, (valid, invalid) in zip(d2, counts):
        dist = [[math.sqrt(v) for v in row] for row in mat]
        rows = []
        for i in range(S):
            m = 0.0
            for j in range(S):
                if j != i:
                    m += dist[i][j]
            rows.append(m)
        medoid = min(range(S), key=lambda i: (rows[i], i))
        best = min(range(S), key=lambda i: (mat[i][S], i)) if has_target else -1
        one = dict(ES=nan, ES_FAIR=nan, DIVERSITY=nan, RMS_member=nan, RMS_best=nan, RMS_medoid=nan, medoid=medoid, best=best, valid=valid,
                   invalid=invalid)
        if valid > 0:
            r = math.sqrt(valid)
            p = 0.0
            for m in rows:
                p += m
            if S > 1:
                one["DIVERSITY"] = p / (S * (S - 1)) / r
            if has_target:
                a = 0.0
                for i in range(S):
                    a += dist[i][S]
                a /= S
                one["ES"] = (a - p / (2 * S * S)) / r
                if S > 1:
                    one["ES_FAIR"] = (a - p / (2 * S * (S - 1))) / r
                one["RMS_member"], one["RMS_best"], one["RMS_medoid"] = a / r, dist[best][S] / r, dist[medoid][S] / r
        for k in keys:
            out[k].append(one[k])
    out["mean"] = {k: (sum(out[k]) / len(out[k]) if out[k] else nan) for k in keys}
    return out


def _mode_record(lams, ts, tnorm2, valid, S, has_target):
    """the scores of one spectrum: lams / ts the live modes' eigenvalues and target coordinates (MODE_Z_RMS is the caller's)"""
    nan = float("nan")
    total = sum(lams)
    one = dict(EXPLAINED=[nan] * S, EFF_MODES=nan, MODE_STD=[nan] * S, SPAN_SHARE=nan, MODE_Z=[nan] * S, MODE_Z_RMS=nan)
    if lams and total > 0:
        one["EFF_MODES"] = total * total / sum(v * v for v in lams)
        for k, v in enumerate(lams):
            one["EXPLAINED"][k] = v / total
            if S > 1 and valid > 0 and v > 0:
                one["MODE_STD"][k] = math.sqrt(v / ((S - 1) * valid))
    if has_target:
        if tnorm2 > 0:
            one["SPAN_SHARE"] = sum(t * t for t in ts) / tnorm2
        if S > 1:
            for k, (v, t) in enumerate(zip(lams, ts)):
                if v > 0:
                    one["MODE_Z"][k] = t / math.sqrt(v / (S - 1) * (1 + 1 / S))
    return one


def ensemble_mode_summary(lam, tcoord, tnorm2, info, counts, S, has_target):
    """What the principal modes of an S-member ensemble say, from what ops.ensemble_modes and ops.ensemble_distances return, on the host
    in float64: lam [..., S], tcoord [..., S], tnorm2 [...], info [..., 2] = (rank, sweeps), counts [..., 2] = (valid, invalid) pixels.
    The live modes of an image are its first `rank` ones.  Per image:
        EXPLAINED[k]  lam_k / sum of the live lam: the share of the ensemble's variance along mode k
        EFF_MODES     (sum lam)^2 / sum lam^2 over the live modes, the participation ratio: 1 for a single mode, S - 1 for an isotropic
                      ensemble -- how many degrees of freedom the members really have
        MODE_STD[k]   sqrt(lam_k / ((S - 1) valid)): the standard deviation along mode k as a per-pixel root mean square
        SPAN_SHARE    sum of t_k^2 over the live modes / tnorm2: the share of the mean's squared error that lies inside the span of the
                      members' variation (with a target)
        MODE_Z[k]     t_k / sqrt(lam_k / (S - 1) (1 + 1 / S)): the error of the mean along mode k in units of the spread along it (the
                      factor 1 + 1/S is the mean's own sampling variance)
        MODE_Z_RMS    the root mean square of MODE_Z over the live modes: near 1 the spread along the ensemble's own modes matches the
                      error, above 1 the ensemble is under-dispersed
        rank, sweeps, valid, invalid
    Lists over modes have length S, NaN at the dead modes; the target's keys are NaN without one; an image of rank 0 (S = 1, no valid
    pixel, equal members) has NaN scores but SPAN_SHARE = 0 when the mean is in error; an image the kernel refused (rank -1: a NaN,
    infinite or negative distance) is NaN throughout and is left out of the pooled record, which counts it in 'refused'.
    'pooled' treats the images as one: the spectra are added mode by mode (sum over images of lam_k where live) and EXPLAINED, EFF_MODES
    and MODE_STD are read off the sum, the latter with the pooled valid pixels; SPAN_SHARE = sum of all live t_k^2 / sum of tnorm2;
    MODE_Z_RMS is over all images' live modes.
    Caveat: at small S the leading sample eigenvalues are biased upward (and the trailing ones downward), so the leading MODE_Z are
    biased low and EFF_MODES is an underestimate; compare ensembles at equal S.
    -> dict(key -> the list over images, 'pooled' -> dict).  Takes tensors, arrays or nested lists."""
    S = _num_samples(S)
    lam = torch.as_tensor(lam, dtype=torch.float64).detach().cpu().reshape(-1, S).tolist()
    tcoord = torch.as_tensor(tcoord, dtype=torch.float64).detach().cpu().reshape(-1, S).tolist()
    tnorm2 = torch.as_tensor(tnorm2, dtype=torch.float64).detach().cpu().reshape(-1).tolist()
    info = torch.as_tensor(info).detach().cpu().to(torch.int64).reshape(-1, 2).tolist()
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, 2).tolist()
    if not len(lam) == len(tcoord) == len(tnorm2) == len(info) == len(counts):
        raise ValueError(f"ensemble_mode_summary: {len(lam)} spectra, {len(tcoord)} rows of coordinates, {len(tnorm2)} norms, {len(info)} rows "
                         f"of info, {len(counts)} rows of counts")
    has_target = bool(has_target)
    nan = float("nan")
    keys = ("EXPLAINED", "EFF_MODES", "MODE_STD", "SPAN_SHARE", "MODE_Z", "MODE_Z_RMS", "rank", "sweeps", "valid", "invalid")
    out = {k: [] for k in keys}
    pool_lam, pool_t2, pool_n2, pool_z2, pool_nz, pool_valid, pool_invalid, refused = [0.0] * S, 0.0, 0.0, 0.0, 0, 0, 0, 0
    for l, t, n2, (rank, sweeps), (valid, invalid) in zip(lam, tcoord, tnorm2, info, counts):
        if rank < 0:
            one = _mode_record([], [], nan, 0, S, False)
            refused += 1
        else:
            rank = min(rank, S)
            one = _mode_record(l[:rank], t[:rank], n2, valid, S, has_target)
            if has_target and S > 1 and rank > 0:
                z2 = sum(z * z for z in one["MODE_Z"][:rank])
                one["MODE_Z_RMS"] = math.sqrt(z2 / rank)
                pool_z2 += z2
                pool_nz += rank
            for k in range(rank):
                pool_lam[k] += l[k]
                pool_t2 += t[k] * t[k]
            pool_n2 += n2
            pool_valid += valid
            pool_invalid += invalid
        one.update(rank=rank, sweeps=sweeps, valid=valid, invalid=invalid)
        for k in keys:
            out[k].append(one[k])
    live = 0
    while live < S and pool_lam[live] > 0:
        live += 1
    pooled = _mode_record(pool_lam[:live], [], 0.0, pool_valid, S, False)
    if has_target:
        if pool_n2 > 0:
            pooled["SPAN_SHARE"] = pool_t2 / pool_n2
        if pool_nz:
            pooled["MODE_Z_RMS"] = math.sqrt(pool_z2 / pool_nz)
    del pooled["MODE_Z"]
    pooled.update(images=len(lam) - refused, refused=refused, valid=pool_valid, invalid=pool_invalid)
    out["pooled"] = pooled
    return out


def calibration_grid(lam_max=8.0, G=513):
    """The table of scale factors a calibration searches: lam_g = g * lam_max / (G - 1), g = 0 .. G - 1, computed in double and rounded
    to float32, as a list of G floats (each a float32 value).  2 <= G <= 1024, lam_max finite and > 0; refused if the rounded table is
    not strictly ascending (a lam_max so small that neighbours collapse)."""
    if not _is_int(G) or not 2 <= G <= 1024:
        raise ValueError(f"calibration_grid: G must be an int in [2, 1024], got {G!r}")
    if isinstance(lam_max, bool) or not isinstance(lam_max, (int, float)) or not (math.isfinite(lam_max) and lam_max > 0):
        raise ValueError(f"calibration_grid: lam_max must be a finite number > 0, got {lam_max!r}")
    table = torch.tensor([g * float(lam_max) / (G - 1) for g in range(G)], dtype=torch.float64).to(torch.float32)
    if not bool(torch.isfinite(table).all()) or not bool((table[1:] > table[:-1]).all()):
        raise ValueError(f"calibration_grid: {G} points up to lam_max = {lam_max!r} are not strictly ascending in float32")
    return [float(v) for v in table]


def conformal_scale(counts, alpha, lams):
    """The calibrated scale factor from the counts of N held-out images (conformal risk control), on the host, in exact rational
    arithmetic (alpha = Fraction(str(alpha)), as order_stat_indices reads its level).
        counts [N][G + 2]   one row per image, in any order: bin g < G = the pixels whose target first lies inside the interval scaled
                            about the median by lams[g] (lo_out = c - lam*(c - lo), hi_out = c + lam*(hi - c)), bin G = the pixels no
                            entry covers, bin G + 1 = the invalid pixels (a NaN, or not lo <= c <= hi)
        n_i    = sum(counts[i][:G + 1])                    the image's valid pixels; a row with n_i = 0 is refused
        L_i(g) = 1 - sum(counts[i][:g + 1]) / n_i          the share of the image's valid pixels outside the interval scaled by lams[g]
        g^     = the smallest g with (sum_i L_i(g) + 1) / (N + 1) <= alpha ;  lam^ = lams[g^]
    -> dict(lam, g, alpha, N, bound, risk, reached, invalid): bound is the left side at g^ (at the last g when no g qualifies), risk
    the list of the N-image mean loss per g, invalid the pooled invalid pixels.  If no g of the table qualifies, reached is False and lam
    and g are None: the table ends too early (a larger lam_max).  N + 1 < 1 / alpha makes the bound unreachable at any lam, since
    the left side is at least 1 / (N + 1): that raises a ValueError naming the least N.
    Guarantee: if the calibration images and a new image are exchangeable, and since the loss lies in [0, 1] and does not increase with
    lam, the EXPECTED share of the new image's pixels outside its interval scaled by lam^ is at most alpha.  That is a statement about
    the image-level risk in expectation over the draw of the calibration set and the new image.  It is not per-pixel coverage, and it
    is not a bound that holds for each image."""
    lams = [float(v) for v in torch.as_tensor(lams).detach().cpu().reshape(-1).tolist()]
    G = len(lams)
    if G < 1:
        raise ValueError("conformal_scale: the table is empty")
    rows = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, G + 2).tolist()
    N = len(rows)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, str, fractions.Fraction)):
        raise ValueError(f"conformal_scale: alpha must be a number in (0, 1), got {alpha!r}")
    a = fractions.Fraction(str(alpha))
    if not 0 < a < 1:
        raise ValueError(f"conformal_scale: alpha must lie in (0, 1), got {alpha!r}")
    if N < 1:
        raise ValueError("conformal_scale: no calibration images")
    if any(c < 0 for r in rows for c in r):
        raise ValueError("conformal_scale: counts must be >= 0")
    n = [sum(r[:G + 1]) for r in rows]
    if any(v == 0 for v in n):
        raise ValueError(f"conformal_scale: image(s) {[i for i, v in enumerate(n) if v == 0]} have no valid pixel")
    if (N + 1) * a < 1:
        raise ValueError(f"conformal_scale: N = {N} calibration images cannot reach alpha = {alpha}: the bound is at least 1 / (N + 1); "
                         f"alpha = {alpha} needs at least N = {math.ceil(1 / a) - 1}")
    cum = [0] * N
    risk, found, bound = [], None, None
    for g in range(G):
        loss = fractions.Fraction(0)
        for i in range(N):
            cum[i] += rows[i][g]
            loss += 1 - fractions.Fraction(cum[i], n[i])
        risk.append(float(loss / N))
        if found is None:
            bound = (loss + 1) / (N + 1)
            if bound <= a:
                found = g
    return dict(lam=None if found is None else lams[found], g=found, alpha=alpha, N=N, bound=float(bound), risk=risk,
                reached=found is not None, invalid=sum(r[G + 1] for r in rows))


SELF_ENSEMBLES = ("flips", "dihedral")
# identity, flip W, flip H, half turn, then the same four after a transposition (bit 0 = transpose, bit 1 = flip H, bit 2 = flip W)
_DIHEDRAL_CODES = (0, 4, 2, 6, 1, 5, 3, 7)


def _self_ensemble(value):
    """the self_ensemble option: None (off), "flips" or "dihedral"; everything else -- bools, ints and other strings included -- is
    refused like solver_order's"""
    if value is None:
        return None
    if not isinstance(value, str) or value not in SELF_ENSEMBLES:
        raise ValueError(f"driftSDE: self_ensemble must be 'flips' or 'dihedral' (or None: off), got {value!r}")
    return value


def self_ensemble_codes(kind):
    """The orientation codes of a geometric self-ensemble, in member order: member s of an input runs under code codes[s % len(codes)].
    A code is 3 bits (include/idiff.h, idiff_dihedral_rows): bit 0 = transpose, bit 1 = flip H, bit 2 = flip W, the flips applied after
    the transposition.  "dihedral": [0, 4, 2, 6, 1, 5, 3, 7] -- identity, flip W, flip H, half turn, then those four after a
    transposition: the eight symmetries of the square.  "flips": the first four, which any H x W takes.  Code 0 comes first, so the
    members with s % len(codes) == 0 are the members of the option-off ensemble, and member s has the same code under both kinds while
    s % 8 < 4."""
    kind = _self_ensemble(kind)
    if kind is None:
        raise ValueError("self_ensemble_codes: kind must be 'flips' or 'dihedral'")
    return list(_DIHEDRAL_CODES[:4] if kind == "flips" else _DIHEDRAL_CODES)


def inverse_code(k):
    """the code that undoes code k: k itself without the transposition (flips are involutions that commute), and with it k with the two
    flip bits swapped (a flip of H before a transposition is a flip of W after it)"""
    if not _is_int(k) or not 0 <= k < 8:
        raise ValueError(f"inverse_code: a code is an int in [0, 8), got {k!r}")
    k = int(k)
    return k if not k & 1 else 1 | ((k & 2) << 1) | ((k & 4) >> 1)


def _max_batch(rows):
    if not _is_int(rows) or rows < 1:
        raise ValueError(f"driftSDE: max_batch must be an int >= 1, got {rows!r}")
    return int(rows)


def _max_chain_rows(rows):
    """window rows per chain of a tiled ensemble as an int >= 1; bools, floats and strings are refused like max_batch's"""
    if not _is_int(rows) or rows < 1:
        raise ValueError(f"driftSDE: max_chain_rows must be an int >= 1, got {rows!r}")
    return int(rows)


def _tiled_ensemble(flag):
    """the tiled_ensemble option as a bool (None: False); anything but a bool is refused, like reuse_graph's"""
    if flag is None:
        return False
    if not isinstance(flag, bool):
        raise ValueError(f"driftSDE: tiled_ensemble must be true or false (or None: false), got {flag!r}")
    return flag


def chain_groups(R, nwin, max_chain_rows):
    """The chains of a tiled ensemble: its R full-resolution rows, each nwin window rows in the nets, in order, as [(r0, r1), ...] with
    G = max(1, max_chain_rows // nwin) consecutive rows per chain (the last may hold fewer).  The groups cover 0..R once."""
    if not (_is_int(R) and R >= 1 and _is_int(nwin) and nwin >= 1):
        raise ValueError(f"chain_groups: R and nwin must be ints >= 1, got {R!r}, {nwin!r}")
    G = max(1, _max_chain_rows(max_chain_rows) // nwin)
    return [(r0, min(r0 + G, R)) for r0 in range(0, R, G)]


def _tile_size(tile):
    """window size of tiled sampling as (Ph, Pw), or None (off).  `tile` is an int P or a pair [Ph, Pw] of ints, each a positive multiple
    of 4; bools, floats and strings are refused like solver_order's"""
    if tile is None:
        return None
    pair = list(tile) if isinstance(tile, (list, tuple)) else [tile, tile]
    if len(pair) != 2 or not all(_is_int(p) and p >= 4 and p % 4 == 0 for p in pair):
        raise ValueError(f"driftSDE: tile must be an int P or a pair [Ph, Pw] of positive multiples of 4 (or None: off), got {tile!r}")
    return int(pair[0]), int(pair[1])


def _tile_overlap(overlap, P):
    """overlap of adjacent windows of size P along one axis: a multiple of 4 in [0, P // 2]; None: P // 8 rounded down to a multiple of 4"""
    if overlap is None:
        return (P // 8) // 4 * 4
    if not _is_int(overlap) or overlap % 4 != 0 or not 0 <= overlap <= P // 2:
        raise ValueError(f"driftSDE: tile_overlap must be an int multiple of 4 in [0, tile // 2 = {P // 2}] (or None: tile // 8), got {overlap!r}")
    return int(overlap)


def tile_axis_plan(L, P, O, align=1):
    """The windows of one axis of length L (window P, overlap O; origins rounded down to a multiple of `align`: 4 on the W axis) and
    their blend -> dict(n, P, origins, zones, first, w0, w1, cov_lo, cov_hi), the per-coordinate tables as numpy arrays of length L.
      * L <= P: one window of length L at 0.  Otherwise n = ceil((L - O) / (P - O)) windows at o_i = (i * (L - P)) // (n - 1): o_0 = 0,
        o_{n-1} = L - P, every stride in (0, P - O].
      * windows i and i+1 blend over the zone [o_{i+1}, min(o_i + P, o_{i+2})) (o_n = inf): a coordinate never has more than two windows
        with non-zero weight, and they are adjacent, also where three windows overlap physically.  At the k-th coordinate of a zone of
        length z window i+1 weighs beta = (k + 0.5) / z and window i 1 - beta, in fp64, each rounded once to fp32.
      * first[c]: the lower window with weight at c, w0 / w1 the weights of windows first and first + 1: exactly 1.0 and 0.0 outside zones.
      * cov_lo[c] <= i < cov_hi[c]: the windows whose extent [o_i, o_i + P) holds c (the scatter's targets)."""
    import numpy as np
    if not (L >= 1 and P >= 1 and 0 <= O <= P // 2 and align >= 1):
        raise ValueError(f"tile_axis_plan: bad arguments L={L}, P={P}, O={O}, align={align}")
    if L <= P:
        n, ext, origins = 1, L, [0]
    else:
        n = -((O - L) // (P - O))
        ext = P
        origins = [((i * (L - P)) // (n - 1)) // align * align for i in range(n)]
    first = np.zeros(L, dtype=np.int32)
    w0 = np.ones(L, dtype=np.float32)
    w1 = np.zeros(L, dtype=np.float32)
    zones = []
    start = 0  # where window i's sole ownership begins
    for i in range(n):
        nxt = origins[i + 1] if i + 1 < n else L
        first[start:nxt] = i
        if i + 1 == n:
            break
        end = min(origins[i] + ext, origins[i + 2] if i + 2 < n else L)
        zones.append((nxt, end))
        z = end - nxt
        if z > 0:
            beta = (np.arange(z, dtype=np.float64) + 0.5) / z
            first[nxt:end] = i
            w0[nxt:end] = (1.0 - beta).astype(np.float32)
            w1[nxt:end] = beta.astype(np.float32)
        start = end
    c = np.arange(L)
    o = np.asarray(origins)
    cov_lo = np.searchsorted(o + ext, c, side="right").astype(np.int32)  # the first window with o_i + ext > c
    cov_hi = np.searchsorted(o, c, side="right").astype(np.int32)        # the windows with o_i <= c
    # what the kernels rely on to stay inside their buffers
    assert origins[0] == 0 and origins[-1] == L - ext and all(0 < b - a <= ext for a, b in zip(origins, origins[1:])), origins
    assert all(v % align == 0 for v in origins) and ((cov_lo < cov_hi) & (cov_lo >= 0) & (cov_hi <= n)).all()
    assert ((first >= cov_lo) & (first < cov_hi)).all() and ((w1 == 0) | (first + 1 < cov_hi)).all()
    return dict(n=n, P=ext, origins=origins, zones=zones, first=first, w0=w0, w1=w1, cov_lo=cov_lo, cov_hi=cov_hi)


class TilePlan:
    """The window grid of an H x W image: `y` / `x` are tile_axis_plan's results (W origins multiples of 4), rows of the window batch run
    ((b * ny + iy) * nx + ix).  to(device) -> the same plan with the packed tables of include/idiff.h on the device:
    ytab / xtab int32 first | cov_lo | cov_hi | origin, ywt / xwt fp32 w0 | w1."""

    def __init__(self, H, W, tile, overlap):
        if W % 4:
            raise ValueError(f"tiled sampling: the image width {W} is not a multiple of 4")
        self.H, self.W = int(H), int(W)
        self.y = tile_axis_plan(self.H, tile[0], overlap[0])
        self.x = tile_axis_plan(self.W, tile[1], overlap[1], align=4)
        self.ny, self.nx, self.Ph, self.Pw = self.y["n"], self.x["n"], self.y["P"], self.x["P"]
        self.ytab = self.ywt = self.xtab = self.xwt = None

    @property
    def grid(self):
        return self.ny, self.nx, self.Ph, self.Pw

    def to(self, device):
        import numpy as np
        for ax, it, wt in ((self.y, "ytab", "ywt"), (self.x, "xtab", "xwt")):
            ints = np.concatenate([ax["first"], ax["cov_lo"], ax["cov_hi"], np.asarray(ax["origins"], dtype=np.int32)]).astype(np.int32)
            setattr(self, it, torch.from_numpy(ints).to(device).contiguous())
            setattr(self, wt, torch.from_numpy(np.concatenate([ax["w0"], ax["w1"]])).to(device).contiguous())
        return self

    def window_index(self):
        """(yy, xx) int64 [ny*nx, Ph, Pw] on the host: the full-image coordinates of every window pixel (tests, torch-side gathers)"""
        oy = torch.tensor(self.y["origins"]).repeat_interleave(self.nx)
        ox = torch.tensor(self.x["origins"]).repeat(self.ny)
        yy = (oy[:, None, None] + torch.arange(self.Ph)[None, :, None]).expand(-1, -1, self.Pw)
        xx = (ox[:, None, None] + torch.arange(self.Pw)[None, None, :]).expand(-1, self.Ph, -1)
        return yy, xx


def _jump_tables(d, n, max_sigma, T, eta, timesteps, order=1):
    """Device tables of a schedule: coef [3, T+1] fp32 holds the jump t_k -> t_{k+1} in row t_k (k < K) and NaN in every other row;
    next_t int32 [T+1] maps t_k to t_{k+1} and every other t to -1.  The expressions and their order are _step_coeffs' with t-1
    replaced by s = t_{k+1}, in fp64, rounded once to fp32: the schedule T, T-1, ..., 0 gives its tables bit for bit.
    order = 2: coef is [5, T+1]; rows 0-2 are the order-1 rows, rows 3-4 the extrapolation weights of the two clocks with p = t_{k-1}:
        rho_d = (0.5 * (d_t - d_s)) / (d_p - d_t)        rho_s = (0.5 * (sg_t - sg_s)) / (sg_p - sg_t)
    in fp64 in that order, rounded once; both 0 in row t_0 (no history), and a clock whose denominator is exactly 0 gets 0 for that
    jump (that clock alone falls back to first order)."""
    d = d.to(torch.float64)
    sg = max_sigma * torch.sqrt(n.to(torch.float64))
    coef = torch.full((3 if order == 1 else 5, T + 1), float("nan"), dtype=torch.float64)
    next_t = torch.full((T + 1,), -1, dtype=torch.int32)
    for t, s in zip(timesteps[:-1], timesteps[1:]):
        ratio = (sg[s] / sg[t]) ** 2 if sg[t] > 0 else 0.0
        et = eta * sg[s] * math.sqrt(max(1.0 - float(ratio), 0.0))
        keep = math.sqrt(max(float(sg[s]) ** 2 - et ** 2, 0.0))
        coef[0, t] = d[t] - d[s]
        coef[1, t] = sg[t] - keep
        coef[2, t] = et
        next_t[t] = s
    if order == 2:
        coef[3:, timesteps[0]] = 0.0
        for p, t, s in zip(timesteps[:-2], timesteps[1:-1], timesteps[2:]):
            for row, lv in ((3, d), (4, sg)):
                den = lv[p] - lv[t]
                coef[row, t] = (0.5 * (lv[t] - lv[s])) / den if float(den) != 0.0 else 0.0
    return coef.to(torch.float32), next_t


def _reuse_graph(flag):
    """the reuse_graph option as a bool (None: False); anything but a bool is refused"""
    if flag is None:
        return False
    if not isinstance(flag, bool):
        raise ValueError(f"driftSDE: reuse_graph must be true or false (or None: false), got {flag!r}")
    return flag


MAX_SESSIONS = 4  # held step graphs per sde; the least recently used is closed first


def session_calls0(off, off0, nper, nsteps=0):
    """state[1] at the start of an image in a held plain chain.  Its step kernel has offset_base = off0 and nper baked in and draws the
    counters off0 + state[1]*nper + v; a fresh Stepper would draw off + step*nper + v.  The two agree for state[1] = (off - off0) / nper,
    which is returned when it is exact, not negative and, with the chain's nsteps advances on top, still fits the 31 bits of the device
    word; otherwise None: the session cannot serve this stream position and a new one is captured (a draw of another size went through
    the stream in between, or the stream was rewound)."""
    diff = off - off0
    if nper < 1 or diff < 0 or diff % nper:
        return None
    q = diff // nper
    return q if q + nsteps < 1 << 31 else None


def _core(net):
    """the UNet behind a net of the sde (an EMA wrapper forwards to its ema_model)"""
    return getattr(net, "ema_model", net)


def weights_signature(modules):
    """what a held graph's packed weights and cached vectors were built from: train_ops.WEIGHT_EPOCH plus (data_ptr, _version) of every
    parameter and buffer of `modules` (objects without parameters contribute nothing).  model.load(), an optimizer step or an in-place
    edit changes it."""
    from ... import train_ops
    sig = [train_ops.WEIGHT_EPOCH[0]]
    for m in modules:
        if hasattr(m, "parameters") and hasattr(m, "buffers"):
            sig.extend((t.data_ptr(), t._version) for t in itertools.chain(m.parameters(), m.buffers()))
    return tuple(sig)


def session_key(sde, kind, rows, chw, ctx_shape, sched, order, T_stop, text_encoder, device):
    """The configuration a held step graph serves; a call reuses a session only under an equal key.  The weights signature comes last."""
    nets = (sde.drift_net, sde.noise_net)
    cores = [_core(n) for n in nets]
    smms = [m for c in cores if hasattr(c, "score_map_modules") for m in c.score_map_modules()]
    return (kind, int(rows), tuple(chw), None if ctx_shape is None else tuple(ctx_shape), None if sched is None else tuple(sched), int(order),
            int(T_stop), int(sde.seed), (sde.T, sde.max_sigma, sde.eta) + tuple(sde.schedule_names), bool(sde.two_streams), str(device),
            tuple(id(n) for n in nets) + (id(text_encoder),), tuple(getattr(c, "conv_dtype", None) for c in cores),
            weights_signature(cores + smms + [text_encoder]))


class driftSDE:
    def __init__(self, nets=None, T=100, max_sigma=0.4, drift_schedule="sigmoid", noise_schedule="sigmoid", eta=1.0, device=None,
                 sample_T=None, sample_timesteps=None, solver_order=None, num_samples=None, max_batch=16, tile=None, tile_overlap=None,
                 interval=None, reuse_graph=None, tiled_ensemble=None, max_chain_rows=128, self_ensemble=None, **_ignored):
        self.T = int(T)
        self.max_sigma = float(max_sigma)
        self.eta = float(eta)
        nets = nets or {}
        self.drift_net = nets.get("drift_net")
        self.noise_net = nets.get("noise_net")
        self.schedule_names = (str(drift_schedule), str(noise_schedule))
        self._h_drift = _level_table(self.T, drift_schedule)
        self._h_noise = _level_table(self.T, noise_schedule)
        self._a, self._b, self._c = _step_coeffs(self._h_drift, self._h_noise, self.max_sigma, self.T, self.eta)
        self.device = device
        self.drift_schedule = self._h_drift.to(device) if device is not None else self._h_drift
        self.noise_schedule = self._h_noise.to(device) if device is not None else self._h_noise
        self.seed = 0
        self._calls = 0  # draws made
        self._off = 0    # Philox counters consumed: draws of any mix of sizes use disjoint counter ranges
        self.two_streams = bool(int(os.environ.get("IDIFF_TWO_STREAMS", "1")))
        self.hip_graph = bool(int(os.environ.get("IDIFF_HIP_GRAPH", "1")))
        self._streams = None
        self._jump = None  # ((timesteps, eta, order), coef, next_t) of the last schedule whose tables were built
        self.solver_order = _solver_order(solver_order)
        self.set_sample_steps(sample_T, sample_timesteps)
        self.tiled_ensemble = _tiled_ensemble(tiled_ensemble)  # read before num_samples and tile: it decides whether the two may meet
        self.num_samples = _num_samples(num_samples)
        self.max_batch = _max_batch(max_batch)
        self.max_chain_rows = _max_chain_rows(max_chain_rows)
        self._member_base = 1  # next unassigned member id; 0 is the stream of _randn_like and the plain chain
        self.last_members = None
        self._tile = self._tile_o = None
        self._tile_plans = None  # ((H, W, tile, overlap, device), TilePlan) of the last image size planned, like _jump
        self.last_tiles = None
        self.set_tiling(tile, tile_overlap)
        self.last_order_stats = None
        self.set_interval(interval)
        self._sessions = collections.OrderedDict()  # session_key -> Session, least recently used first
        self.last_session = None  # None: the per-call path ran; 'captured' / 'replayed': a session was built / reused by the last call
        self.reuse_graph = _reuse_graph(reuse_graph)
        self.last_member_ops = None
        self.self_ensemble = _self_ensemble(self_ensemble)

    def set_self_ensemble(self, kind=None):
        """"flips" / "dihedral": the members of reverse_ddpm_ensemble run on flipped / transposed copies of the input, member s under
        self_ensemble_codes(kind)[s % len(codes)], and are turned back before they are reduced.  None: off.  Only
        reverse_ddpm_ensemble reads it; with num_samples = 1 it does nothing."""
        self.self_ensemble = _self_ensemble(kind)

    def set_reuse_graph(self, flag=None):
        """True: reverse_ddpm / reverse_ddpm_ensemble keep their captured step graph in a Session of the sde and replay it for every
        later image of the same configuration (same bits; the sde then owns the graph's memory until close_sessions()).  False / None:
        every call captures and frees its own graph, and the sessions held so far are closed."""
        self.reuse_graph = _reuse_graph(flag)
        if not self.reuse_graph:
            self.close_sessions()

    def close_sessions(self):
        """drop every held step graph with its buffers and memory pool"""
        while self._sessions:
            self._sessions.popitem(last=False)[1].close()

    def _hold_session(self, key, session):
        """keep `session` as the most recently used one; beyond MAX_SESSIONS the least recently used are closed"""
        self._sessions[key] = session
        self._sessions.move_to_end(key)
        while len(self._sessions) > MAX_SESSIONS:
            self._sessions.popitem(last=False)[1].close()

    def set_interval(self, level=None):
        """credible level L in (0, 1) of the interval maps reverse_ddpm_ensemble leaves in last_order_stats (None: off).  Only
        reverse_ddpm_ensemble reads it; with num_samples = 1 the plain chain runs and it does nothing."""
        self.interval = _interval(level)

    def set_num_samples(self, num_samples=None, max_batch=None, max_chain_rows=None):
        """S members per input for reverse_ddpm_ensemble (None / 1: off -- model.test() then runs reverse_ddpm); max_batch: rows per chain;
        max_chain_rows: window rows per chain of a tiled ensemble (chain_groups)"""
        num = _num_samples(num_samples)
        self._refuse_ensemble_of_tiles(num, getattr(self, "_tile", None))
        self.num_samples = num
        if max_batch is not None:
            self.max_batch = _max_batch(max_batch)
        if max_chain_rows is not None:
            self.max_chain_rows = _max_chain_rows(max_chain_rows)

    def set_tiled_ensemble(self, flag=None):
        """True: num_samples > 1 and a tiling may be set together, and reverse_ddpm_ensemble runs an image that exceeds the window as
        tiled member chains.  False / None: the two options refuse each other; refused while both are set."""
        flag = _tiled_ensemble(flag)
        if not flag and self.num_samples > 1 and self._tile is not None:
            raise ValueError(f"driftSDE: tiled_ensemble cannot be turned off while num_samples = {self.num_samples} and tile = "
                             f"{list(self._tile)} are both set; unset one of the two first")
        self.tiled_ensemble = flag

    def _refuse_ensemble_of_tiles(self, num_samples, tile):
        if num_samples > 1 and tile is not None and not self.tiled_ensemble:
            raise ValueError(f"driftSDE: num_samples = {num_samples} together with tile = {list(tile)} is not supported: a posterior ensemble "
                             "of a tiled chain is out of scope; unset one of the two, or set tiled_ensemble: true")

    def set_tiling(self, tile=None, overlap=None):
        """Tiled sampling: windows of `tile` = P or [Ph, Pw] pixels (multiples of 4) that overlap by `overlap` (a multiple of 4 in
        [0, P // 2] of either axis; None: P // 8 rounded down to a multiple of 4, per axis).  tile None: off, overlap must then be None
        too.  reverse_ddpm takes the tiled path for an image that exceeds the window in some axis; reverse_ddpm_tiled always does."""
        size = _tile_size(tile)
        if size is None:
            if overlap is not None:
                raise ValueError(f"driftSDE: tile_overlap = {overlap!r} without tile")
            self._tile = self._tile_o = None
            return
        over = (_tile_overlap(overlap, size[0]), _tile_overlap(overlap, size[1]))
        self._refuse_ensemble_of_tiles(self.num_samples, size)
        self._tile, self._tile_o = size, over

    @property
    def tile(self):
        """(Ph, Pw) of tiled sampling, or None"""
        return self._tile

    @property
    def tile_overlap(self):
        """(Oh, Ow), or None"""
        return self._tile_o

    def _tile_plan(self, H, W, device):
        """the device TilePlan of an H x W image under the current tiling, built once per (H, W, tile, overlap)"""
        key = (int(H), int(W), self._tile, self._tile_o, str(device))
        if self._tile_plans is None or self._tile_plans[0] != key:
            self._tile_plans = (key, TilePlan(H, W, self._tile, self._tile_o).to(device))
        return self._tile_plans[1]

    def set_solver_order(self, order=None):
        """1 (or None): the first-order jump; 2: the second-order multistep jump (reverse_ddpm only, like set_sample_steps)"""
        self.solver_order = _solver_order(order)

    def set_sample_steps(self, sample_T=None, sample_timesteps=None):
        """Reverse-chain length: sample_T = K uniform jumps, or an explicit sample_timesteps list (0 appended); neither restores the
        plain T-step chain.  Only reverse_ddpm reads it: the nets, the training sampler and the tables of the T-step chain stay."""
        sched = _sample_schedule(self.T, sample_T, sample_timesteps)
        self._sched = sched
        if sched is not None:
            self._schedule_tables(sched)

    @property
    def timesteps(self):
        """the reverse chain's timesteps t_0 = T > ... > t_K = 0 (T, T-1, ..., 0 without a few-step schedule)"""
        return list(self._sched) if self._sched is not None else list(range(self.T, -1, -1))

    def _schedule_tables(self, timesteps, order=None):
        """(coef [3, T+1] fp32 -- [5, T+1] for solver order 2 --, next_t int32 [T+1]) of a schedule, on the host; built once per
        schedule and order (order None: the sde's own)"""
        order = self.solver_order if order is None else _solver_order(order)
        key = (tuple(timesteps), self.eta, order)
        if self._jump is None or self._jump[0] != key:
            self._jump = (key,) + _jump_tables(self._h_drift, self._h_noise, self.max_sigma, self.T, self.eta, key[0], order)
        return self._jump[1], self._jump[2]

    def set_gpu(self, device):
        self.device = device
        self.drift_schedule = self._h_drift.to(device)
        self.noise_schedule = self._h_noise.to(device)

    def set_seed(self, seed):
        self.seed = int(seed)
        self._calls = 0
        self._off = 0
        self._member_base = 1

    def _randn_like(self, x):
        off = self._off
        self._calls += 1
        self._off += (x.numel() + 3) // 4
        return ops.randn(x.shape, x.device, self.seed, off)

    # ---- training-state sampler -------------------------------------------------------------------
    def forward_diffusion(self, x0, cond, t=None, eps=None):
        """-> (t [B,1,1,1] long, x_t, drift, std_noise, noise); t drawn on the host like the reference's samplers
        (utils/sde_utils.py:330-331), eps on-device unless injected."""
        x0 = x0.contiguous()
        cond = cond.contiguous()
        dev = x0.device
        B = x0.shape[0]
        if t is None:
            t = torch.randint(1, self.T + 1, (B, 1, 1, 1)).long()
        th = t.detach().cpu().reshape(-1)
        d = self._h_drift[th]
        sn = (self.max_sigma * torch.sqrt(self._h_noise[th])).to(torch.float32)
        if eps is None:
            eps = self._randn_like(x0)
        eps = eps.contiguous()
        zero = torch.zeros(B, dtype=torch.float32)
        dd, nd, sd, zd, od = d.to(dev), (-d).to(dev), sn.to(dev), zero.to(dev), (1 - d).to(dev)
        drift = ops.mix3_per_sample(cond, x0, eps, dd, nd, zd)           # d*(cond - x0)
        noise = ops.mix3_per_sample(eps, x0, cond, sd, zd, zd)           # max_sigma*sqrt(n_t)*eps
        x_t = ops.mix3_per_sample(x0, cond, eps, od, dd, sd)             # (1-d)*x0 + d*cond + s*eps
        return t.to(dev), x_t, drift, eps, noise

    # ---- sampling ---------------------------------------------------------------------------------
    def _pred(self, net, a, b, t, names, text_encoder, image_context):
        out = net(a, b, t, names, text_encoder, image_context=image_context)
        return out[0] if isinstance(out, tuple) else out

    def predict(self, xa, x, cond, tdev, names, text_encoder, image_context):
        """(R_hat, eps_hat) of one denoising step.  The two networks are independent given the state, so on a GPU they
        are enqueued on two HIP streams: each net's small late-stage kernels (32x32 levels, token chains, kernel tails)
        overlap with the other net's work instead of leaving CUs idle."""
        if not (self.two_streams and xa.is_cuda):
            return (self._pred(self.drift_net, xa, cond, tdev, names, text_encoder, image_context),
                    self._pred(self.noise_net, xa, x, tdev, names, text_encoder, image_context))
        main = torch.cuda.current_stream()
        if self._streams is None:
            self._streams = (torch.cuda.Stream(), torch.cuda.Stream())
        s1, s2 = self._streams
        s1.wait_stream(main)
        s2.wait_stream(main)
        from ..modules import MSM_degEmb_Unet as _U
        with torch.cuda.stream(s1):
            r_hat = self._pred(self.drift_net, xa, cond, tdev, names, text_encoder, image_context)
        with torch.cuda.stream(s2):
            e_hat = self._pred(self.noise_net, xa, x, tdev, names, text_encoder, image_context)
        main.wait_stream(s1)
        main.wait_stream(s2)
        if _U.SMM_SIDE:  # (experiment) a net's decoder ran on its side stream, which only the origin may join (MSM_degEmb_Unet.SMM_SIDE)
            for net in (self.drift_net, self.noise_net):
                if getattr(net, "_side_stream", None) is not None:
                    main.wait_stream(net._side_stream)
        r_hat.record_stream(main)
        e_hat.record_stream(main)
        return r_hat, e_hat

    # ---- one denoising step as a replayable unit ----------------------------------------------------
    class Stepper:
        """The body of the reverse loop with every per-step scalar in device memory (timestep vector, (a_t, b_t, c_t) tables,
        Philox call count, step index), so the same launches serve every t -- eagerly, or as ONE captured HIP graph that is
        replayed per step (`IDIFF_HIP_GRAPH=0` disables the capture).  The graph holds the two UNet forwards on their two
        streams, the fused update and the state advance; the host does not touch the loop between replays.
        `timesteps` (a few-step schedule t_0 > ... > t_K = 0) swaps in the schedule's jump tables and the table-driven state advance;
        without it the plain t -> t-1 chain runs.  `solver_order` = 2 (needs `timesteps`) swaps in the second-order update, its
        5-row table and the two history buffers it keeps between replays.
        `members` (int64 [rows] on the device, ops.member_ids) swaps in the member step: row r draws its z from member members[r]'s own
        stream, and the run consumes none of the sde's stream (`_off`, `_calls` stay).  `xa` hands in an x - cond already formed
        (ops.ensemble_init)."""

        def __init__(self, sde, x, cond, names, text_encoder, image_context, noises=None, t_start=None, t_stop=0, timesteps=None,
                     solver_order=1, members=None, xa=None):
            self.sde, self.names, self.text_encoder, self.ctx = sde, names, text_encoder, image_context
            dev = x.device
            self.x, self.cond = x, cond
            self.members = members
            self.xa = ops.axpby(x, cond, 1.0, -1.0) if xa is None else xa
            self.T, self.t_stop = sde.T, int(t_stop)
            self.order = _solver_order(solver_order)
            if self.order == 2 and timesteps is None:
                raise ValueError("Stepper: solver_order = 2 runs on a schedule (timesteps)")
            if timesteps is None:
                self.next_t = None
                t0 = sde.T if t_start is None else int(t_start)
                self.coef = torch.stack([sde._a, sde._b, sde._c]).to(device=dev, dtype=torch.float32).contiguous()
            else:
                ts = list(timesteps)
                if t_start is not None or len(ts) < 2 or ts[-1] != 0 or ts[0] > sde.T or any(a <= b for a, b in zip(ts, ts[1:])):
                    raise ValueError(f"Stepper: timesteps must decrease strictly from at most T={sde.T} to 0 (no t_start), got {ts}")
                t0 = self.t_first = ts[0]
                coef, next_t = sde._schedule_tables(ts, self.order)
                self.coef = coef.to(dev).contiguous()
                self.next_t = next_t.to(dev).contiguous()
            self.tdev = torch.full((x.shape[0],), float(t0), dtype=torch.float32, device=dev)
            self.state = torch.tensor([t0, 0, 0], dtype=torch.int32, device=dev)  # {t, draws of this run, step index}
            self.noises = None if noises is None else noises.contiguous()
            self.nper = (x.numel() + 3) // 4
            self.off_base = sde._off  # this run's draws start where the stream's earlier ones ended
            self.graph = None
            self.steps_done = 0
            # order 2: the previous jump's predictions; not read at t_0, whose rho rows are 0
            self.r_prev, self.e_prev = (torch.empty_like(x), torch.empty_like(x)) if self.order == 2 else (None, None)

        def _body(self):
            self._update(*self._predict())
            self._advance()

        def _predict(self):
            return self.sde.predict(self.xa, self.x, self.cond, self.tdev, self.names, self.text_encoder, self.ctx)

        def _update(self, r_hat, e_hat):
            """the fused update of x / xa from this step's predictions: the member, second-order or plain step"""
            seed = self.sde.seed
            if self.members is not None:
                ops.drift_reverse_step_members_dev(self.x, r_hat, e_hat, self.r_prev, self.e_prev, self.noises, self.cond, self.xa, self.coef,
                                                   self.state, self.members, seed)
            elif self.order == 2:
                ops.drift_reverse_step2_dev(self.x, r_hat, e_hat, self.r_prev, self.e_prev, self.noises, self.cond, self.xa, self.coef, self.state,
                                            seed, self.nper, self.off_base)
            else:
                ops.drift_reverse_step_dev(self.x, r_hat, e_hat, self.noises, self.cond, self.xa, self.coef, self.state, seed, self.nper, self.off_base)

        def _advance(self):
            if self.next_t is None:
                ops.step_state_advance(self.state, self.tdev, self.T, self.t_stop)
            else:
                ops.step_state_advance_table(self.state, self.tdev, self.next_t, self.t_first, self.t_stop)

        def _warm_step(self):
            """one step eagerly on the side stream: fills every weight / text cache outside the graph's memory pool.  It IS a
            denoising step (x, xa and the device state {t, Philox count, step index} advance), whatever happens to the capture."""
            main = torch.cuda.current_stream()
            self.stream = torch.cuda.Stream()
            self.stream.wait_stream(main)
            with torch.cuda.stream(self.stream):
                self._body()
            main.wait_stream(self.stream)

        def _capture(self):
            """capture the next step as a HIP graph (enqueues nothing that executes)"""
            main = torch.cuda.current_stream()
            self.stream.wait_stream(main)
            with torch.cuda.stream(self.stream):
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # thread-local capture mode: a polling thread of the process (e.g. the RCCL watchdog of a multi-GPU job) must
                # not invalidate the capture
                with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
                    self._body()
            main.wait_stream(self.stream)
            return g

        @torch.no_grad()
        def prepare(self):
            """Warm step + graph capture; returns the number of denoising steps it executed (1, counted in steps_done, also when
            the capture then fails and the loop stays eager); 0 when capture is off or already attempted."""
            sde = self.sde
            if not (sde.hip_graph and self.x.is_cuda and self.graph is None):
                return 0
            self._warm_step()
            self.steps_done += 1
            self._account(1)
            try:
                self.graph = self._capture()
            except Exception as e:  # stay on the eager HIP path (same kernels), say why once
                self.graph = False
                print(f"[instancediff_amd] HIP graph capture unavailable ({e!r}); running the step eagerly")
            return 1

        @torch.no_grad()
        def run(self, nsteps):
            sde = self.sde
            nsteps -= self.prepare() if nsteps >= 3 else 0
            if self.graph:
                main = torch.cuda.current_stream()
                self.stream.wait_stream(main)
                with torch.cuda.stream(self.stream):
                    for _ in range(nsteps):
                        self.graph.replay()
                main.wait_stream(self.stream)
            else:
                for _ in range(nsteps):
                    self._body()
            self.steps_done += nsteps
            self._account(nsteps)
            return self.x

        def _account(self, nsteps):
            """the sde's Philox accounting of nsteps steps; member runs draw from their own streams and leave it alone"""
            if self.members is None:
                self.sde._calls += nsteps
                self.sde._off += nsteps * self.nper

        @property
        def mode(self):
            """'graph' when the loop replays a captured HIP graph, 'eager' otherwise (reported by bench.py)"""
            return "graph" if self.graph else "eager"

    class TiledStepper(Stepper):
        """Stepper for tiled sampling: x / cond are the full image, `plan` its device TilePlan; names and image_context come in per window
        row.  A step runs predict on chunks of at most sde.max_batch window rows, lands the chunks' predictions in the persistent r_tiles /
        e_tiles (one chunk: the nets' outputs are used as they are), then the fused tiled step on the full image -- which also rewrites
        the window inputs x_tiles / xa_tiles -- and the state advance over all window rows.  Warm step, capture, replay and the Philox
        accounting (nper = the FULL image's float4 count, as the plain chain's) are Stepper's.
        `members` (int64 [rows of x] on the device) makes x the full-resolution rows of an ensemble: row r draws its z from member
        members[r]'s stream as in the untiled member chain, whatever the tiling, and the sde's stream is left alone; `xa` hands in the
        full-resolution x - cond (ops.ensemble_init)."""

        def __init__(self, sde, x, cond, plan, names, text_encoder, image_context, **kw):
            super().__init__(sde, x, cond, names, text_encoder, image_context, **kw)
            if self.members is not None and (self.members.dim() != 1 or self.members.numel() != x.shape[0]):
                raise ValueError(f"TiledStepper: members must hold one id per full-resolution row ({x.shape[0]})")
            self.plan = plan
            R = x.shape[0] * plan.ny * plan.nx
            if len(names) != R or (image_context is not None and image_context.shape[0] != R):
                raise ValueError(f"TiledStepper: names / image_context must come per window row ({R})")
            self.tdev = torch.full((R,), float(self.state[0].item()), dtype=torch.float32, device=x.device)
            self.cond_tiles = ops.tile_gather(cond, plan)
            self.x_tiles = ops.tile_gather(x, plan)
            self.xa_tiles = ops.tile_gather(self.xa, plan)
            self.chunks = []
            for r0 in range(0, R, sde.max_batch):
                r1 = min(r0 + sde.max_batch, R)
                self.chunks.append((r0, r1, list(names[r0:r1]), None if image_context is None else image_context[r0:r1].contiguous()))
            if len(self.chunks) > 1:
                self.r_tiles, self.e_tiles = torch.empty_like(self.x_tiles), torch.empty_like(self.x_tiles)

        def _predict(self):
            for r0, r1, names, ctx in self.chunks:
                r_hat, e_hat = self.sde.predict(self.xa_tiles[r0:r1], self.x_tiles[r0:r1], self.cond_tiles[r0:r1], self.tdev[r0:r1], names,
                                                self.text_encoder, ctx)
                if len(self.chunks) == 1:
                    return r_hat, e_hat
                # 1*r + 0*r: a copy by a library launch, into the rows the step reads
                ops.axpby(r_hat, r_hat, 1.0, 0.0, out=self.r_tiles[r0:r1])
                ops.axpby(e_hat, e_hat, 1.0, 0.0, out=self.e_tiles[r0:r1])
            return self.r_tiles, self.e_tiles

        def _update(self, r_tiles, e_tiles):
            if self.members is not None:
                ops.drift_reverse_step_tiled_members_dev(self.x, r_tiles, e_tiles, self.r_prev, self.e_prev, self.noises, self.cond, self.x_tiles,
                                                         self.xa_tiles, self.plan, self.coef, self.state, self.members, self.sde.seed)
                return
            ops.drift_reverse_step_tiled_dev(self.x, r_tiles, e_tiles, self.r_prev, self.e_prev, self.noises, self.cond, self.x_tiles,
                                             self.xa_tiles, self.plan, self.coef, self.state, self.sde.seed, self.nper, self.off_base)

    class Session:
        """A captured step graph that outlives the call: the buffers it is baked on, ONE ordinary Stepper over them, and strong
        references to every tensor the graph reads without owning.
          * x, xa, cond [rows, C, H, W], the context buffer, the int32 class-index buffer the nets take as `names` and, for a member
            chain, the int64 member buffer are refilled per image by library launches and a few bytes of host-to-device copy.
          * `held`: the nets' cache values after the warm step (MSM_degEmb_Unet.held_cache_values).  Several of those caches hold one
            value and replace it when a call of another batch size or context comes through; the graph holds addresses.
          * `vecs`: the single-token context vectors of the warm step.  The library refills the context buffer through raw pointers,
            so the nets' cache key (ctx._version, identity) cannot see it: begin() recomputes every vector and copies it into the
            tensor the graph reads.
        start() serves the first image (warm step and capture, Stepper.prepare), begin() every later one; the caller then runs
        stepper.run() and copies x out, since x belongs to the next image."""

        def __init__(self, sde, key, rows, cond, image_context, members):
            # the sde owns its sessions, so the session and its Stepper see the sde through a weak proxy: no reference cycle, and an
            # sde that is dropped frees its graphs at once by reference count -- never at some later garbage collection, which
            # could fall inside another chain's graph capture
            self.sde, self.key = weakref.proxy(sde), key
            dev = cond.device
            shape = (rows,) + tuple(cond.shape[1:])
            self.x, self.xa, self.cond = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3))
            self.ctx = None if image_context is None else torch.empty((rows,) + tuple(image_context.shape[1:]), dtype=torch.float32, device=dev)
            self.idx = torch.zeros(rows, dtype=torch.int32, device=dev)
            self.members = torch.ones(rows, dtype=torch.int64, device=dev) if members else None
            self.stepper = None
            self.held, self.vecs = [], []

        def _fill(self, cond, idx, image_context, members, offset, calls0, S, row0):
            """this image's inputs into the buffers; the chain's start and device state in one launch"""
            st, sde = self.stepper, self.sde
            self.idx.copy_(torch.tensor(idx, dtype=torch.int32))
            if self.members is not None:
                self.members.copy_(torch.tensor(members, dtype=torch.int64))
            if self.ctx is not None:
                ops.axpby(image_context, image_context, 1.0, 0.0, out=self.ctx)
            ops.chain_begin(cond, self.cond, self.x, self.xa, st.state, st.tdev, sde.max_sigma, sde.seed, offset=offset,
                            t0=st.t_first if st.next_t is not None else st.T, calls0=calls0, members=self.members, S=S, row0=row0)

        def start(self, cond, idx, image_context, text_encoder, sched, order, T_stop, members=None, offset=0, S=1, row0=0):
            """the first image: the Stepper on the buffers, the fill, then warm step and capture -> the steps executed (1)"""
            self.stepper = driftSDE.Stepper(self.sde, self.x, self.cond, self.idx, text_encoder, self.ctx, t_stop=T_stop, timesteps=sched,
                                            solver_order=order, members=self.members, xa=self.xa)
            self._fill(cond, idx, image_context, members, offset, 0, S, row0)
            done = self.stepper.prepare()
            if self.stepper.graph:
                for net in (self.sde.drift_net, self.sde.noise_net):
                    core = _core(net)
                    self.held.extend(core.held_cache_values())
                    c = core._ctx_cache
                    if self.ctx is not None and c is not None and c[2]() is self.ctx:
                        self.vecs.extend((ca, c[1][id(ca)]) for ca in core.cross_attns())
                self.held.append(text_encoder)
            return done

        def begin(self, cond, idx, image_context, members=None, offset=0, calls0=0, S=1, row0=0):
            """a later image: refill the buffers, rewind the device state, refresh the context vectors the graph reads"""
            self._fill(cond, idx, image_context, members, offset, calls0, S, row0)
            for ca, held in self.vecs:
                fresh = ca.single_token_vec(self.ctx)
                ops.axpby(fresh, fresh, 1.0, 0.0, out=held)

        def close(self):
            self.stepper = self.x = self.xa = self.cond = self.ctx = self.idx = self.members = None
            self.held, self.vecs = [], []

    def _session_indices(self, names, cond, image_context, nsteps):
        """the class indices of `names` when a session may serve the call, else None (the per-call path runs): reuse_graph on, a chain
        that would capture (HIP graphs on, device tensors, at least 3 steps), fp32 inputs, and both nets UNets of this package in eval
        mode that agree on the indices"""
        if not (self.reuse_graph and self.hip_graph and cond.is_cuda and nsteps >= 3 and cond.dtype == torch.float32):
            return None
        if image_context is not None and (image_context.dtype != torch.float32 or image_context.device != cond.device):
            return None
        cores = [_core(self.drift_net), _core(self.noise_net)]
        if not all(hasattr(c, "held_cache_values") and hasattr(c, "type_map_ind") and not getattr(c, "training", False) for c in cores):
            return None
        if torch.is_tensor(names) or any(n not in c.type_map_ind for c in cores for n in names):
            return None
        idx = [cores[0].type_map_ind[n] for n in names]
        return idx if idx == [cores[1].type_map_ind[n] for n in names] else None

    def _session_run(self, kind, cond, idx, text_encoder, image_context, sched, nsteps, order, T_stop, rows, members=None, S=1, row0=0):
        """One chain of `rows` rows through a held session -> (the session's x -- which the next image overwrites --, its stepper,
        'captured' | 'replayed'), or through a session that failed to capture and is dropped -> (x, stepper, None).  A plain chain's
        x_T draw keeps the per-call accounting: one draw of the batch's size at the stream's position."""
        key = session_key(self, kind, rows, cond.shape[1:], None if image_context is None else image_context.shape[1:], sched, order, T_stop,
                          text_encoder, cond.device)
        offset = nper = 0
        if kind == "plain":
            nper = (cond.numel() + 3) // 4
            offset = self._off
            self._calls += 1
            self._off += nper
        ses = self._sessions.get(key)
        calls0 = 0
        if ses is not None and kind == "plain":
            calls0 = session_calls0(self._off, ses.stepper.off_base, nper, nsteps)
            if calls0 is None:
                self._sessions.pop(key).close()
                ses = None
        if ses is not None:
            self._sessions.move_to_end(key)
            ses.begin(cond, idx, image_context, members=members, offset=offset, calls0=calls0, S=S, row0=row0)
            ses.stepper.run(nsteps)
            return ses.x, ses.stepper, "replayed"
        for stale in [k for k in self._sessions if k[:-1] == key[:-1]]:  # the same configuration on weights that have changed since
            self._sessions.pop(stale).close()
        ses = driftSDE.Session(self, key, rows, cond, image_context, kind == "member")
        done = ses.start(cond, idx, image_context, text_encoder, sched, order, T_stop, members=members, offset=offset, S=S, row0=row0)
        ses.stepper.run(nsteps - done)
        if not ses.stepper.graph:
            return ses.x, ses.stepper, None
        self._hold_session(key, ses)
        return ses.x, ses.stepper, "captured"

    def _chain_plan(self, reverse_type, optimize_type, noises, T_stop, who="reverse_ddpm"):
        """-> (schedule or None, steps, solver order) of a reverse chain down to T_stop, after the option checks"""
        if optimize_type not in ("inputRes", "predict_noise", ""):
            raise NotImplementedError(f"optimize_type={optimize_type!r}: only the active 'inputRes' path of the reference "
                                      "(drift_noise_model.py:231-232) is in scope")
        if "std" not in str(reverse_type):
            # optimize_target (drift_noise_model.py:68,581-604): 'std*' nets predict LQ-GT and the standard noise, which is what
            # the update consumes; 'scaled*' nets predict d_t*(LQ-GT) and s_t*eps and would need rescaling -- not silently ignored
            raise NotImplementedError(f"reverse_type={reverse_type!r}: only the 'std' prediction targets of config.yml:144 are in scope")
        order = self.solver_order
        sched = self._sched if (self._sched is not None or order == 1) else self.timesteps
        if sched is not None:
            if T_stop not in sched:
                raise ValueError(f"{who}: T_stop={T_stop} is not a point of the schedule {sched}")
            nsteps = sched.index(T_stop)
            if noises is not None and noises.shape[0] < nsteps:
                raise ValueError(f"{who}: noises holds {noises.shape[0]} draws for a {nsteps}-step chain")
        else:
            nsteps = self.T - T_stop
        return sched, nsteps, order

    def _start_state(self, cond, x_T):
        """a private copy of x_T, drawn as cond + max_sigma*z from the sde's stream when none is given"""
        if x_T is None:
            x_T = ops.axpby(cond, self._randn_like(cond), 1.0, self.max_sigma)
        return x_T.contiguous().clone()

    def _record_run(self, stepper, nsteps, order):
        self.last_mode = stepper.mode  # 'graph' | 'eager': how the loop of this call ran
        self.last_steps = nsteps
        self.last_solver_order = order

    @torch.no_grad()
    def reverse_ddpm(self, cond, names, text_encoder, reverse_type="std", optimize_type="inputRes", image_context=None, x_T=None,
                     noises=None, T_stop=0):
        """Iterative denoising from x_T = cond + max_sigma*z down to t=1.  `noises` (optional, [T, ...]) injects
        the per-step draws (parity runs; noises[i] is used at loop iteration i, t = T-i); x_T optional.
        With a few-step schedule (sample_T / sample_timesteps) the loop runs K = len(timesteps) - 1 jumps t_k -> t_{k+1}, noises is
        [K, ...] indexed by step and T_stop must be 0 or a schedule point.  self.last_steps: the steps this call ran.
        solver_order = 2 always runs the schedule path (T, T-1, ..., 0 when no schedule is set).  self.last_solver_order: the order that ran."""
        if self._tile is not None and cond.dim() == 4 and (cond.shape[2] > self._tile[0] or cond.shape[3] > self._tile[1]):
            return self.reverse_ddpm_tiled(cond, names, text_encoder, reverse_type=reverse_type, optimize_type=optimize_type,
                                           image_context=image_context, x_T=x_T, noises=noises, T_stop=T_stop)
        sched, nsteps, order = self._chain_plan(reverse_type, optimize_type, noises, T_stop)
        cond = cond.contiguous()
        self.last_tiles = None
        self.last_session = None
        idx = self._session_indices(names, cond, image_context, nsteps) if (x_T is None and noises is None) else None
        if idx is not None:
            ctx = None if image_context is None else image_context.contiguous()
            x, stepper, self.last_session = self._session_run("plain", cond, idx, text_encoder, ctx, sched, nsteps, order, T_stop, cond.shape[0])
            self._record_run(stepper, nsteps, order)
            return ops.axpby(x, x, 1.0, 0.0)  # a copy by a library launch: the session's x is the next image's
        x = self._start_state(cond, x_T)
        stepper = driftSDE.Stepper(self, x, cond, names, text_encoder, image_context, noises=noises, t_stop=T_stop, timesteps=sched,
                                   solver_order=order)
        out = stepper.run(nsteps)
        self._record_run(stepper, nsteps, order)
        return out

    @torch.no_grad()
    def reverse_ddpm_tiled(self, cond, names, text_encoder, reverse_type="std", optimize_type="inputRes", image_context=None, x_T=None,
                           noises=None, T_stop=0):
        """reverse_ddpm on the window grid of set_tiling, whatever the image size (a single window included).  cond, x_T, noises and the
        result are full images ([B, C, H, W], W a multiple of 4); the schedule, solver order, eta, T_stop, the x_T draw and the Philox
        accounting are reverse_ddpm's for that image, and with on-device noise every pixel gets the z the plain chain would give it.
        `names` and `image_context` are repeated per window: the whole image's embedding serves each of its windows.  The window rows
        run through the nets in chunks of at most max_batch.  self.last_tiles: the grid that ran, (ny, nx, Ph, Pw)."""
        if self._tile is None:
            raise ValueError("reverse_ddpm_tiled: no tiling is set (set_tiling / the tile option)")
        self._refuse_ensemble_of_tiles(self.num_samples, self._tile)
        sched, nsteps, order = self._chain_plan(reverse_type, optimize_type, noises, T_stop, who="reverse_ddpm_tiled")
        cond = cond.contiguous()
        if cond.dim() != 4:
            raise ValueError(f"reverse_ddpm_tiled: cond must be [B, C, H, W], got {tuple(cond.shape)}")
        B, _, H, W = cond.shape
        if W % 4:
            raise ValueError(f"reverse_ddpm_tiled: the image width {W} is not a multiple of 4")
        plan = self._tile_plan(H, W, cond.device)
        self.last_session = None  # a tiled chain always captures per call
        x = self._start_state(cond, x_T)
        nwin = plan.ny * plan.nx
        names_rep = [n for n in names for _ in range(nwin)]
        ctx_rep = None if image_context is None else image_context.repeat_interleave(nwin, dim=0)
        stepper = driftSDE.TiledStepper(self, x, cond, plan, names_rep, text_encoder, ctx_rep, noises=noises, t_stop=T_stop, timesteps=sched,
                                        solver_order=order)
        out = stepper.run(nsteps)
        self._record_run(stepper, nsteps, order)
        self.last_tiles = plan.grid
        return out

    def _assign_members(self, B, S, members):
        """ids of the B*S rows (row b*S + s): explicit `members` ([B*S] or [B, S] ints >= 1, no duplicates) or the next B*S of the
        sde's counter, which starts at 1, is reset by set_seed and is left alone by explicit ids"""
        if members is None:
            ids = list(range(self._member_base, self._member_base + B * S))
            self._member_base += B * S
            return ids
        ids = torch.as_tensor(members).reshape(-1).tolist()
        if len(ids) != B * S or any(not isinstance(m, int) or isinstance(m, bool) or m < 1 for m in ids) or len(set(ids)) != len(ids):
            raise ValueError(f"reverse_ddpm_ensemble: members must be {B * S} distinct ints >= 1 (0 is the sde's own stream), got {ids}")
        return ids

    @torch.no_grad()
    def reverse_ddpm_ensemble(self, cond, names, text_encoder, reverse_type="std", optimize_type="inputRes", image_context=None,
                              num_samples=None, members=None, noises=None, T_stop=0, return_samples=False):
        """S posterior samples per input row as one batched chain -> (mean [B, ...], std [B, ...][, samples [B, S, ...]]).
        Row b*S + s is member m(b, s), whose x_T draw and per-step z come from its own Philox stream (include/idiff.h): its image is the
        same in any batch, chunking or call order.  The B*S rows run in chunks of at most max_batch rows, each through a Stepper of its
        own (schedule, solver_order, warm step, capture and T_stop as in reverse_ddpm), and are reduced on the device.  `noises`
        ([steps, B*S, ...]) injects the per-step draws.  self.last_members: the ids used, [B, S].
        With `interval` = L set, self.last_order_stats = dict(lo, hi, median [B, ...], level, nominal, ks): the order statistics of
        order_stat_indices(S, L) as contiguous maps, from one ops.ensemble_order_stats launch over the samples (plus one axpby for the
        median of an even S, and for B > 1 one ops.gather_channel per map); None without it.
        With `tiled_ensemble` on and a tiling set, an image that exceeds the window in some axis (reverse_ddpm's rule; W a multiple of 4)
        runs as tiled member chains: the rows start at full resolution (ops.ensemble_init), are grouped in order by chain_groups(B*S,
        ny*nx, max_chain_rows), and each group is one TiledStepper over its rows.  A member's noise is the untiled chain's, so neither
        the tiling nor the grouping changes which z a pixel gets.  self.last_tiles: the grid (None on the untiled path); reuse_graph
        does not apply (a tiled chain captures per call).
        With `self_ensemble` = "flips" / "dihedral" and S > 1 (cond [B, C, H, W], W a multiple of 4, H == W for "dihedral"), member s
        runs on the input turned by code self_ensemble_codes(kind)[s % len(codes)]: one ops.dihedral_rows launch writes the B*S turned
        rows, which run through the row machinery above as B*S inputs of one member each (same ids, names and context -- an embedding has
        no orientation; a tiled ensemble turns the full-resolution rows, not the windows; a session's chain_begin takes the turned rows
        with S = 1), and one more launch with the inverse codes turns every member back before samples, mean, std, the order statistics
        and score_ensemble see it.  Both launches stay outside the captured graphs.  self.last_member_ops: the codes used, int64
        [B, S]; None with the option off or S = 1, when nothing above changes.  `noises` is injected as is, in the rows' own (turned)
        frame.  Then:
          * row (b, s) is bit-equal to a one-member call (num_samples = 1, members = [m(b, s)], option off) on the turned cond[b],
            turned back;
          * members with code 0 are bit-equal to the same members with the option off;
          * a member's image still does not depend on batch, chunking, grouping or graph reuse;
          * the spread now also holds the nets' orientation dependence: a different ensemble from the option-off one, not a reduced one."""
        S = self.num_samples if num_samples is None else _num_samples(num_samples)
        self._refuse_ensemble_of_tiles(S, self._tile)
        codes = self_ensemble_codes(self.self_ensemble) if (self.self_ensemble is not None and S > 1) else None
        if codes is not None:  # refused here, before anything is launched
            if cond.dim() != 4:
                raise ValueError(f"reverse_ddpm_ensemble: self_ensemble needs cond as [B, C, H, W], got {tuple(cond.shape)}")
            if cond.shape[3] % 4:
                raise ValueError(f"reverse_ddpm_ensemble: self_ensemble needs an image width that is a multiple of 4, got {cond.shape[3]}")
            if any(k & 1 for k in codes) and cond.shape[2] != cond.shape[3]:
                raise ValueError(f"reverse_ddpm_ensemble: self_ensemble = {self.self_ensemble!r} transposes and needs a square image, got "
                                 f"{cond.shape[2]} x {cond.shape[3]} ('flips' takes any H x W)")
        sched, nsteps, order = self._chain_plan(reverse_type, optimize_type, noises, T_stop, who="reverse_ddpm_ensemble")
        cond = cond.contiguous()
        B = cond.shape[0]
        R = B * S
        # reverse_ddpm's rule: with the switch on, an image that exceeds the window in some axis runs as tiled member chains
        tiled = (self.tiled_ensemble and self._tile is not None and cond.dim() == 4
                 and (cond.shape[2] > self._tile[0] or cond.shape[3] > self._tile[1]))
        if tiled and cond.shape[3] % 4:
            raise ValueError(f"reverse_ddpm_ensemble: the image width {cond.shape[3]} is not a multiple of 4")
        if (cond.numel() // B) % 4:
            raise ValueError(f"reverse_ddpm_ensemble: a sample has {cond.numel() // B} elements, not a multiple of 4")
        if noises is not None and (noises.dim() < 2 or noises.shape[1] != R):
            raise ValueError(f"reverse_ddpm_ensemble: noises must be [steps, B*S = {R}, ...], got {tuple(noises.shape)}")
        ids = self._assign_members(B, S, members)
        mdev = ops.member_ids(ids, cond.device)
        names_rep = [n for n in names for _ in range(S)]
        ctx_rep = None if image_context is None else image_context.repeat_interleave(S, dim=0)
        self.last_session = None
        self.last_tiles = None
        self.last_member_ops = None
        # rows_in / S_in: what the row machinery below expands to the B*S rows -- the B inputs, S members each, or with a self-ensemble the
        # B*S inputs already turned, one member each
        rows_in, S_in = cond, S
        if codes is not None:
            rows_in, S_in = ops.dihedral_rows(cond, codes, S=S, in_rep=S), 1
        idx = self._session_indices(names_rep, cond, image_context, nsteps) if (noises is None and not tiled) else None
        if tiled:
            # chains of G consecutive full-resolution rows, each one TiledStepper over its G*nwin window rows; a tiled chain always
            # captures per call
            plan = self._tile_plan(cond.shape[2], cond.shape[3], cond.device)
            nwin = plan.ny * plan.nx
            cond_rep, x, xa = ops.ensemble_init(rows_in, S_in, mdev, self.max_sigma, self.seed)
            for r0, r1 in chain_groups(R, nwin, self.max_chain_rows):
                stepper = driftSDE.TiledStepper(self, x[r0:r1], cond_rep[r0:r1], plan, [n for n in names_rep[r0:r1] for _ in range(nwin)],
                                                text_encoder, None if ctx_rep is None else ctx_rep[r0:r1].repeat_interleave(nwin, dim=0),
                                                noises=None if noises is None else noises[:, r0:r1].contiguous(), t_stop=T_stop,
                                                timesteps=sched, solver_order=order, members=mdev[r0:r1], xa=xa[r0:r1])
                stepper.run(nsteps)
            self.last_tiles = plan.grid
        elif idx is not None:
            # each chunk through the member session of its row count: a full chunk and a shorter last chunk are two sessions
            x = torch.empty((R,) + tuple(cond.shape[1:]), dtype=torch.float32, device=cond.device)
            how = []
            for r0 in range(0, R, self.max_batch):
                r1 = min(r0 + self.max_batch, R)
                rows, stepper, state = self._session_run("member", rows_in, idx[r0:r1], text_encoder, None if ctx_rep is None else ctx_rep[r0:r1],
                                                         sched, nsteps, order, T_stop, r1 - r0, members=ids[r0:r1], S=S_in, row0=r0)
                ops.axpby(rows, rows, 1.0, 0.0, out=x[r0:r1])
                how.append(state)
            self.last_session = None if None in how else ("captured" if "captured" in how else "replayed")
        else:
            cond_rep, x, xa = ops.ensemble_init(rows_in, S_in, mdev, self.max_sigma, self.seed)
            for r0 in range(0, R, self.max_batch):
                r1 = min(r0 + self.max_batch, R)
                stepper = driftSDE.Stepper(self, x[r0:r1], cond_rep[r0:r1], names_rep[r0:r1], text_encoder,
                                           None if ctx_rep is None else ctx_rep[r0:r1].contiguous(),
                                           noises=None if noises is None else noises[:, r0:r1].contiguous(), t_stop=T_stop, timesteps=sched,
                                           solver_order=order, members=mdev[r0:r1], xa=xa[r0:r1])
                stepper.run(nsteps)
        self._record_run(stepper, nsteps, order)
        self.last_members = torch.tensor(ids, dtype=torch.int64).view(B, S)
        if codes is not None:  # every member back into the input's frame, outside the captured graphs
            x = ops.dihedral_rows(x, [inverse_code(k) for k in codes], S=S)
            self.last_member_ops = torch.tensor([codes[s % len(codes)] for s in range(S)] * B, dtype=torch.int64).view(B, S)
        samples = x.view((B, S) + tuple(cond.shape[1:]))
        mean, std = ops.ensemble_stats(samples)
        self.last_order_stats = None if self.interval is None else self._order_stats(samples, self.interval)
        return (mean, std, samples) if return_samples else (mean, std)

    @staticmethod
    def score_ensemble(samples, target, want_map=False):
        """Ensemble scores of samples [B, S, ...] (reverse_ddpm_ensemble(..., return_samples=True)) against target [B, ...] ->
        (sums float64 [B, 3], counts int32 [B, S + 2], crps_map [B, ...] or None) on the device, from one ops.ensemble_scores call (two
        launches, no host copy); ensemble_score_summary(sums, counts, S) reads CRPS / SSR / RANK_DEV / OUTLIERS off them."""
        if not torch.is_tensor(samples) or samples.dim() < 3:
            raise ValueError("score_ensemble: samples must be a [B, S, ...] tensor (reverse_ddpm_ensemble(..., return_samples=True))")
        if not torch.is_tensor(target) or tuple(target.shape) != (samples.shape[0],) + tuple(samples.shape[2:]):
            raise ValueError(f"score_ensemble: target must be [B, ...] = {(samples.shape[0],) + tuple(samples.shape[2:])}, got "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        return ops.ensemble_scores(samples.contiguous(), target.contiguous(), want_map=want_map)

    @staticmethod
    def region_scores(samples_or_output, target, labels, L):
        """The ensemble-scores record per region of a uint8 label map: samples [B, S, ...] (or one restoration [B, ...], S = 1) against
        target [B, ...], labels [B, ...] or one shared [...] -> (sums float64 [B, L, 4], counts int32 [B, L, S + 2], outside int32 [B]) on
        the device, from one ops.region_scores call (two launches, no host copy); region_score_summary(sums, counts, outside, S) reads
        the per-region CRPS / RMSE / PSNR / BIAS / SSR / RANK_DEV / OUTLIERS and the error shares off them."""
        x = samples_or_output
        if not torch.is_tensor(target) or target.dim() < 2:
            raise ValueError("region_scores: target must be a [B, ...] tensor")
        want = (tuple(target.shape), tuple(target.shape[:1]) + (x.shape[1] if torch.is_tensor(x) and x.dim() > 1 else 0,) + tuple(target.shape[1:]))
        if not torch.is_tensor(x) or tuple(x.shape) not in want:
            raise ValueError(f"region_scores: samples must be [B, S, ...] or [B, ...] for target {tuple(target.shape)}, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) not in (tuple(target.shape), tuple(target.shape[1:])):
            raise ValueError(f"region_scores: labels must be a uint8 tensor of shape {tuple(target.shape)} or {tuple(target.shape[1:])}")
        return ops.region_scores(x.contiguous(), target.contiguous(), labels.contiguous(), L)

    @staticmethod
    def despeckle_stats(samples_or_output, ref, labels, L):
        """The sums behind the no-reference despeckling statistics per region of a uint8 label map: samples [B, S, C, H, W] (or one
        restoration [B, C, H, W], S = 1) against ref [B, C, H, W] (the noisy input, or the target), labels [B, C, H, W] or one shared
        [C, H, W] -> (sums float64 [B, S, L, 12], counts int32 [B, S, L, 4], outside int32 [B]) on the device, from one
        ops.despeckle_stats call (two launches, no host copy) on the [0, 1] intensity scale; despeckle_summary(sums, counts, outside) reads
        ENL / SSI / SMPI / MEAN_RATIO / VAR_RATIO / EPI / LAP_RATIO / CNR off them, homogeneous_cells(sums, counts) the ENL of the most
        homogeneous cells of a grid."""
        x = samples_or_output
        if not torch.is_tensor(ref) or ref.dim() != 4:
            raise ValueError("despeckle_stats: ref must be a [B, C, H, W] tensor")
        want = (tuple(ref.shape), tuple(ref.shape[:1]) + (x.shape[1] if torch.is_tensor(x) and x.dim() > 1 else 0,) + tuple(ref.shape[1:]))
        if not torch.is_tensor(x) or tuple(x.shape) not in want:
            raise ValueError(f"despeckle_stats: samples must be [B, S, C, H, W] or [B, C, H, W] for ref {tuple(ref.shape)}, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) not in (tuple(ref.shape), tuple(ref.shape[1:])):
            raise ValueError(f"despeckle_stats: labels must be a uint8 tensor of shape {tuple(ref.shape)} or {tuple(ref.shape[1:])}")
        if ref.shape[-1] % 4:
            raise ValueError(f"despeckle_stats: the image width must be a multiple of 4, got {int(ref.shape[-1])}")
        return ops.despeckle_stats(x.contiguous(), ref.contiguous(), labels.contiguous(), L)

    @staticmethod
    def sparsification(output, uncertainty, target, K=20):
        """Sparsification records of an uncertainty map [B, ...] (output_std, an interval width, a CRPS map) for the restoration
        output [B, ...] against target [B, ...] -> (sums, counts, sums_oracle, counts_oracle, tau) on the device: two
        ops.sparsification calls, the map's and the oracle's (three launches each, no sort, no host copy);
        sparsification_summary(sums, counts, sums_oracle, counts_oracle, K) reads the curves and AUSE / AURG off them."""
        K = _sparsification_K(K)
        for name, t in (("output", output), ("uncertainty", uncertainty), ("target", target)):
            if not torch.is_tensor(t) or t.dim() < 2 or tuple(t.shape) != tuple(output.shape):
                raise ValueError(f"sparsification: {name} must be a [B, ...] tensor of the output's shape, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        output, target = output.contiguous(), target.contiguous()
        sums, counts, tau = ops.sparsification(uncertainty.contiguous(), output, target, K)
        sums_oracle, counts_oracle, _ = ops.sparsification(None, output, target, K)
        return sums, counts, sums_oracle, counts_oracle, tau

    @staticmethod
    def member_distances(samples, target=None):
        """Image-to-image distances of samples [B, S, ...] (reverse_ddpm_ensemble(..., return_samples=True)), with target [B, ...] as a
        last row when given -> (d2 float64 [B, M, M], counts int32 [B, 2], pick int32 [B, 2] = medoid, best member) on the device, from
        one ops.ensemble_distances call (two launches, no host copy); ensemble_distance_summary(d2, counts, S, target is not None)
        reads ES / ES_FAIR / DIVERSITY off them, ops.ensemble_pick_rows(samples, pick, col) fetches a picked member."""
        if not torch.is_tensor(samples) or samples.dim() < 3:
            raise ValueError("member_distances: samples must be a [B, S, ...] tensor (reverse_ddpm_ensemble(..., return_samples=True))")
        if target is not None and (not torch.is_tensor(target) or tuple(target.shape) != (samples.shape[0],) + tuple(samples.shape[2:])):
            raise ValueError(f"member_distances: target must be [B, ...] = {(samples.shape[0],) + tuple(samples.shape[2:])}, got "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        return ops.ensemble_distances(samples.contiguous(), None if target is None else target.contiguous())

    @staticmethod
    def principal_modes(samples, target=None, K=4):
        """The principal components of samples [B, S, ...] (reverse_ddpm_ensemble(..., return_samples=True)) about their per-pixel mean,
        with target [B, ...] placed in them when given -> dict(modes float32 [B, min(K, S), ...]: the leading unit-norm mode images
        u_k; lam float64 [B, S]: the variance sums along the modes, descending; vec float64 [B, S, S]: row k = the members'
        coordinates along u_k divided by sqrt(lam_k); tcoord float64 [B, S] = <target - mean, u_k>; tnorm2 float64 [B] =
        |target - mean|^2; info int32 [B, 2] = (rank, sweeps); counts int32 [B, 2] = (valid, invalid) pixels), all on the device.
        One ops.ensemble_distances call, one ops.ensemble_modes call and one ops.ensemble_project call (four launches for K <= 8), no
        host copy; ensemble_mode_summary(lam, tcoord, tnorm2, info, counts, S, target is not None) reads EXPLAINED / EFF_MODES /
        SPAN_SHARE / MODE_Z off them.  A member is mean + sum_k sqrt(lam_k) vec[k][s] u_k; a mode past the rank is a zero image."""
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError(f"principal_modes: K must be an int >= 1, got {K!r}")
        if not torch.is_tensor(samples) or samples.dim() < 3:
            raise ValueError("principal_modes: samples must be a [B, S, ...] tensor (reverse_ddpm_ensemble(..., return_samples=True))")
        if target is not None and (not torch.is_tensor(target) or tuple(target.shape) != (samples.shape[0],) + tuple(samples.shape[2:])):
            raise ValueError(f"principal_modes: target must be [B, ...] = {(samples.shape[0],) + tuple(samples.shape[2:])}, got "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        samples = samples.contiguous()
        S = samples.shape[1]
        d2, counts, _ = ops.ensemble_distances(samples, None if target is None else target.contiguous())
        lam, vec, coef, tcoord, tnorm2, info = ops.ensemble_modes(d2, S, target is not None)
        modes = ops.ensemble_project(samples, coef[:, :min(K, S)])
        return dict(modes=modes, lam=lam, vec=vec, tcoord=tcoord, tnorm2=tnorm2, info=info, counts=counts)

    @staticmethod
    def power_spectra(samples_or_output, target=None):
        """Radial power spectra of an ensemble's samples [B, S, C, H, W] (reverse_ddpm_ensemble(..., return_samples=True)) or of one
        restoration [B, C, H, W] (S = 1), with target [B, C, H, W] when given -> a dict of float64 per-bin power sums on the device
        (ops.radial_power_spectrum; bins, their point counts and frequencies: ops.radial_bins(H, W)):
            output [B, C, nb]                 the restoration; for samples their per-pixel mean (ops.ensemble_stats)
            members [B, C, S, nb]             every member (samples only)
            target, residual [B, C, nb]       the truth, and output - target          (with a target)
            member_residuals [B, C, S, nb]    member - target                         (samples and a target)
        The differences are formed in fp64 inside the kernel.  One radial_power_spectrum call for the planes themselves and one for
        the residual planes, no host copy; spectrum_summary(spectra, counts, S) reads the ratios and the spread-skill curve off it."""
        x = samples_or_output
        if not torch.is_tensor(x) or x.dim() not in (4, 5):
            raise ValueError("power_spectra: takes samples [B, S, C, H, W] or an output [B, C, H, W]")
        if x.dim() == 5:
            B, S, Cn = x.shape[:3]
            mean, _ = ops.ensemble_stats(x.contiguous())
            rows = torch.cat([mean.unsqueeze(1), x], dim=1).transpose(1, 2)  # [B, C, 1 + S, H, W]: the mean, then the members
        else:
            (B, Cn), S = x.shape[:2], 0
            rows = x.unsqueeze(2)
        if target is not None and (not torch.is_tensor(target) or tuple(target.shape) != (B, Cn) + tuple(x.shape[-2:])):
            raise ValueError(f"power_spectra: target must be [B, C, H, W] = {(B, Cn) + tuple(x.shape[-2:])}, got "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        planes = rows if target is None else torch.cat([rows, target.unsqueeze(2)], dim=2)
        own = ops.radial_power_spectrum(planes.contiguous())  # [B, C, 1 + S (+ 1), nb]
        out = dict(output=own[:, :, 0])
        if S:
            out["members"] = own[:, :, 1:1 + S]
        if target is not None:
            out["target"] = own[:, :, 1 + S]
            res = ops.radial_power_spectrum(rows.contiguous(), sub=target.contiguous(), sub_rep=1 + S)
            out["residual"] = res[:, :, 0]
            if S:
                out["member_residuals"] = res[:, :, 1:]
        return out

    @staticmethod
    def _order_stats(samples, level):
        """lo / hi / median maps of samples [B, S, ...] at credible level `level`, each a contiguous [B, ...]: planes k_lo, k_hi, k_m0,
        k_m1 of ONE selection launch over the samples.  With B = 1 the maps are that result's planes themselves; with B > 1 a plane
        is strided over the batch and is copied out by ops.gather_channel (a library launch per map, exact).  An even S's median is
        0.5*x_(k_m0) + 0.5*x_(k_m1) (ops.axpby: both products exact, one rounded add), an odd S's is plane k_m0 itself."""
        idx = order_stat_indices(samples.shape[1], level)
        ks = [idx["k_lo"], idx["k_hi"], idx["k_m0"], idx["k_m1"]]
        planes = ops.ensemble_order_stats(samples, ks)
        B = samples.shape[0]
        shape = (B,) + tuple(samples.shape[2:])
        flat = planes.view(B, len(ks), 1, -1)

        def pick(i):
            if B == 1:
                return planes[:, i]
            return ops.gather_channel(flat, torch.tensor([i] * B, dtype=torch.int32).to(planes.device)).view(shape)

        lo, hi, m0 = pick(0), pick(1), pick(2)
        median = m0 if idx["k_m0"] == idx["k_m1"] else ops.axpby(m0, pick(3), 0.5, 0.5)
        return dict(lo=lo, hi=hi, median=median, level=level, nominal=idx["nominal"], ks=ks)
