"""`CLIPDriftModel` -- the two-network (drift + noise) model wrapper with the reference's method surface
(models/drift_noise_model.py:27-756) over the MI355X-native nets.

Kept from the reference: constructor/`create_CLIPDriftModel` option names (:758-810), feed_data (:182-195),
optimize_parameters -> optimize_parameters_inputRes (:231-232, 242-312), optimize_score_map (:234-240),
test (:648-652), get_visuals/get_nets, save/load file naming `{iter}_{DP,NP,DN,NN}.pth` +
`lastest_*_ema.pth` [sic] (:670-755), save_training_state/resume_training, set_eval/set_train/set_gpu,
loss-message helpers, learning-rate helpers.
Changed on purpose:
  * data parallelism = the optimizers' flat gradient buffers all-reduced over RCCL, one all-reduce each per step (parallel.GradSync)
    instead of 10 DistributedDataParallel wrappers with find_unused_parameters (:115-146);
  * the 9 per-step `.item()` host syncs (:299-309) become one device->host copy of a 5-float loss record;
  * the 8 dead alternative train steps (:314-629) are not reproduced (out of scope);
  * `.cuda()` is not hard-coded: the device is an argument;
  * the 224 hard-coded in optimize_score_map (:234) is the input size.
"""
import os
import time
from collections import OrderedDict

import torch
import torch.nn as nn

from .modules import create_net
from .modules.MSM_degEmb_Unet import ScoreMapModule
from .text_encoder import build_text_encoder


class EMA(nn.Module):
    """Minimal stand-in for ema_pytorch.EMA with the same state-dict key prefixes (`online_model.`, `ema_model.`)
    so `lastest_*_ema.pth` files keep their layout (drift_noise_model.py:122,139,151-152,687-692)."""

    def __init__(self, model, beta=0.995, update_every=10):
        super().__init__()
        import copy
        self.online_model = model
        self.ema_model = copy.deepcopy(model)
        for p in self.ema_model.parameters():
            p.requires_grad_(False)
        self.beta, self.update_every = beta, update_every
        self.register_buffer("step", torch.zeros((), dtype=torch.long))
        self.register_buffer("initted", torch.zeros((), dtype=torch.bool))

    @torch.no_grad()
    def update(self):
        self.step += 1
        if int(self.step) % self.update_every != 0:
            return
        if not bool(self.initted):
            for pe, po in zip(self.ema_model.parameters(), self.online_model.parameters()):
                pe.copy_(po)
            self.initted.fill_(True)
            return
        from .. import ops
        for pe, po in zip(self.ema_model.parameters(), self.online_model.parameters()):
            if pe.is_cuda and pe.is_contiguous() and po.is_contiguous():
                ops.axpby(pe.data, po.data, self.beta, 1.0 - self.beta, out=pe.data)  # HIP kernel, in place
            else:
                pe.lerp_(po.to(pe.dtype), 1.0 - self.beta)

    def forward(self, *a, **k):
        return self.ema_model(*a, **k)


CONV_DTYPES = ("f32", "bf16")


def parse_conv_dtype(value):
    """model option conv_dtype -> "f32" | "bf16" (None = "f32"); anything else raises ValueError"""
    if value is None:
        return "f32"
    v = str(value).strip().lower() if isinstance(value, str) else value
    if v not in CONV_DTYPES:
        raise ValueError(f"conv_dtype must be one of {CONV_DTYPES}, got {value!r}")
    return v


class CLIPDriftModel():
    def __init__(self, text_encoder_pretrain_path, drift_net_lr, noise_net_lr, weight_decay_drift, beta1, beta2, nepoch, eta_min,
                 dist=False, gpu=True, optimize_type='predict_noise', optimize_target='std', if_train=True, dnet_settings=None,
                 nnet_settings=None, drift_loss='l2', noise_loss='none', if_MultiScoreMap=False, score_map_ch_mult=[1, 1, 2, 4],
                 score_map_ngf=64, use_image_context=False, use_degra_context=False, CLIP_Type="CLIP", device=None, text_encoder=None,
                 class_tokens=None, score_map_dropout=0.1, score_map_decoder="ContextDecoder", score_map_if_flash=False, conv_dtype="f32",
                 grad_clip_norm=None, skip_nonfinite_steps=False, accum_steps=1):
        """score_map_dropout: dropout of the ScoreMapModules' decoder blocks in training mode -- the reference builds them with
        ContextDecoder's default 0.1 (models/_modified_BiomedCLIP.py:1194-1201; drift_noise_model.py:110-112 passes no value);
        model option `score_map_dropout` overrides (0 = the deterministic training function of rounds 1-2).
        score_map_decoder: "ContextDecoder" (the frozen spec) or "ContextDecoder_Hierachical" (TransformerDecoderLayer_scaled blocks,
        models/_modified_BiomedCLIP.py:552-590,1247-1308); model option of the same name.
        score_map_if_flash (with ContextDecoder_Hierachical): the decoder attentions in the reference's half-precision form
        (Attention_flash, :481-517; the reference class's default) -- a labelled reduced-precision variant, inference only; False =
        fp32, what if_flash=False computes.
        conv_dtype: operand precision of both nets' 3x3 convs, sampling and training -- "f32" (default, the parity path) or "bf16",
        the labelled reduced-precision variant (operands and weights rounded once to bf16 after the fp32 gather, fp32 sums and epilogue;
        csrc/conv_bf16.hip); model option of the same name.  Anything else raises ValueError.
        grad_clip_norm (a finite number > 0, or None) / skip_nonfinite_steps (bool): the gradient guard of both optimizers (FusedAdam's
        max_grad_norm / skip_nonfinite, each net clipped by its own global norm); model options of the same names.  Both off (the
        default): the training step launches what it always launched.
        accum_steps (an int >= 1): gradient accumulation; model option of the same name.  Every optimize_parameters() is a micro-step on
        the fed batch; the accum_steps-th of a group exchanges, applies both Adam steps to the mean of the group's gradients (equal
        micro-batch sizes assumed), updates the EMAs and copies the group's mean losses to the host -- `stepped` says whether the last
        call did.  1 (the default): every call is a step, as always."""
        conv_dtype = parse_conv_dtype(conv_dtype)
        from ..train_ops import parse_accum_steps, parse_max_grad_norm, parse_skip_nonfinite
        self.accum_steps = parse_accum_steps(accum_steps)
        self.stepped, self._loss_acc = False, None  # the last optimize_parameters() applied a step; the open group's loss record
        self.grad_clip_norm = parse_max_grad_norm(grad_clip_norm, "grad_clip_norm")
        self.skip_nonfinite_steps = parse_skip_nonfinite(skip_nonfinite_steps, "skip_nonfinite_steps")
        self.grad_info, self.skipped_steps = None, 0
        dnet_settings = dict(dnet_settings)
        nnet_settings = dict(nnet_settings)
        for s in (dnet_settings, nnet_settings):  # :58-61
            s['use_image_context'] = use_image_context
            s['use_degra_context'] = use_degra_context
        self.dnet_settings, self.nnet_settings = dnet_settings, nnet_settings
        self.score_map_ch_mult = score_map_ch_mult
        self.use_image_context, self.use_degra_context = use_image_context, use_degra_context
        self.optimize_target, self.optimize_type = optimize_target, optimize_type
        self.drift_loss, self.noise_loss = drift_loss, noise_loss
        self.dist = dist
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if (gpu and torch.cuda.is_available()) else torch.device("cpu")
        self.device = torch.device(device)
        if text_encoder is None:
            text_encoder, token_embed_dim = build_text_encoder(text_encoder_pretrain_path, CLIP_Type)
        else:
            token_embed_dim = 768 if CLIP_Type == "BiomedCLIP" else 512  # :70-77
        for p in text_encoder.parameters():
            p.requires_grad_(False)
        self.text_encoder = text_encoder.to(self.device)
        self.token_embed_dim = token_embed_dim
        self.score_map_dropout = float(score_map_dropout)

        def prompts(settings):
            if settings.get('text_module') != 'scoremap':
                return None
            if settings.get('if_MultiScoreMap'):
                return nn.ModuleList([ScoreMapModule(visual_dim=score_map_ngf * score_map_ch_mult[i], CLIP_Type=CLIP_Type,
                                                     token_embed_dim=token_embed_dim, dropout=score_map_dropout, decoder_type=score_map_decoder, if_flash=score_map_if_flash)
                                      for i in range(len(score_map_ch_mult))])
            # reference models/drift_noise_model.py:113-114,130-131: ONE default ScoreMapModule() handed to create_net().  The UNet that
            # consumes it is not part of the reference snapshot; this build's frozen spec puts it on the
            # full-resolution level (visual_dim = nf, the module's default 64) with its score map embedded into `score_map_chan` channels
            # of that level's skip
            nf = int(settings.get('nf', 64) or 64)
            return ScoreMapModule(visual_dim=nf, CLIP_Type=CLIP_Type, token_embed_dim=token_embed_dim, dropout=score_map_dropout,
                                  decoder_type=score_map_decoder, if_flash=score_map_if_flash)

        self.drift_prompt = prompts(dnet_settings)
        self.noise_prompt = prompts(nnet_settings)
        if class_tokens is not None:  # real class-prompt token ids [K, N1] (the reference: clip.tokenize(prompts, context_length=N1))
            for smms in (self.drift_prompt, self.noise_prompt):
                for m in ([] if smms is None else (smms if isinstance(smms, nn.ModuleList) else [smms])):
                    m.set_class_tokens(class_tokens)
        self.drift_net = create_net(dnet_settings, CLIP_ScoreMapModule=self.drift_prompt).to(self.device)
        self.noise_net = create_net(nnet_settings, CLIP_ScoreMapModule=self.noise_prompt).to(self.device)
        self.conv_dtype = conv_dtype
        self.drift_net.conv_dtype = self.noise_net.conv_dtype = conv_dtype
        if self.drift_prompt is not None:
            self.dp_ema = EMA(self.drift_prompt, beta=0.995, update_every=10)
            self.np_ema = EMA(self.noise_prompt, beta=0.995, update_every=10)
        self.dn_ema = self.nn_ema = None  # created lazily: a deep copy of both nets doubles weight memory (reference :151-152)
        self.grad_sync = None
        if dist and torch.distributed.is_available() and torch.distributed.is_initialized():
            from ..parallel import GradSync
            self.grad_sync = GradSync()
            self.grad_sync.broadcast_parameters(list(self.drift_net.parameters()) + list(self.noise_net.parameters()))
        if if_train:
            from ..train_ops import FusedAdam
            guard = dict(max_grad_norm=self.grad_clip_norm, skip_nonfinite=self.skip_nonfinite_steps, accum_steps=self.accum_steps)
            self.drift_optimizer = FusedAdam(self.drift_net.parameters(), lr=drift_net_lr, weight_decay=weight_decay_drift, betas=(beta1, beta2), **guard)
            self.noise_optimizer = FusedAdam(self.noise_net.parameters(), lr=noise_net_lr, weight_decay=weight_decay_drift, betas=(beta1, beta2), **guard)
            self.drift_lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.drift_optimizer, T_max=nepoch, eta_min=eta_min)
            self.noise_lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.noise_optimizer, T_max=nepoch, eta_min=eta_min)
        self.visuals = None
        self.reinit_loss_message()

    # ---- reference plumbing ------------------------------------------------------------------------
    def update_lr(self):
        self.drift_lr_scheduler.step()
        self.noise_lr_scheduler.step()

    def get_current_learning_rate(self):
        return self.noise_optimizer.param_groups[0]["lr"]

    def set_sde(self, sde):
        self.sde = sde

    def feed_data(self, data):  # :182-195
        self.input = data['input'].to(self.device, torch.float32).contiguous()
        self.target = data['target'].to(self.device, torch.float32).contiguous()
        self.names = list(data['names'])
        self.A_emb = data['A_emb'].to(self.device, torch.float32).contiguous() if self.use_image_context else None
        time_idx, drift_noised_x, drift, std_noise, noise = self.sde.forward_diffusion(self.target, self.input)
        self.t, self.drift_noised_x, self.drift, self.std_noise, self.noise = time_idx, drift_noised_x, drift, std_noise, noise

    def reinit_loss_message(self):  # :197-218
        self.loss_info = {'latest': {'l': 0, 'nsml': 0, 'dsml': 0, 'nl': 0, 'dl': 0},
                          'avg': {'l': 0, 'dl': 0, 'nl': 0, 'dsml': 0, 'nsml': 0}, 'num': 0}

    def get_loss_message(self):  # :220-229
        num = max(self.loss_info['num'], 1)
        message = ""
        for k in self.loss_info['latest'].keys():
            message += '({}={:4f}/{:4f})'.format(k, self.loss_info['latest'][k], self.loss_info['avg'][k] / num)
        return message

    def get_grad_message(self):
        """the gradient guard's line for the log: both nets' gradient norms and clip coefficients of the latest step and the running
        count of skipped steps; empty until a guarded step has run"""
        gi = self.grad_info
        if not gi:
            return ""
        message = ""
        for k, key in (('d', 'drift'), ('n', 'noise')):
            if gi[key] is not None:
                message += '({}gn={:.4e} {}coef={:.4f})'.format(k, gi[key]['norm'], k, gi[key]['coef'])
        return message + '(skipped={:d})'.format(gi['skipped_steps'])

    def optimize_parameters(self):  # :231-232
        """-> (loss, forward time); with accum_steps > 1 the loss is None unless this call closed its group (self.stepped), and then
        the mean over the group"""
        return self.optimize_parameters_inputRes()

    @property
    def micro_step(self):
        """micro-steps of the open group taken so far (0: no group is open)"""
        return self.drift_optimizer.micro_step

    def set_accum_steps(self, accum_steps):
        """micro-steps per optimizer step of both optimizers, from the next group on; refused while a group is open"""
        for o in (self.drift_optimizer, self.noise_optimizer):
            o.set_accum_steps(accum_steps)
        self.accum_steps = self.drift_optimizer.accum_steps

    def discard_accumulated(self):
        """drop an open group of micro-steps (gradients and loss records).  -> micro-steps dropped"""
        dropped = max(o.discard_accumulated() for o in (self.drift_optimizer, self.noise_optimizer))
        self._loss_acc = None
        return dropped

    def optimize_score_map(self, score_maps, label, size=None, mult=[1, 2, 4, 8], want_grads=False):
        """sum_i MSE(score_maps[i], Resize((size[0]//mult[i], size[1]//mult[i]))(label)) / 2   (:234-240).
        `size` defaults to the label's own H, W (the reference hard-codes [224, 224], its dataset's size).  Resize is torchvision's
        bilinear tensor resize WITHOUT antialiasing: the reference pins PyTorch 1.13.1 (README.md:28), i.e. torchvision 0.14, where
        `Resize(size)` on a tensor means antialias=None = off (it became on-by-default for tensors only in 0.17).
        Returns the loss as a 0-dim device tensor (HIP resize + MSE kernels; no graph is recorded -- the training step feeds
        autograd the explicit per-map gradients, which `want_grads=True` also returns)."""
        from ..train_ops import score_map_losses
        label = label.contiguous()
        H, W = (int(size[0]), int(size[1])) if size is not None else tuple(label.shape[-2:])
        rec = torch.zeros(len(score_maps), device=label.device, dtype=torch.float32)
        grads = score_map_losses(score_maps, label, rec, 0, mult=mult, size=(H, W), want_grad=want_grads)
        loss = rec.sum() / 2.0
        return (loss, grads) if want_grads else loss

    def optimize_parameters_inputRes(self):
        """(x_t-cond, cond)->drift; (x_t-cond, x_t)->noise; L2 + score-map pyramid losses; Adam (:242-312)."""
        from ..train_ops import train_step_inputRes
        return train_step_inputRes(self)

    # ---- sampling ----------------------------------------------------------------------------------
    @torch.no_grad()
    def test(self, **kw):  # :648-652
        """one restoration per input; with sde.num_samples > 1 (driftSDE) a posterior ensemble: output / get_visuals() are the per-pixel
        mean of the members, output_std their spread, samples the members [B, S, ...] when called with return_samples=True; with
        sde.interval set as well, output_median / output_lo / output_hi are the per-pixel median and credible-interval maps (else None)"""
        self.output_std = self.samples = None
        self.output_median = self.output_lo = self.output_hi = None
        self.output_modes = None
        if getattr(self.sde, "num_samples", 1) > 1:
            res = self.sde.reverse_ddpm_ensemble(self.input, self.names, self.text_encoder, reverse_type=self.optimize_target,
                                                 optimize_type=self.optimize_type, image_context=self.A_emb, **kw)
            out, self.output_std = res[0], res[1]
            self.samples = res[2] if len(res) > 2 else None
            stats = getattr(self.sde, "last_order_stats", None)
            if stats is not None:
                self.output_median, self.output_lo, self.output_hi = stats["median"], stats["lo"], stats["hi"]
        else:
            out = self.sde.reverse_ddpm(self.input, self.names, self.text_encoder, reverse_type=self.optimize_target,
                                        optimize_type=self.optimize_type, image_context=self.A_emb, **kw)
        self.output = out
        self.visuals = out.detach().cpu().numpy()

    def score_ensemble(self, want_map=False):
        """ensemble scores of the members test(return_samples=True) left in self.samples against self.target (driftSDE.score_ensemble) ->
        (sums [B, 3], counts [B, S + 2], crps_map or None) on the device"""
        if getattr(self, "samples", None) is None:
            raise ValueError("score_ensemble: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        return self.sde.score_ensemble(self.samples, self.target, want_map=want_map)

    def member_distances(self, with_target=True):
        """image-to-image distances of the members test(return_samples=True) left in self.samples, with self.target as a last row when
        with_target (driftSDE.member_distances) -> (d2 [B, M, M] float64, counts [B, 2], pick [B, 2] = medoid, best member) on the
        device: two launches.  The picks are kept for pick_member."""
        if getattr(self, "samples", None) is None:
            raise ValueError("member_distances: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        d2, counts, pick = self.sde.member_distances(self.samples, self.target if with_target else None)
        self._member_pick = (self.samples, bool(with_target), pick)
        return d2, counts, pick

    def pick_member(self, which="medoid"):
        """one member per image out of self.samples -> [B, ...]: "medoid", the member with the smallest summed distance to the other
        members (a real draw, and the most central one), or "best", the member nearest to self.target (the oracle pick).  One launch on
        the picks of the last member_distances() call for these samples; without such a call (for "best": one with the target) it is
        made first."""
        if which not in ("medoid", "best"):
            raise ValueError(f'pick_member: which must be "medoid" or "best", got {which!r}')
        if getattr(self, "samples", None) is None:
            raise ValueError("pick_member: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        held = getattr(self, "_member_pick", None)
        if held is None or held[0] is not self.samples or (which == "best" and not held[1]):
            self.member_distances(with_target=which == "best")
            held = self._member_pick
        from .. import ops
        return ops.ensemble_pick_rows(self.samples.contiguous(), held[2], 0 if which == "medoid" else 1)

    def principal_modes(self, K=4, with_target=True):
        """the principal modes of the members test(return_samples=True) left in self.samples, with self.target placed in them when
        with_target (driftSDE.principal_modes) -> dict(modes, lam, vec, tcoord, tnorm2, info, counts) on the device.  The mode images
        are kept as self.output_modes [B, min(K, S), C, H, W], the record for mode_traversal."""
        if getattr(self, "samples", None) is None:
            raise ValueError("principal_modes: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        rec = self.sde.principal_modes(self.samples, self.target if with_target else None, K=K)
        self.output_modes = rec["modes"]
        self._modes = (self.samples, rec)
        return rec

    def mode_traversal(self, k, alpha):
        """self.output moved along mode k by alpha standard deviations of the ensemble -> [B, C, H, W]:
        output + alpha sqrt(lam_k / (S - 1)) u_k, one ops.axpby per image (the per-image scalar costs one small host read of lam).
        Needs principal_modes(K > k) for the held samples; without such a call it is made first, without the target."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"mode_traversal: k must be an int >= 0, got {k!r}")
        if getattr(self, "samples", None) is None:
            raise ValueError("mode_traversal: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        S = self.samples.shape[1]
        if k >= S:
            raise ValueError(f"mode_traversal: k = {k} is outside the {S} modes of {S} members")
        held = getattr(self, "_modes", None)
        if held is None or held[0] is not self.samples or held[1]["modes"].shape[1] <= k:
            self.principal_modes(K=max(k + 1, 4), with_target=False)
            held = self._modes
        from .. import ops
        rec = held[1]
        lam_k = rec["lam"][:, k].cpu().tolist()
        out = torch.empty_like(self.output)
        for b, l in enumerate(lam_k):
            scale = float(alpha) * (l / (S - 1)) ** 0.5 if l > 0 else 0.0
            ops.axpby(self.output[b].contiguous(), rec["modes"][b, k], 1.0, scale, out=out[b])
        return out

    def sparsification(self, K=20, key="std"):
        """sparsification records of an uncertainty map of the ensemble test(return_samples=True) left, for self.output against
        self.target (driftSDE.sparsification) -> (sums, counts, sums_oracle, counts_oracle, tau) on the device.  key: "std", the
        members' spread output_std; "width", output_hi - output_lo (needs the sde's interval); "crps", the CRPS map of
        score_ensemble(want_map=True): a key that knows the truth, for comparison."""
        if key not in ("std", "width", "crps"):
            raise ValueError(f'sparsification: key must be "std", "width" or "crps", got {key!r}')
        if getattr(self, "samples", None) is None:
            raise ValueError("sparsification: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
        if key == "std":
            unc = self.output_std
        elif key == "width":
            if self.output_lo is None or self.output_hi is None:
                raise ValueError("sparsification: no interval maps are held; run test(return_samples=True) with the sde's interval set first")
            from .. import ops
            unc = ops.axpby(self.output_hi, self.output_lo, 1.0, -1.0)
        else:
            unc = self.score_ensemble(want_map=True)[2]
        return self.sde.sparsification(self.output, unc, self.target, K=K)

    def region_scores(self, labels, L, what="ensemble"):
        """the ensemble-scores record per region of a uint8 label map, of what test() left against self.target (driftSDE.region_scores)
        -> (sums [B, L, 4], counts [B, L, S + 2], outside [B]) on the device.  what: "ensemble", the members in self.samples (needs
        test(return_samples=True)); "output", self.output as an ensemble of one (S = 1: MAE / RMSE / bias per region); "median",
        output_median (needs the sde's interval).  labels: [B, C, H, W], one shared [C, H, W], or [H, W], which is expanded over the
        channels; a label >= L (255 by convention) keeps its pixel out of every region."""
        if what not in ("ensemble", "output", "median"):
            raise ValueError(f'region_scores: what must be "ensemble", "output" or "median", got {what!r}')
        if getattr(self, "output", None) is None:
            raise ValueError("region_scores: no output is held; run test() first")
        if what == "ensemble":
            if getattr(self, "samples", None) is None:
                raise ValueError("region_scores: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
            held = self.samples
        elif what == "median":
            if getattr(self, "output_median", None) is None:
                raise ValueError("region_scores: no median map is held; run test(return_samples=True) with the sde's interval set first")
            held = self.output_median
        else:
            held = self.output
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
            raise ValueError("region_scores: labels must be a uint8 tensor")
        labels = labels.to(self.target.device)
        if labels.dim() == 2:
            labels = labels[None].expand(self.target.shape[1], -1, -1)
        return self.sde.region_scores(held, self.target, labels.contiguous(), L)

    def despeckle_stats(self, labels, L, what="ensemble", against="input"):
        """the sums behind the no-reference despeckling statistics per region of a uint8 label map, of what test() left
        (driftSDE.despeckle_stats) -> (sums [B, S, L, 12], counts [B, S, L, 4], outside [B]) on the device.  what: as in region_scores
        ("ensemble": the members in self.samples; "output": self.output, S = 1; "median": output_median).  against: "input", the noisy
        image the chain started from (needs no ground truth), or "target".  labels: [B, C, H, W], one shared [C, H, W], or [H, W], which is
        expanded over the channels; a label >= L (255 by convention) keeps its pixel out of every region."""
        if what not in ("ensemble", "output", "median"):
            raise ValueError(f'despeckle_stats: what must be "ensemble", "output" or "median", got {what!r}')
        if against not in ("input", "target"):
            raise ValueError(f'despeckle_stats: against must be "input" or "target", got {against!r}')
        if getattr(self, "output", None) is None:
            raise ValueError("despeckle_stats: no output is held; run test() first")
        if what == "ensemble":
            if getattr(self, "samples", None) is None:
                raise ValueError("despeckle_stats: no samples are held; run test(return_samples=True) with the sde's num_samples > 1 first")
            held = self.samples
        elif what == "median":
            if getattr(self, "output_median", None) is None:
                raise ValueError("despeckle_stats: no median map is held; run test(return_samples=True) with the sde's interval set first")
            held = self.output_median
        else:
            held = self.output
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
            raise ValueError("despeckle_stats: labels must be a uint8 tensor")
        ref = self.input if against == "input" else self.target
        labels = labels.to(ref.device)
        if labels.dim() == 2:
            labels = labels[None].expand(ref.shape[1], -1, -1)
        return self.sde.despeckle_stats(held, ref, labels.contiguous(), L)

    def power_spectra(self, with_target=True):
        """radial power spectra of what test() left (driftSDE.power_spectra): of the members in self.samples and their mean after
        test(return_samples=True), else of self.output (the plain chain: S = 1), against self.target when with_target -> a dict of
        float64 [B, C, (S,) nb] power sums on the device; spectrum_summary(spectra, ops.radial_bins(H, W)[1], S) turns them into
        PSDs, the ratios to the truth's spectrum and the per-frequency spread-skill curve."""
        if getattr(self, "output", None) is None:
            raise ValueError("power_spectra: no output is held; run test() first")
        held = self.samples if getattr(self, "samples", None) is not None else self.output
        return self.sde.power_spectra(held, self.target if with_target else None)

    def get_visuals(self):
        return self.visuals

    def get_nets(self, use_ema=False):  # :657-668
        if use_ema:
            self._ensure_net_ema()
            return {'noise_net': self.nn_ema, 'drift_net': self.dn_ema}
        return {'noise_net': self.noise_net, 'drift_net': self.drift_net}

    def _ensure_net_ema(self):
        if self.dn_ema is None:
            self.dn_ema = EMA(self.drift_net, beta=0.995, update_every=10)
            self.nn_ema = EMA(self.noise_net, beta=0.995, update_every=10)

    def set_eval(self):
        self.drift_net.eval()
        self.noise_net.eval()

    def set_train(self):
        self.drift_net.train()
        self.noise_net.train()

    def set_gpu(self, device):  # :635-642
        self.drift_net.to(device)
        self.noise_net.to(device)
        self.text_encoder = self.text_encoder.to(device)
        self.device = torch.device(device)

    # ---- checkpoint wire format (:670-755) -----------------------------------------------------------
    @staticmethod
    def save_network(network, network_label, iter_label, save_dir):
        state_dict = OrderedDict((k, v.detach().cpu()) for k, v in network.state_dict().items())
        torch.save(state_dict, os.path.join(save_dir, "{}_{}.pth".format(iter_label, network_label)))

    def save(self, iter_label, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        self._ensure_net_ema()
        if self.dnet_settings['text_module'] == 'scoremap':
            self.save_network(self.drift_prompt, "DP", iter_label, save_dir)
            self.save_network(self.noise_prompt, "NP", iter_label, save_dir)
            self.save_network(self.dp_ema, "DP_ema", 'lastest', save_dir)
            self.save_network(self.np_ema, "NP_ema", 'lastest', save_dir)
        self.save_network(self.drift_net, "DN", iter_label, save_dir)
        self.save_network(self.noise_net, "NN", iter_label, save_dir)
        self.save_network(self.dn_ema, "DN_ema", 'lastest', save_dir)
        self.save_network(self.nn_ema, "NN_ema", 'lastest', save_dir)

    def save_training_state(self, epoch, iter_step, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        state = {"epoch": epoch, "iter": iter_step,
                 "schedulers": [self.drift_lr_scheduler.state_dict(), self.noise_lr_scheduler.state_dict()],
                 "optimizers": [self.drift_optimizer.state_dict(), self.noise_optimizer.state_dict()]}
        torch.save(state, os.path.join(save_dir, "{}.state".format(iter_step)))

    @staticmethod
    def load_training_state(path, trusted=False):
        """Read a `{iter}.state` file (the call trainUM.py makes before resume_training).  This build's layout (state dicts) loads
        under torch's `weights_only=True`.  The reference pickles the optimizer and scheduler OBJECTS (:694-704), which that mode
        rejects (it cannot even rebuild Adam's defaultdict); they are read by an unpickler whose find_class admits exactly what such
        a file holds -- torch.optim.Adam, CosineAnnealingLR, Parameter / tensor / storage rebuilders, defaultdict / OrderedDict --
        and nothing that could run code.  A pickle holding anything else needs `trusted=True` (option path.resume_state_trusted),
        i.e. the unrestricted unpickler the reference's torch 1.13 `torch.load` was."""
        import pickle
        try:
            return torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError:
            pass
        try:
            return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_restricted_pickle())
        except pickle.UnpicklingError as e:
            if not trusted:
                raise RuntimeError(f"{path}: holds more than state dicts and pickled Adam / CosineAnnealingLR objects ({e}); set "
                                   f"path.resume_state_trusted: true to unpickle it without restrictions") from e
        return torch.load(path, map_location="cpu", weights_only=False)

    def resume_training(self, resume_state):
        """Both `.state` layouts resume: this build's (state dicts) and the reference's, which pickles the scheduler and optimizer
        OBJECTS (models/drift_noise_model.py:694-704; its own resume_training then swaps them in wholesale, :702-704 -- optimizers
        that update orphaned copies of the weights).  From reference objects the Adam moments, step counts, hyper-parameters and
        the schedulers' epochs are taken over into the live fused optimizers."""
        for sch, s in zip((self.drift_lr_scheduler, self.noise_lr_scheduler), resume_state['schedulers']):
            if hasattr(s, "state_dict"):  # a pickled scheduler object
                s = {k: v for k, v in s.state_dict().items() if k != "optimizer"}
            sch.load_state_dict(s)
        for opt, s in zip((self.drift_optimizer, self.noise_optimizer), resume_state['optimizers']):
            if hasattr(s, "state_dict") or "flat" not in s:  # a torch.optim.Adam object or its state dict
                opt.load_torch_adam(s)
            else:
                opt.load_state_dict(s)
        # iterations with a skipped step: the state holds one count per optimizer, and the larger is the most that is known of both
        self.skipped_steps = max(self.drift_optimizer.skipped_steps, self.noise_optimizer.skipped_steps)

    @staticmethod
    def load_network(load_path, network, strict=True):
        load_net = torch.load(load_path, map_location="cpu")
        clean = OrderedDict()
        for k, v in load_net.items():  # strip DDP prefixes of reference-era checkpoints (:712-730)
            clean[k.replace('module.', '')] = v
        network.load_state_dict(clean, strict=strict)

    def load(self, iter_label, save_dir):
        if self.dnet_settings['text_module'] == 'scoremap':
            self.load_network(os.path.join(save_dir, f"{iter_label}_DP.pth"), self.drift_prompt)
            self.load_network(os.path.join(save_dir, f"{iter_label}_NP.pth"), self.noise_prompt)
        self.load_network(os.path.join(save_dir, f"{iter_label}_DN.pth"), self.drift_net)
        self.load_network(os.path.join(save_dir, f"{iter_label}_NN.pth"), self.noise_net)
        self._ensure_net_ema()
        for label, net in (("DP", getattr(self, "dp_ema", None)), ("NP", getattr(self, "np_ema", None)), ("DN", self.dn_ema), ("NN", self.nn_ema)):
            path = os.path.join(save_dir, f"lastest_{label}_ema.pth")
            if net is not None and os.path.exists(path):
                self.load_network(path, net)


def _restricted_pickle():
    """a `pickle`-shaped module for torch.load(pickle_module=...) whose Unpickler resolves only the globals of a reference-era
    `.state` file (see CLIPDriftModel.load_training_state)"""
    import pickle
    import types
    allowed = {("collections", "OrderedDict"), ("collections", "defaultdict"), ("builtins", "dict"), ("builtins", "set"),
               ("builtins", "list"), ("builtins", "tuple"), ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"),
               ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_parameter"), ("torch._utils", "_rebuild_parameter_with_state"),
               ("torch._tensor", "_rebuild_from_type_v2"), ("torch.nn.parameter", "Parameter"), ("torch", "Size"), ("torch", "device"),
               ("torch.storage", "UntypedStorage"), ("torch.serialization", "_get_layout"),
               ("torch.optim.adam", "Adam"), ("torch.optim.lr_scheduler", "CosineAnnealingLR")}

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            key = ("builtins" if module == "__builtin__" else module, name)  # protocol-2 pickles (torch.save's default) say __builtin__
            if key in allowed or (module == "torch" and name.endswith("Storage")):
                return super().find_class(module, name)
            raise pickle.UnpicklingError(f"global {module}.{name} is not on the .state allow-list")

    # load / loads go through the allow-listing class too: torch's legacy (non-zip) loader calls pickle_module.load(f) directly for
    # the magic number, protocol, sys_info and storage keys -- with the plain pickle.load a crafted single-pickle file ran its
    # __reduce__ callable before any find_class of ours was asked
    def load(f, **kw):
        return Unpickler(f, **kw).load()

    def loads(b, **kw):
        import io
        return Unpickler(io.BytesIO(b), **kw).load()

    mod = types.ModuleType("idiff_restricted_pickle")
    mod.__dict__.update({k: getattr(pickle, k) for k in ("dump", "dumps", "Pickler", "PickleError", "UnpicklingError",
                                                         "HIGHEST_PROTOCOL", "DEFAULT_PROTOCOL")})
    mod.load, mod.loads = load, loads
    mod.Unpickler = Unpickler
    return mod


def create_CLIPDriftModel(train_opt, model_opt, phase='train', **extra):  # :758-810
    kw = dict(drift_net_lr=model_opt['drift_net_lr'], noise_net_lr=model_opt['noise_net_lr'],
              weight_decay_drift=model_opt['weight_decay_drift'], beta1=model_opt['beta1'], beta2=model_opt['beta2'],
              nepoch=train_opt['nepoch'], eta_min=model_opt['eta_min'], optimize_target=model_opt['optimize_target'],
              optimize_type=model_opt['optimize_type'], if_train=(phase == 'train'), dnet_settings=model_opt['dnet_settings'],
              nnet_settings=model_opt['nnet_settings'], drift_loss=model_opt['drift_loss'], noise_loss=model_opt['noise_loss'],
              dist=train_opt['dist'], use_image_context=model_opt['use_image_context'], use_degra_context=model_opt['use_degra_context'],
              CLIP_Type=model_opt["CLIP_Type"] if "CLIP_Type" in model_opt and model_opt["CLIP_Type"] else "CLIP")
    if 'if_MultiScoreMap' in model_opt and model_opt['if_MultiScoreMap'] is not None:
        kw.update(if_MultiScoreMap=model_opt['if_MultiScoreMap'], score_map_ch_mult=model_opt['score_map_ch_mult'],
                  score_map_ngf=model_opt['score_map_ngf'])
    if model_opt.get('score_map_dropout') is not None:
        kw.update(score_map_dropout=float(model_opt['score_map_dropout']))
    if model_opt.get('score_map_decoder'):
        kw.update(score_map_decoder=str(model_opt['score_map_decoder']))
    if model_opt.get('score_map_if_flash') is not None:
        kw.update(score_map_if_flash=bool(model_opt['score_map_if_flash']))
    if model_opt.get('conv_dtype') is not None:
        kw.update(conv_dtype=parse_conv_dtype(model_opt['conv_dtype']))
    if model_opt.get('grad_clip_norm') is not None:
        kw.update(grad_clip_norm=model_opt['grad_clip_norm'])
    if model_opt.get('skip_nonfinite_steps') is not None:
        kw.update(skip_nonfinite_steps=model_opt['skip_nonfinite_steps'])
    if model_opt.get('accum_steps') is not None:
        kw.update(accum_steps=model_opt['accum_steps'])
    kw.update(extra)
    return CLIPDriftModel(model_opt['text_encoder_pretrain_path'], **kw)
