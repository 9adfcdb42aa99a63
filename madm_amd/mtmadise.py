"""``MTMADISE`` -- the meta-architecture of the path with BOTH branches of the reference's ``forward``
(/root/reference/modeling/meta_arch/mtmadise.py:177-691 on top of CMDISE, modeling/meta_arch/cmdise.py:114-349):

* eval  (:657-691): ``MadmInference.forward`` (meta_arch.py);
* train (:180-656, BASELINE config 4): ``model(list[dict]) -> dict[str, scalar Tensor]`` as engine/train_loop.py:277-302
  expects it -- differentiable through standard autograd w.r.t. every ``requires_grad`` parameter, so
  ``scaler.scale(sum(losses.values())).backward()`` / DDP-style hooks / ``clip_grad_norm_`` work unchanged.

One training call = EMA update of the teacher (:184-185), source pass ('default' adapter, :239-256), ClassMix image
(:261-279), target pass on the mixed image (:284-302), teacher pass under no_grad with the EMA projections / head /
prompt (:308-337), pseudo labels + label / weight mixing (:339-392), the colour-label latents of the VAE-decoder losses
(:253-254, 394-397) and ``CmdiseCriterion`` (:441-492).  Every tensor op runs on libmadm_hip kernels: the two gradient
passes are recorded on tapes that ``_student_pass`` owns and passes down as ``tape=`` arguments (block-boundary tape of the
UNet's one forward, raw conv outputs of projections / head) and the losses come back as
the outputs of ONE autograd node (``_TrainStepFn``) whose backward walks those records with the explicit gradient kernels
(backward.py, head.py, backbone.py, criterion.py), weighting each loss by the upstream gradient it receives.

Masked image consistency (``mic`` / ``mic_reg``, :404-420, :471-488; MIC, Hoyer et al. 2023): a third recorded student
pass on the colour-augmented target image with 32 x 32 blocks masked (augment.block_mask), under the target adapter; ``mic``
adds ``masked_prompt_consistency_loss`` (CE of its logits against the teacher's pseudo labels), ``mic_reg`` skips the
projections and the head and adds ``mic_vae_decoder_loss`` (L1 / L2 of its UNet output against the colour latent of the
pseudo labels).  The reference runs it at one image per process only (it raises for B > 1); here every image gets its own
mask and its own pseudo labels in the masked CE -- the same values at B = 1 (masked image consistency).

Options of the reference that no shipped config enables (mask_diff, noise_reg, denoise_supervise, fd, fd_attention,
merge_with_pl_data, remove_amp / remove_texture, sem_seg_head_sec_modal=True, prompt masking) raise NotImplementedError.
``reg_uncertain`` only feeds the reference's visualisation (:327-333 -> vis_data :596-601); it changes nothing in a step
but the teacher call's ``return_unet_final_output`` (which the VAE-decoder branch computes anyway).

The periodic picture (``vis_period`` / ``output_dir``, :552-653 + cmdise.py:238-305): every ``vis_period`` iterations
``<output_dir>/vis_results/{iter:06d}_rank{local_rank}.png`` with the reference's tiles in its order, composed by one HIP
launch on the training stream and written in line or, with ``vis_async=True``, by a writer thread (vis.py; DESIGN.md, the periodic training picture).  The
reference's extra picture-only teacher pass (:603-644) runs too, with its generator draws and BatchNorm side effects.  Off
(``None`` / 0, the default) nothing is allocated, no generator is touched, no thread exists.
"""
import os
import random
import time
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

from . import augment, ops, labels as L, optim
from . import backward as bw
from .meta_arch import MadmInference
from .nn import Tok


class MTMADISE(MadmInference):
    psweight_ignore_top = 15          # cmdise.py:117

    def __init__(self, backbone, sem_seg_head, criterion, *, target_modality, train_palette, lora_configs=(),
                 vae_decoder_loss='', vae_decoder_loss_type=None, vae_decoder_loss_weight=(1.0, 1.0), reg_uncertain=False,
                 reg_target_palette=None, add_zero_grad=False, rev_noise_sup=False, rev_noise_end_iter=None,
                 rev_noise_gradually=False, denoise_timestep_range=None, eval_with_noise=None, max_iter=None,
                 sem_seg_head_sec_modal=False, ema_alpha=0.999, pseudo_threshold=0.968, blur=True, color_jitter_strength=0.2,
                 color_jitter_probability=0.2, enable_mixup=True, pl_crop=False, color_aug_flag=True, ema_w_unet=False,
                 pixel_mean=(0.0, 0.0, 0.0), pixel_std=(255.0, 255.0, 255.0), size_divisibility=64, color_aug=None,
                 mic=False, mask_ratio=None, mic_reg=False, MIC_reg_wo_pl_val=False, vis_period=None, output_dir=None,
                 vis_max_cols=5, vis_denorm=(0.5, 0.5), vis_async=False, **unsupported):
        for k, v in unsupported.items():
            if k in ("mask_diff", "noise_reg", "denoise_supervise", "fd", "fd_attention",
                     "merge_with_pl_data", "remove_amp", "remove_texture", "prompt_confidence",
                     "w_rgb_lora", "wo_lora") and v:
                raise NotImplementedError(f"MTMADISE option {k}={v!r}: no shipped config enables it (SURVEY.md App. C.11)")
        if sem_seg_head_sec_modal:
            raise NotImplementedError("sem_seg_head_sec_modal=True (a second head copy) is not built")
        assert not (mic and mic_reg), "mic and mic_reg exclude each other (mtmadise.py:78-81)"
        super().__init__(backbone, sem_seg_head, target_modality=target_modality, lora_configs=lora_configs,
                         pixel_mean=pixel_mean, pixel_std=pixel_std, size_divisibility=size_divisibility,
                         eval_with_noise=eval_with_noise)
        self.criterion = criterion
        self.train_iter_index = 0
        self.ema_alpha, self.pseudo_threshold = ema_alpha, pseudo_threshold
        # The EMA teacher's forward on a side stream beside the student's source pass: OFF by default since round 6.  Made race-free
        # (operands the teacher builds lazily on the side stream are ordered in front of main one by one: ops.side_builds), the
        # student trails the teacher layer by layer and the step is 0.4 .. 1.4 % SLOWER than in line (same box, three runs each:
        # 228.8 / 227.9 / 234.1 vs 225.7 / 224.4 / 233.1 ms, profiles/round6_ab_train_teacher_stream.txt); round 5's +1.5 % was
        # measured with the race in place.  MADM_TEACHER_OVERLAP=1 switches it on (tested: tests/test_train_gpu.py).
        self.overlap_teacher = bool(int(os.environ.get("MADM_TEACHER_OVERLAP", "0")))
        self._teacher_stream, self._teacher_warm = None, set()
        self.blur, self.color_jitter_strength, self.color_jitter_probability = blur, color_jitter_strength, color_jitter_probability
        self.enable_mixup, self.pl_crop, self.color_aug_flag = enable_mixup, pl_crop, color_aug_flag
        self.color_aug = color_aug        # callable(strong_parameters, data [N,3,H,W]) -> data; None: augment.strong_color
        self.vae_decoder_loss = vae_decoder_loss or ''
        self.vae_decoder_loss_type = vae_decoder_loss_type
        self.vae_decoder_loss_weight = list(vae_decoder_loss_weight)
        self.reg_uncertain, self.add_zero_grad = reg_uncertain, add_zero_grad
        self.rev_noise_sup, self.rev_noise_end_iter, self.rev_noise_gradually = rev_noise_sup, rev_noise_end_iter, rev_noise_gradually
        self.denoise_timestep_range = denoise_timestep_range
        self.train_max_iter = max_iter
        self.ema_w_unet = ema_w_unet
        # masked image consistency (cmdise.py:136-137,181-184; mtmadise.py:36,41,78-81): BlockMaskGenerator(ratio, 32)
        self.mic, self.mic_reg, self.MIC_reg_wo_pl_val = bool(mic), mic_reg, MIC_reg_wo_pl_val
        self.mask_ratio = 0.7 if mask_ratio is None else mask_ratio
        self.mask_block_size = 32
        self.deferred_mask_flags = None     # a list: the trainer collects the range flags of mask_image and raises at its end
        self.train_palette = L.pad_palette(train_palette)                       # mtmadise.py:97-99
        # the periodic picture (cmdise.py:212-215,231; mtmadise.py:552): None / 0 = off
        self.vis_period = int(vis_period) if vis_period else None
        if self.vis_period is not None and self.vis_period < 0:
            raise ValueError(f"vis_period must be a positive number of iterations (None / 0: off), got {vis_period!r}")
        if self.vis_period and not output_dir:
            raise ValueError("vis_period needs output_dir: the pictures go to <output_dir>/vis_results")
        self.output_dir, self.vis_max_cols = output_dir, int(vis_max_cols)
        if self.vis_max_cols < 1 or len(tuple(vis_denorm)) != 2:
            raise ValueError("vis_max_cols must be >= 1 and vis_denorm a (scale, shift) pair")
        self.vis_denorm = (float(vis_denorm[0]), float(vis_denorm[1]))
        self.vis_writer = self.last_vis = None
        # vis_async: the writer thread is off by default until tools/bench_vis.py has shown its training-thread cost below the
        # in-line host approach's on an MI355X (the periodic training picture: not measured yet)
        self._vis_classes = len(list(train_palette)) // 3      # reg_target_tensor is built from the UNPADDED palette (:92-94)
        self._vis_reg_target = None
        if self.vis_period:
            from . import vis, dist as _dist
            n_tiles = 8 + (2 if (mic or mic_reg) else 0) + sum(c in self.vae_decoder_loss for c in 'st') + \
                (3 if reg_uncertain else 0) + ((2 if 's' in self.vae_decoder_loss else 1) if rev_noise_sup else 0)
            if n_tiles > vis.MAX_TILES:
                raise ValueError(f"this configuration's picture has {n_tiles} tiles, a sheet holds {vis.MAX_TILES}: "
                                 "switch vis_period off or drop an option that only adds tiles")
            self.vis_writer = vis.VisWriter(output_dir, rank=_dist.env_world()[1], async_write=vis_async)
        if reg_target_palette is None:
            self.reg_target_palette = list(self.train_palette)
        else:
            assert reg_target_palette == 'discrete'
            self.reg_target_palette = L.pad_palette([255, 0, 255, 0, 255, 0, 127, 255, 127, 255, 127, 127, 0, 255, 255, 255,
                                                     255, 0, 0, 0, 255, 255, 0, 0, 127, 0, 127, 255, 255, 255, 0, 0, 0])
        self._inti_ema_weights()

    # ------------------------------------------------------------------ EMA teacher (cmdise.py:307-349)
    def _inti_ema_weights(self):
        bb = self.backbone
        bb.ema_feature_projections = deepcopy(bb.feature_projections)
        self.ema_sem_seg_head = deepcopy(self.sem_seg_head)
        self.ema_parms = [bb.ema_feature_projections, self.ema_sem_seg_head]
        self.updated_parms = [bb.feature_projections, self.sem_seg_head]
        ldm = bb.feature_extractor.ldm_extractor
        if self.ema_w_unet:
            ldm.ema_unet = deepcopy(ldm.unet)
            for m in ldm.ema_unet.modules():      # an EMA copy moves every step: no composed proj_out operand (sd_unet)
                if m.__class__.__name__ == "Transformer2DModel":
                    m.__dict__["weights_move"] = True
            self.ema_parms.append(ldm.ema_unet)
            self.updated_parms.append(ldm.unet)
        fe = bb.feature_extractor
        fe.ema_clip_project_others = deepcopy(fe.clip_project_others)
        self.ema_parms.append(fe.ema_clip_project_others)
        self.updated_parms.append(fe.clip_project_others)
        for m in self.ema_parms:
            for p in m.parameters():
                p.detach_()
                p.requires_grad = False
        # teacher parameters live in one flat buffer; student runs that are contiguous in an optimizer's flat buffer are
        # matched span-wise by optim.EmaPairs (a handful of launches per update instead of ~120 tiny ones)
        tp = [p for m in self.ema_parms for p in m.parameters()]
        sp = [p for m in self.updated_parms for p in m.parameters()]
        assert len(tp) == len(sp)
        self._ema_teacher_flat = optim.FlatParams(tp, with_grad=False) if tp and tp[0].is_cuda else None
        self._ema_pairs = optim.EmaPairs(tp, sp)

    def _update_ema(self, it):
        alpha_teacher = min(1 - 1 / (it + 1), self.ema_alpha)
        self._ema_pairs.update(alpha_teacher)

    # ------------------------------------------------------------------ helpers
    def _images(self, batched_inputs, key):
        """(x - pixel_mean) / pixel_std + ImageList zero padding to a multiple of 64 (:189-191,199-200)."""
        dev = next(self.parameters()).device
        xs = [x[key].to(dev).float() for x in batched_inputs]
        H, W = xs[0].shape[-2:]
        assert all(tuple(x.shape[-2:]) == (H, W) for x in xs), "training crops share one size (dataset mapper)"
        d = self.size_divisibility
        Hp, Wp = (H + d - 1) // d * d, (W + d - 1) // d * d
        return ops.scale_pad_nchw(torch.stack(xs).contiguous(), 1.0 / self.pixel_std, Hp, Wp)

    def _labels(self, batched_inputs):
        dev = next(self.parameters()).device
        g = torch.stack([x['source_label'].to(dev) for x in batched_inputs]).long()
        if g.dim() == 3:
            g = g[:, None]
        H, W = g.shape[-2:]
        d = self.size_divisibility
        assert H % d == 0 and W % d == 0, "label padding (ImageList pads labels with 0) is not needed by the shipped 512 crops"
        return g.contiguous()

    def _student_pass(self, img, input_modal, head=True):
        """backbone(img, return_unet_final_output=True, input_modal=...) + sem_seg_head, recorded for the backward:
        feature_extractor.py:156-170 -> ldm_base.py:832-924 -> ldm_diffusers.py:143-217 -> feature_extractor.py:367-396 ->
        daformer_head.py:702-749.
        Returns (logit tokens Tok, unet_final_output dict, record); ``head=False`` (the mic_reg pass): encoder and UNet only,
        no projections / head, logits None."""
        bb = self.backbone
        gen = bb.feature_extractor
        ldm = gen.ldm_extractor
        img = bb.preprocess_image(img)
        B = img.shape[0]
        project = gen.clip_project_rgb if input_modal == 'rgb' else gen.clip_project_others
        with torch.no_grad():
            cond_inputs, cond_emb = project(gen.uncond_inputs, None, repeat=B)
            batched = dict(img=img, cond_inputs=cond_inputs, cond_emb=cond_emb)
            st = ldm._stage_encode(batched)
            unet_tape = bw._Tape()
            feats, extra = ldm._stage_unet(st, batched, tape=unet_tape, _return_tokens=True, return_unet_final_output=True)
            proj_tape, head_tape, logits = None, None, None
            if head:
                proj_tape = []
                fd = bb.forward_features(feats, img.shape[-2:], tape=proj_tape)
                hd = self.sem_seg_head
                head_tape = {}
                toks = [fd['output_features'].tok[k] for k in hd.in_keys]
                logits = hd.forward_tokens(toks, tape=head_tape)
        no_grad_w = ()
        if ldm.vae_decoder_loss and not ldm.final_fuse_vae_decoder_feat:
            no_grad_w = (feats[0].W,)          # the decoder image is ``.detach()``ed (ldm_diffusers.py:196-201)
        rec = dict(unet_tape=unet_tape, proj_tape=proj_tape, head_tape=head_tape, project=project, B=B, no_grad_w=no_grad_w,
                   adapter=self.active_lora_adapter())     # the backward recomputes the fused LoRA operands: same adapter
        return logits, extra, rec

    def _color_latent(self, label, palette):
        """convert_label_to_rgb (:159-175) + vae_encoder(...)[0] (:253-254, 394-396)."""
        from .ldm_rocm import vae_encoder
        rgb, valid = L.convert_label_to_rgb(label, palette)
        lat = vae_encoder(vae=self.backbone.feature_extractor.ldm_extractor.vae, images=rgb, encoder_block_indices=[])[0]
        return lat, valid

    def _strong_color(self, strong_parameters, data, force=False):
        """``force``: the masked image's strong_transform call passes no color_aug_flag (mtmadise.py:406): always on."""
        if not (self.color_aug_flag or force):
            return data
        if self.color_aug is not None:
            return self.color_aug(strong_parameters, data)
        return augment.strong_color(strong_parameters, data)

    # ------------------------------------------------------------------ forward
    def forward(self, batched_inputs):
        if not self.training:
            return MadmInference.forward(self, batched_inputs)
        return self.forward_train(batched_inputs)

    def forward_train(self, batched_inputs):
        with ops.sync_profile():       # eager launches, one step in flight: the lone-launch rows of the tile table
            return self._forward_train(batched_inputs)

    def _forward_train(self, batched_inputs):
        if self.train_iter_index > 0:
            self._update_ema(self.train_iter_index)
        with torch.no_grad():
            source = self._images(batched_inputs, 'source_rgb')
            assert not isinstance(batched_inputs[0]['target_second_modality'], dict)
            target = self._images(batched_inputs, 'target_second_modality')
            gt = self._labels(batched_inputs)                                             # [B, 1, H, W] i64
        B = source.shape[0]
        tmod = self.target_modality
        strong_parameters = {
            'mix': None,
            'color_jitter': random.uniform(0, 1),
            'color_jitter_s': self.color_jitter_strength,
            'color_jitter_p': self.color_jitter_probability,
            'blur': random.uniform(0, 1) if self.blur else 0,
            'mean': None, 'std': None,          # pixel_mean == 0: aug_mean / aug_std are None (cmdise.py:236-238)
        }
        crit = self.criterion
        K = self.sem_seg_head.num_classes
        ctxs = {}

        # ---- teacher: pseudo labels ----
        # The EMA teacher's forward reads nothing the student passes write (its own UNet / head copies, the frozen VAE) and its
        # result is needed only where the labels are mixed: it runs on a side stream beside the two student forwards (from the
        # second step on: the first builds the shared packed operands of the frozen modules in one stream).  Same kernels,
        # same values; the Python-side random draws keep their order (random: two uniforms above, this randint; numpy: the
        # class choices below).
        main_stream = torch.cuda.current_stream(source.device)
        # ... per input geometry: a batch / crop size seen for the first time (a short last batch) runs in line, so whatever a
        # first pass at that size builds lazily is built in ONE stream; the shared constant caches are stream-safe on top of
        # that (ldm_rocm._StreamSafeCache: an entry filled on the side stream is waited for by its users on other streams)
        warm_key = (B, tuple(source.shape[-2:]), tuple(target.shape[-2:]))
        overlap = self.overlap_teacher and warm_key in self._teacher_warm
        side = main_stream
        if overlap:
            if self._teacher_stream is None:
                self._teacher_stream = torch.cuda.Stream(device=source.device)
            side = self._teacher_stream
            side.wait_stream(main_stream)                 # inputs, and this step's EMA update, are in front of it
        # (operands the teacher pass builds lazily on the side stream -- it shares the student's UNet unless ema_w_unet -- are
        # ordered in front of the main stream's passes one by one: ops.side_builds / ops.note_build)
        with torch.no_grad(), torch.cuda.stream(side), ops.side_builds(main_stream):
            self.set_lora_adapter(state=tmod)
            kw = dict(input_modal='others', ema_forward=True)
            if self.rev_noise_sup and self.train_iter_index <= self.rev_noise_end_iter:
                t_ = random.randint(self.denoise_timestep_range[0], self.denoise_timestep_range[1])
                if self.rev_noise_gradually:
                    t_ = int(t_ * (1 - self.train_iter_index / self.rev_noise_end_iter))
                kw['timestep'] = (t_, t_ + 1)
            pl_out = None
            if self.reg_uncertain:
                low_res_feats, pl_out = self.backbone(target, return_unet_final_output=True, **kw)
            else:
                low_res_feats = self.backbone(target, **kw)
            head_t = self.ema_sem_seg_head
            ema_logits = head_t.forward_tokens([low_res_feats['output_features'].tok[k] for k in head_t.in_keys])
            ema_nchw = ops.nhwc_to_nchw(ema_logits.t, B, K, ema_logits.H, ema_logits.W)
            pseudo_prob, pseudo_label, pseudo_weight = L.pseudo_labels(ema_nchw, target.shape[2:], self.pseudo_threshold)
            del low_res_feats, ema_logits
        self._teacher_warm.add(warm_key)

        # ---- source pass ('default' adapter, input_modal 'rgb') ----
        self.set_lora_adapter(state='default')
        source_logits, source_out, rec_s = self._student_pass(source, 'rgb')
        with torch.no_grad():
            if 's' in self.vae_decoder_loss:
                source_color_gt_latent, source_color_gt_mask = self._color_latent(gt, self.reg_target_palette)

            # ---- mixed image (ClassMix + colour augmentation) ----
            if self.enable_mixup:
                mix_classes = L.get_class_choices(gt)        # get_class_masks' RNG calls; the masks are re-derived per use
                mixed = []
                for i in range(B):
                    _, img_i, _ = L.class_mix(gt[i], mix_classes[i], source[i], target[i])
                    mixed.append(self._strong_color(strong_parameters, img_i[None]))
                mixed_img = torch.cat(mixed)
            else:
                mixed_img = self._strong_color(strong_parameters, target.clone())

        # ---- target pass on the mixed image ----
        self.set_lora_adapter(state=tmod)
        target_logits, target_out, rec_t = self._student_pass(mixed_img, 'mixed')

        # ---- masked image consistency: the masked pass (:404-420) -- reads nothing of the teacher, so it runs before the wait ----
        rec_m = masked_img = mask_u = mask_flag = None
        if self.mic or self.mic_reg:
            with torch.no_grad():
                strong_parameters['mix'] = None
                masked_img = self._strong_color(strong_parameters, target.clone(), force=True)   # torch jitter, numpy sigma
                masked_img, mask_u, mask_flag = augment.block_mask(masked_img, self.mask_ratio,
                                                                   self.mask_block_size)     # then the torch grid
            self.set_lora_adapter(state=tmod)
            masked_logits, masked_out, rec_m = self._student_pass(masked_img, 'others', head=bool(self.mic))

        # ---- label / weight mixing with the teacher's pseudo labels ----
        if overlap:
            main_stream.wait_stream(side)
            for t_side in (ema_nchw, pseudo_prob, pseudo_label, pseudo_weight):
                t_side.record_stream(main_stream)
        with torch.no_grad():
            # pseudo_val (:347-348) as a device scalar, taken before pl_crop zeroes the top rows of the weight
            pseudo_val = pseudo_weight.reshape(-1)[:1].clone() if self.mic_reg else None
            if self.pl_crop:
                pseudo_weight[:, :self.psweight_ignore_top, :] = 0
            if self.enable_mixup:
                gt_pixel_weight = torch.ones_like(pseudo_weight)
                lbls, wts = [], []
                for i in range(B):
                    _, w_i, l_i = L.class_mix(gt[i], mix_classes[i], gt_pixel_weight[i][None], pseudo_weight[i][None],
                                              label1=pseudo_label[i][None])
                    lbls.append(l_i)
                    wts.append(w_i)
                mixed_lbl = torch.stack(lbls)                                    # [B, 1, H, W]
                mixed_seg_weight = torch.cat(wts)                                # [B, H, W]
            else:
                mixed_lbl = pseudo_label[:, None]
                mixed_seg_weight = pseudo_weight
            if 't' in self.vae_decoder_loss:
                target_color_gt_latent, target_color_gt_mask = self._color_latent(mixed_lbl, self.reg_target_palette)
                target_color_gt_mask = target_color_gt_mask * pseudo_weight[:, None]
            if self.mic_reg:                                                              # :343-345
                pl_color_latent, _ = self._color_latent(pseudo_label[:, None], self.reg_target_palette)

            # ---- losses (criterion.py:155-254) ----
            losses = {}
            losses['source_loss'], ctxs['source_loss'] = crit.ce_forward(source_logits, K, gt[:, 0])
            losses['target_loss'], ctxs['target_loss'] = crit.ce_forward(target_logits, K, mixed_lbl[:, 0],
                                                                         pixel_weight=mixed_seg_weight)
            if 's' in self.vae_decoder_loss:
                losses['vae_decoder_source_loss'], ctxs['vae_decoder_source_loss'] = crit.decoder_loss_forward(
                    source_out['before_vae.decoder'], source_color_gt_latent, source_color_gt_mask,
                    self.vae_decoder_loss_weight[0], self.vae_decoder_loss_type)
            if 't' in self.vae_decoder_loss:
                losses['vae_decoder_target_loss'], ctxs['vae_decoder_target_loss'] = crit.decoder_loss_forward(
                    target_out['before_vae.decoder'], target_color_gt_latent, target_color_gt_mask,
                    self.vae_decoder_loss_weight[1], self.vae_decoder_loss_type)
            if self.mic:            # :471-476 -> criterion.py:211-218; per-image pseudo labels for B > 1
                losses['masked_prompt_consistency_loss'], ctxs['masked_prompt_consistency_loss'] = crit.ce_forward(
                    masked_logits, K, pseudo_label, pixel_weight=pseudo_weight)
            if self.mic_reg:        # :477-488 -> criterion.py:247-253
                pw = None if self.MIC_reg_wo_pl_val else pseudo_val
                losses['mic_vae_decoder_loss'], ctxs['mic_vae_decoder_loss'] = crit.mic_decoder_loss_forward(
                    masked_out['before_vae.decoder'], pl_color_latent, pw, self.mic_reg, self.vae_decoder_loss_type)
        if mask_flag is not None:   # mask_image's range assert: at the trainer's end-of-step sync, else here (one sync)
            if self.deferred_mask_flags is not None:
                self.deferred_mask_flags.append(mask_flag)
            else:
                augment.check_mask_flag(mask_flag)
        self.train_iter_index += 1

        names = list(losses.keys())
        params = [p for p in self.parameters() if p.requires_grad]
        zero_ids = set()
        if self.add_zero_grad:          # :654-655: ``sum(torch.sum(p)) * 0.`` over the LoRA tensors of the other adapters --
            losses['zero_grad'] = torch.zeros((), device=source.device)     # value 0, gradient 0 (not None) for each of them
            names.append('zero_grad')
            zero_ids = {id(p) for p in self.unused_lora_parameters(tmod) if p.requires_grad}
        state = dict(model=self, names=names, ctxs=ctxs, rec_s=rec_s, rec_t=rec_t, rec_m=rec_m, params=params,
                     zero_ids=zero_ids)
        self.last_step = dict(mixed_img=mixed_img, mixed_lbl=mixed_lbl, mixed_seg_weight=mixed_seg_weight,
                              pseudo_label=pseudo_label, pseudo_weight=pseudo_weight, ema_logits=ema_nchw,
                              source_logits=source_logits, target_logits=target_logits)
        if rec_m is not None:
            self.last_step.update(masked_img=masked_img, mask_grid=mask_u)
            if self.mic:
                self.last_step['masked_logits'] = masked_logits
        if self.vis_period and self.train_iter_index % self.vis_period == 0:
            if overlap and pl_out is not None:
                pl_out['after_vae.decoder'].record_stream(main_stream)
            self._vis_dump(source=source, target=target, gt=gt, source_out=source_out, target_out=target_out,
                           masked_out=masked_out if self.mic_reg else None, pl_out=pl_out, pseudo_prob=pseudo_prob,
                           pl_timestep=kw.get('timestep'))
        outs = _TrainStepFn.apply(state, len(names), *[losses[n] for n in names], *params)
        return dict(zip(names, outs))

    # ------------------------------------------------------------------ the periodic picture (mtmadise.py:552-653)
    def _vis_logits(self, tok):
        """Head output tokens -> f32 [B, K, h, w] (the sheet's kernel resizes and takes the argmax)."""
        K = self.sem_seg_head.num_classes
        return ops.nhwc_to_nchw(tok.t, tok.B, K, tok.H, tok.W)

    def vis_tiles(self, *, source, target, gt, source_out, target_out, masked_out, pl_out, pseudo_prob, pl_timestep):
        """The reference's ``vis_data`` (:559-601) in its order, from what the step already holds (``last_step`` + the
        decoder outputs).  Decoder images stay in [-1, 1] and carry their own (0.5, 0.5) denorm: the reference's
        ``(x + 1) / 2``.  The pseudo-label tile is drawn from ``pseudo_label`` itself -- the argmax of the up-sampled teacher
        logits that the step trained on, the same picture as the reference's logits tile."""
        ls = self.last_step
        pl_info = 'target_sec_modal_pl'
        if pl_timestep is not None and self.train_iter_index <= self.rev_noise_end_iter:      # :556-557, after the += 1
            pl_info += '_{}_t'.format(pl_timestep[0])
        half = (0.5, 0.5)
        tiles = [
            dict(data_type='image', info='source_rgb', data=source),
            dict(data_type='logits', info='source_pred', data=self._vis_logits(ls['source_logits'])),
            dict(data_type='label', info='source_label', data=gt),
            dict(data_type='image', info='target_sec_modal', data=target),
            dict(data_type='label', info=pl_info, data=ls['pseudo_label']),
            dict(data_type='image', info='mixup_modal', data=ls['mixed_img']),
            dict(data_type='logits', info='mixup_pred', data=self._vis_logits(ls['target_logits'])),
            dict(data_type='label', info='mixup_label', data=ls['mixed_lbl']),
        ]
        if self.mic or self.mic_reg:                                  # :571-576
            tiles.append(dict(data_type='image', info='masked_image', data=ls['masked_img']))
            if self.mic:
                tiles.append(dict(data_type='logits', info='masked_image_pred', data=self._vis_logits(ls['masked_logits'])))
            else:
                tiles.append(dict(data_type='image', info='masked_vae_decoder_out', data=masked_out['after_vae.decoder'],
                                  denorm=half))
        if 's' in self.vae_decoder_loss:
            tiles.append(dict(data_type='image', info='source_vae_decoder_out', data=source_out['after_vae.decoder'],
                              denorm=half))
        if 't' in self.vae_decoder_loss:
            tiles.append(dict(data_type='image', info='target_vae_decoder_out', data=target_out['after_vae.decoder'],
                              denorm=half))
        if self.reg_uncertain:                                        # :329-333, 596-601
            if self._vis_reg_target is None:
                pal = torch.tensor(self.train_palette[:3 * self._vis_classes], dtype=torch.float32, device=source.device)
                self._vis_reg_target = (pal / 255.0).reshape(self._vis_classes, 3).t().reshape(1, 3, -1, 1, 1).contiguous()
            after01 = (pl_out['after_vae.decoder'] + 1) / 2
            prob_reg = 1 / (torch.norm(after01[:, :, None] - self._vis_reg_target, dim=1) + 1e-3)
            pseudo_prob_reg = torch.softmax(prob_reg, dim=1).max(dim=1)[0]
            tiles += [dict(data_type='logits', info='pl_reg', data=prob_reg),
                      dict(data_type='heatmap', info='pl_prob_reg', data=pseudo_prob_reg),
                      # the share of confident pixels stays a device scalar: the writer thread formats the title
                      dict(data_type='heatmap', info='pl_prob_{:.3f}', data=pseudo_prob,
                           info_value=ls['pseudo_weight'].reshape(-1)[-1:].clone())]
        return tiles

    def _vis_extra_pass(self, target):
        """The reference's picture-only pass (:603-644): the STUDENT backbone under the target adapter and the EMA head on
        the target image -- without noise up to ``rev_noise_end_iter``, afterwards at a ``random.randint`` timestep of
        ``denoise_timestep_range``.  Its generator draws (noise, dropout, that randint) and the BatchNorm statistics it moves
        are the reference's."""
        if not self.rev_noise_sup:
            return []
        kw, tag = dict(input_modal='others'), 'no_noise_t'
        if self.train_iter_index > self.rev_noise_end_iter:
            t_ = random.randint(self.denoise_timestep_range[0], self.denoise_timestep_range[1])
            kw['timestep'] = (t_, t_ + 1)
            tag = 'noise_{}_t'.format(t_)
        tiles = []
        self.set_lora_adapter(state=self.target_modality)
        if 's' in self.vae_decoder_loss:
            feats, out = self.backbone(target, return_unet_final_output=True, **kw)
            tiles.append(dict(data_type='image', info=tag + '_reg', data=out['after_vae.decoder'], denorm=(0.5, 0.5)))
        else:
            feats = self.backbone(target, **kw)
        head_t = self.ema_sem_seg_head
        logits = head_t.forward_tokens([feats['output_features'].tok[k] for k in head_t.in_keys])
        tiles.append(dict(data_type='logits', info=tag + '_pred', data=self._vis_logits(logits)))
        return tiles

    def _vis_dump(self, **held):
        from . import vis
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t0 = time.perf_counter()
        with torch.no_grad():
            ev[0].record()
            extra = self._vis_extra_pass(held['target'])
            ev[1].record()
            t1 = time.perf_counter()
            tiles = self.vis_tiles(**held) + extra
            canvas = self.vis_writer.submit(self.train_iter_index, tiles, cols_max=self.vis_max_cols,
                                            palette=self.train_palette, denorm=self.vis_denorm)
            ev[2].record()
        B = held['source'].shape[0]
        H, W = held['source'].shape[-2:]
        # kept until the next dump.  For tools: ``events`` = (start, picture-only pass done, sheet composed) on the training
        # stream, ``host_ms`` = what the call cost the training thread (picture-only pass, tile list + submit)
        self.last_vis = dict(iteration=self.train_iter_index, infos=[t['info'] for t in tiles], canvas=canvas,
                             meta=vis.VisWriter.describe(tiles, B, H, W, self.vis_max_cols),
                             path=self.vis_writer.path(self.train_iter_index), events=ev,
                             host_ms=((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))

    def unused_lora_parameters(self, used_modal):
        """The tensors ``add_zero_gead_on_unused_lora`` sums (mtmadise.py:149-157): every UNet parameter whose name holds
        'lora' but not the target modality -- the 'default' adapter included."""
        unet = self.backbone.feature_extractor.ldm_extractor.unet
        return [p for name, p in unet.named_parameters() if 'lora' in name and used_modal not in name]

    def add_zero_gead_on_unused_lora(self, used_modal):
        """The reference's own formulation through torch autograd (kept for callers outside ``forward_train``, which
        folds the term into its autograd node: value 0, zero gradients, the tensors count as touched for AdamW)."""
        loss = [torch.sum(p) for p in self.unused_lora_parameters(used_modal)]
        return sum(loss) * 0.

    # ------------------------------------------------------------------ backward of one recorded student pass
    def _backward_pass(self, rec, dlogits, dsample, add):
        """dlogits: tokens [M, k_tile] (compute dtype) or None; dsample: NCHW f32 gradient of 'before_vae.decoder' or None;
        ``add(param, grad)`` accumulates a parameter gradient (called in the order the backward produces them: head,
        projections, UNet up -> mid -> down -> conv_in, batched K/V and time-embedding tails, prompt / time gates)."""
        bb = self.backbone
        gen = bb.feature_extractor
        self.set_lora_adapter(rec["adapter"])
        tape = rec["unet_tape"]
        unet = tape.unet
        dins = {}
        if dlogits is not None:
            head = self.sem_seg_head
            dfeats, hg = head.backward_tokens(rec["head_tape"], dlogits)
            hp = dict(head.named_parameters())
            for k_, v in hg.items():
                add(hp[k_], v)
            dins, pg = bb.backward_features(rec["proj_tape"], dict(zip(head.in_keys, dfeats)), no_grad_inputs=rec["no_grad_w"])
            bp = dict(bb.named_parameters())
            for k_, v in pg.items():
                add(bp[k_], v)
        dtaps = []
        for tk in tape.tapped:
            d = dins.get(tk.W)
            if d is None:
                d = torch.zeros_like(tk.t)
            dtaps.append(d if d.shape[1] == tk.C else d[:, :tk.C].contiguous())
        ds = None
        if dsample is not None:
            ds = bw.sample_grad_tokens(unet, dsample, tape.sample.t.dtype)
        up = dict(unet.named_parameters())

        def unet_grad(k_, v):
            p = up.get(k_)
            if p is not None and p.requires_grad:
                add(p, v)

        res = bw.unet_backward_from_state(tape, dtaps, dsample=ds, base_grads=bw.wants_base_grads(unet),
                                          grad_cb=unet_grad)
        # prompt / time conditioning
        project = rec["project"]
        if any(p.requires_grad for p in project.parameters()):
            dctx = bw.prompt_grad(res["ctx"], (rec["B"], -1, gen.uncond_inputs.shape[2]))
            pg = project.backward(gen.uncond_inputs, dctx.contiguous(), res["cond_emb"])
            pp = dict(project.named_parameters())
            for k_, v in pg.items():
                add(pp[k_], v)


class _TrainStepFn(torch.autograd.Function):
    """The whole training forward as ONE autograd node: outputs = the loss scalars the HIP forward computed, inputs = every
    trainable parameter; backward = the explicit gradient kernels over the two (three with masked image consistency)
    recorded student passes, each loss weighted
    by the gradient that reaches it (sum of the losses, GradScaler scale, per-loss weights -- all stay device scalars)."""

    @staticmethod
    def forward(ctx, state, n_losses, *rest):
        ctx.state = state
        ctx.n_losses = n_losses
        return tuple(v.clone() for v in rest[:n_losses])

    @staticmethod
    def backward(ctx, *gouts):
        with ops.sync_profile():
            return _TrainStepFn._backward(ctx, *gouts)

    @staticmethod
    def _backward(ctx, *gouts):
        st = ctx.state
        model, names, ctxs, params = st["model"], st["names"], st["ctxs"], st["params"]
        crit = model.criterion
        g = {n: (go if go is not None else None) for n, go in zip(names, gouts)}
        acc = {}
        touched = set()
        early = set()
        sink = getattr(model, "grad_sink", None)     # train.MadmTrainer: gradients go straight into its flat buffer and
        passes = []                                  # finished spans are all-reduced while the backward still runs
        dtype = st["rec_s"]["unet_tape"].sample.t.dtype
        for rec, ce_name, dec_name in ((st["rec_s"], 'source_loss', 'vae_decoder_source_loss'),
                                       (st["rec_t"], 'target_loss', 'vae_decoder_target_loss'),
                                       (st["rec_m"], 'masked_prompt_consistency_loss', 'mic_vae_decoder_loss')):
            if rec is None:
                continue
            if (ce_name in ctxs and g.get(ce_name) is not None) or (dec_name in ctxs and g.get(dec_name) is not None):
                passes.append((rec, ce_name, dec_name))
        # gradient sink: a parameter's span is finished by the LAST pass that runs (final); the earlier ones accumulate, and
        # what only they touched is finished after the walk
        for i, (rec, ce_name, dec_name) in enumerate(passes):
            last = i == len(passes) - 1

            def add(p, v, last=last):
                v = v.reshape(p.shape)
                touched.add(id(p))
                if sink is not None:                 # straight into the trainer's flat buffer (batched adds); the LAST
                    if last:                         # pass marks the parameter's span as finished
                        early.discard(id(p))
                        sink.final(p, v)
                    else:
                        early.add(id(p))
                        sink.accumulate(p, v)
                    return
                cur = acc.get(id(p))
                acc[id(p)] = v if cur is None else cur + v

            dlogits = None
            if ce_name in ctxs and g.get(ce_name) is not None:
                dlogits = crit.ce_backward(ctxs[ce_name], g[ce_name], dtype)
            dsample = None
            if dec_name in ctxs and g.get(dec_name) is not None:
                dsample = crit.decoder_loss_backward(ctxs[dec_name], g[dec_name])
            ops.GRAD_ZEROS.reset(dlogits.device if dlogits is not None else dsample.device)   # one memset per pass
            adapter_now = model.active_lora_adapter()
            try:
                model._backward_pass(rec, dlogits, dsample, add)
            finally:
                model.set_lora_adapter(adapter_now)
            if sink is not None:
                sink.flush()
        ops.GRAD_ZEROS.drop()
        if g.get('zero_grad') is not None:     # zero gradients of the other adapters' LoRA tensors: present, not None
            for p in params:
                if id(p) in st["zero_ids"] and id(p) not in touched:
                    touched.add(id(p))
                    if sink is None:
                        acc[id(p)] = torch.zeros_like(p)
                    else:
                        early.add(id(p))       # the flat gradient buffer is already zero: only mark the span finished
        st["rec_s"] = st["rec_t"] = st["rec_m"] = None       # free the tapes
        model.last_grad_param_ids = touched    # torch.optim.AdamW skips parameters whose grad is None
        if sink is not None:
            for p in params:                   # gradients only the first pass produced: already added, now finished
                if id(p) in early:
                    sink.final(p, None)
            sink.backward_done()
            return (None, None) + (None,) * ctx.n_losses + (None,) * len(params)
        return (None, None) + (None,) * ctx.n_losses + tuple(acc.get(id(p)) for p in params)
