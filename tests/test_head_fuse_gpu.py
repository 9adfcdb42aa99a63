"""``DAFormerHead(final_fuse_vae_decoder_feat=True)`` on the GPU: the fused upsample + concat + classifier kernel of
libmadm_headfuse.so and the composed path (resize + two-source conv) it replaces, on lattice inputs (torch.equal with the exact
float64 result), on random inputs (a derived per-element bound) and inside NaN-canaried strided windows; the 128 -> 32 -> 64
GroupNorm bottleneck alone; the head against the fixtures the reference's own class produced (tests/golden/headfuse_*.npz); one
training step and one graphed inference forward of the whole model with a flagged head."""
import random

import numpy as np
import pytest
import torch

import head_fuse_util as hu
from util import to_tokens, from_tokens, rel_err
from window_util import Guarded, layout

pytestmark = pytest.mark.gpu
DT3 = [torch.float32, torch.bfloat16, torch.float16]
ID3 = ["f32", "bf16", "f16"]
KERNEL_CASES = [(h, w, k) for (h, w) in hu.KERNEL_SIZES for k in hu.KERNEL_KS]
KERNEL_IDS = [f"{h}x{w}-K{k}" for h, w, k in KERNEL_CASES]


def _tok(x, dtype):
    """[B, H, W, C] float64 (CPU) -> [B*H*W, C] device tokens"""
    return x.reshape(-1, x.shape[-1]).to(dtype).contiguous().cuda()


def _fused(hd, proj, w, bias, B, h, wl, out=None):
    from madm_amd import ops
    return ops.upsample_cat_classify(hd, proj, w, bias, B, h, wl, out=out)


def _composed(hd, proj, w, bias, B, h, wl):
    from madm_amd import ops
    up = ops.resize_bilinear(hd, B, h, wl, 2 * h, 2 * wl)
    return ops.conv2d(up, w, B, 2 * h, 2 * wl, N=w.shape[0], x2=proj, bias=bias, out_f32=True)


def _operands(case, dtype):
    hd, proj, wt, bias = case
    return _tok(hd, dtype), _tok(proj, dtype), wt.to(dtype).contiguous().cuda(), bias.float().contiguous().cuda()


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=KERNEL_IDS)
def test_lattice_inputs_give_the_exact_result(cuda, dtype, case):
    """Every value either path forms is an integer its type holds and every partial sum is below 2^24 (checked on the host by
    tests/test_head_fuse_host.py): both paths must produce THE float64 result, every padded class column zero."""
    h, w, k = case
    data = hu.lattice_case(h, w, k)
    want = hu.check_exact(*data).reshape(-1, hu.kp_of(k)).float()
    ops_ = _operands(data, dtype)
    for name, fn in (("fused", _fused), ("composed", _composed)):
        got = fn(*ops_, hu.KERNEL_B, h, w).cpu()
        assert got.dtype == torch.float32 and torch.equal(got, want), \
            f"{name}: {(got != want).sum().item()} of {want.numel()} elements differ, worst {(got - want).abs().max().item()}"
        assert not got[:, k:].any()


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=KERNEL_IDS)
def test_random_inputs_meet_the_per_element_bound(cuda, dtype, case):
    """head_fuse_util.classify_bound: 7 f32 roundings of the blend, ONE rounding of the blended value to the compute dtype,
    C1 + C2 + 1 f32 additions at a whole ulp each -- against float64 on inputs already rounded to the dtype."""
    h, w, k = case
    data = hu.random_case(h, w, k, dtype)
    want = hu.classify_ref(*data, dtype).reshape(-1, hu.kp_of(k))
    bound = hu.classify_bound(*data, dtype).reshape(-1, hu.kp_of(k))
    ops_ = _operands(data, dtype)
    for name, fn in (("fused", _fused), ("composed", _composed)):
        got = fn(*ops_, hu.KERNEL_B, h, w).cpu().double()
        ratio = ((got - want).abs() / bound.clamp(min=1e-300))[:, :k]
        print(f"{name} {h}x{w} K{k}: worst |error| / bound {ratio.max().item():.3f}")
        assert float(ratio.max()) <= 1.0, (name, float(ratio.max()))
        assert not got[:, k:].any()


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("kind", ["tight", "wide"])
@pytest.mark.parametrize("case", [(3, 5, 11), (17, 9, 19)], ids=["3x5-K11", "17x9-K19"])
def test_strided_windows_keep_their_canaries(cuda, dtype, kind, case):
    """hd, proj and the output inside windows of larger NaN-filled buffers: nothing outside the output window is written, no NaN
    is read into the result, and the result equals the dense run bit for bit."""
    h, w, k = case
    B, kp = hu.KERNEL_B, hu.kp_of(k)
    hd, proj, wt, bias = _operands(hu.random_case(h, w, k, dtype), dtype)
    dense = _fused(hd, proj, wt, bias, B, h, w)
    epc = 4 if dtype == torch.float32 else 8
    g_hd = Guarded(hd.shape[0], hu.C1, dtype, **dict(zip(("ld", "c0"), layout(kind, hu.C1, epc))))
    g_pr = Guarded(proj.shape[0], hu.C2, dtype, **dict(zip(("ld", "c0"), layout(kind, hu.C2, epc))))
    g_w = Guarded(kp, hu.C1 + hu.C2, dtype, **dict(zip(("ld", "c0"), layout(kind, hu.C1 + hu.C2, epc))))
    g_out = Guarded(dense.shape[0], kp, torch.float32, **dict(zip(("ld", "c0"), layout(kind, kp, 4))))
    got = _fused(g_hd.load(hd), g_pr.load(proj), g_w.load(wt), bias, B, h, w, out=g_out.view)
    torch.cuda.synchronize()
    for g, what in ((g_hd, "hd"), (g_pr, "proj"), (g_w, "w"), (g_out, "out")):
        g.check(what)
    assert not torch.isnan(got).any() and torch.equal(got, dense)


# ---- the 128 -> 32 -> 64 GroupNorm bottleneck ----------------------------------------------------------------------------------
def _blocks():
    from madm_amd import weights
    from madm_amd.head import NarrowBottleneckBlock
    from oracle import third_party as tp
    blk = weights.synth_init_(NarrowBottleneckBlock(128, 64, bottleneck_channels=32), 5, "p.").cuda()
    ref = weights.synth_init_(tp.BottleneckBlock(128, 64, bottleneck_channels=32, norm="GN"), 5, "p.").eval()
    assert {k: tuple(v.shape) for k, v in blk.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    return blk, ref


# |g| of a whole tensor / worst element of a small tensor: the gates of tests/test_train_gpu.py::test_train_step_matches_fixture
NTOL = {torch.float32: 2e-3, torch.float16: 4e-2, torch.bfloat16: 8e-2}
ETOL = {torch.float32: 1e-2, torch.float16: 5e-1, torch.bfloat16: 1.0}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", [(6, 10), (34, 18)], ids=["6x10", "34x18"])
def test_narrow_bottleneck_block(cuda, dtype, hw):
    """GroupNorm(32 groups) over 32 and 64 channels -- one and two channels per group -- in the statistics, the norm folded into
    the 3x3 conv and groupnorm_backward; forward at the gates of test_eval_gpu.py::test_bottleneck_block, backward at the
    training step's gradient gates."""
    from madm_amd.nn import Tok
    H, W = hw
    blk, ref = _blocks()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 128, H, W), generator=g)
    dy = torch.randn((2, 64, H, W), generator=g)
    if dtype == torch.bfloat16:
        x, dy = x.to(dtype).float(), dy.to(dtype).float()
    xr = x.clone().requires_grad_(True)
    want = ref(xr)
    want.backward(dy)
    tape = []
    got = blk(Tok(to_tokens(x, dtype), 2, H, W), tape=tape)
    e, l2 = rel_err(from_tokens(got.t, 2, H, W), want.detach())
    print(f"forward {e:.2e} {l2:.2e}")
    assert e < (3e-5 if dtype == torch.float32 else 3e-2), f"{e:.2e} {l2:.2e}"
    dx, grads = blk.backward(tape[0], to_tokens(dy, dtype))
    params = dict(ref.named_parameters())
    assert set(grads) == set(params)
    rows = [("dx", from_tokens(dx, 2, H, W), xr.grad)] + [(n, grads[n].float().cpu(), params[n].grad) for n in sorted(params)]
    for n, a, b in rows:
        assert tuple(a.shape) == tuple(b.shape), (n, a.shape, b.shape)
        ne = abs(a.double().norm().item() - b.double().norm().item()) / b.double().norm().item()
        ee = rel_err(a, b)[0]
        print(f"   {n}: |g| {ne:.2e} worst element {ee:.2e}")
        assert ne < NTOL[dtype] and ee < ETOL[dtype], (n, ne, ee)


# ---- the head against the reference's fixtures ---------------------------------------------------------------------------------
def _head(flag=True, K=hu.K):
    from madm_amd.head import DAFormerHead
    from oracle import madm_path
    head = DAFormerHead(in_channels=list(hu.CHANNELS), in_keys=list(hu.KEYS), in_index=[0, 1, 2, 3], channels=256, num_classes=K,
                        norm_cfg=dict(type='BN'), decoder_params=madm_path.head_decoder_params(),
                        final_fuse_vae_decoder_feat=flag)
    return hu.init_head_(head).cuda()


def _toks(feats, dtype):
    from madm_amd.nn import Tok
    return [Tok(to_tokens(feats[k], dtype), feats[k].shape[0], feats[k].shape[2], feats[k].shape[3]) for k in hu.KEYS]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,route", [("headfuse_eval", "fused"), ("headfuse_eval_odd", "fused"),
                                        ("headfuse_eval_odd_s0", "composed")])
def test_eval_head_matches_the_reference_fixture(cuda, dtype, name, route):
    """Gates of test_eval_gpu.py::test_daformer_head_small.  64 x 64 and 72 x 40 halve exactly and take the fused kernel (the
    72 x 40 case again through the composed path), 71 x 39 does not and takes the composed path: the route is asserted."""
    gold = torch.from_numpy(hu.load_fixture(name)["logits"])
    head = _head().eval()
    toks = _toks(hu.case_feats(name), dtype)
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    for force_composed in (False, True):
        head.fused_classifier = not force_composed
        lg = head.forward_tokens(toks)
        assert head.last_route == ("composed" if force_composed else route)
        got = from_tokens(lg.t[:, :hu.K], lg.B, lg.H, lg.W)
        e, l2 = rel_err(got, gold)
        print(f"{name} {head.last_route}: {e:.2e} {l2:.2e}")
        assert got.shape == gold.shape and e < tol, f"{head.last_route}: {e:.2e} {l2:.2e}"


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_train_head_matches_the_reference_fixture(cuda, dtype):
    """Train mode, B = 2, the fixture's Dropout2d scale and dlogits: logits, the 46 parameter gradients, the four feature
    gradients and the BatchNorm running statistics at the gates test_train_step_matches_fixture holds the same quantities to
    (16-bit modes with its loss scale of 4096)."""
    from madm_amd import ops
    name = "headfuse_train"
    gold = hu.load_fixture(name)
    head = _head().train()
    head.dropout_scale_override = hu.case_dropout_scale(name)
    feats = hu.case_feats(name)
    toks = _toks(feats, dtype)
    tape = {}
    lg = head.forward_tokens(toks, tape=tape)
    assert head.last_route == "composed"          # the taped forward keeps the upsampled operand for the backward
    f32 = dtype == torch.float32
    e, l2 = rel_err(from_tokens(lg.t[:, :hu.K], lg.B, lg.H, lg.W), torch.from_numpy(gold["logits"]))
    print(f"logits {e:.2e} {l2:.2e}")
    assert (e < 1e-3) if f32 else (l2 < (2e-2 if dtype == torch.float16 else 1e-1)), (e, l2)
    gscale = 1.0 if f32 else 4096.0
    dl = to_tokens(hu.case_dlogits(name) * gscale, dtype, cpad=ops.k_tile(dtype))
    dfeats, grads = head.backward_tokens(tape, dl)
    params = dict(head.named_parameters())
    assert set(grads) == set(params) and len(params) == 46
    worst = []
    for n, g in grads.items():
        assert tuple(g.shape) == tuple(params[n].shape), (n, g.shape)
        got, gn = hu.sample(g.float().cpu() / gscale)
        ref, rn = gold["grad:" + n], float(gold["gnorm:" + n])
        ne, ee = abs(gn - rn) / rn, rel_err(torch.from_numpy(got), torch.from_numpy(ref))[0]
        worst.append((ne, ee, n))
        assert ne < NTOL[dtype] and ee < ETOL[dtype], (n, ne, ee)
    for k, f, d in zip(hu.KEYS, toks, dfeats):
        got, gn = hu.sample(from_tokens(d[:, :f.C], f.B, f.H, f.W) / gscale)
        ref, rn = gold["dfeat:" + k], float(gold["dfnorm:" + k])
        ne, ee = abs(gn - rn) / rn, rel_err(torch.from_numpy(got), torch.from_numpy(ref))[0]
        worst.append((ne, ee, "dfeat:" + k))
        assert ne < NTOL[dtype] and ee < ETOL[dtype], (k, ne, ee)
    print("worst |g|", max(worst)[::2], "worst element", max(worst, key=lambda r: r[1])[1:])
    if f32:
        bufs = dict(head.named_buffers())
        for k in gold:
            if k.startswith("bn:"):
                assert rel_err(bufs[k[3:]].cpu(), torch.from_numpy(gold[k]))[0] < 1e-4, k


def test_flag_off_head_is_untouched_by_a_flagged_one(cuda):
    """The unflagged head gives the same bits before and after a flagged head ran in the process (fused and composed route)."""
    dtype = torch.float16
    feats = hu.case_feats("headfuse_eval")
    toks = _toks(feats, dtype)
    plain = _head(flag=False).eval()
    assert "vae_decoder_feat_proj" not in dict(plain.named_modules()) and plain.conv_seg.weight.shape[1] == 256
    before = plain.forward_tokens(toks).t.clone()
    assert plain.last_route is None
    flagged = _head().eval()
    for fused in (True, False):
        flagged.fused_classifier = fused
        flagged.forward_tokens(toks)
    after = plain.forward_tokens(toks).t
    assert torch.equal(before, after)


# ---- the whole model -----------------------------------------------------------------------------------------------------------
def _backbone(dtype, size, finetune_unet="all"):
    from madm_amd.ldm_rocm import LdmRocm
    from madm_amd.backbone import BasePromptTimeGenerator, AttentionFeatureExtractorBackbone
    from oracle import madm_path
    cfg = madm_path.DEPTH_CFG
    ldm = LdmRocm("", encoder_block_indices=[], unet_block_indices=[5, 8, 11], decoder_block_indices=(), input_range='-1+1',
                  unet_block_indices_type='after', finetune_unet=finetune_unet, compute_dtype=dtype, weights='synthetic', seed=0,
                  vae_decoder_loss=True)
    gen = BasePromptTimeGenerator(learnable_cond_prompt=True, learnable_cond_time=True, clip_state='no', num_timesteps=1,
                                  clip_model_name="ViT-L-14-336", ldm_extractor=ldm, same_cond_params=True)
    return AttentionFeatureExtractorBackbone(
        attention_features_res=None, feature_dims=list(cfg["feature_dims"]), projection_dim=list(cfg["projection_dim"]),
        attention_features_location=None, feature_extractor=gen, num_res_blocks=1, out_features=list(cfg["out_features"]),
        backbone_in_size=(size, size))


def _flagged_head():
    from madm_amd.head import DAFormerHead
    from oracle import madm_path
    return DAFormerHead(in_channels=list(hu.CHANNELS), in_keys=list(hu.KEYS), in_index=[0, 1, 2, 3], channels=256,
                        dropout_ratio=0.1, num_classes=hu.K, norm_cfg=dict(type='BN'), align_corners=False,
                        decoder_params=madm_path.head_decoder_params(), final_fuse_vae_decoder_feat=True)


def _train_model(dtype, n_steps=1):
    """MTMADISE of the Depth config at the size of test_train_step_matches_fixture, with a flagged head and the fixture's
    injected Dropout2d scales for ``n_steps`` steps."""
    from golden_util import TRAIN_CASE, init_eval_params, train_palette, train_dropout_scales, model_args
    from madm_amd.criterion import CmdiseCriterion
    from madm_amd.mtmadise import MTMADISE
    backbone, head = _backbone(dtype, TRAIN_CASE["size"]), _flagged_head()
    init_eval_params(backbone, head)
    args = dict(target_modality="Depth", train_palette=train_palette(hu.K), vae_decoder_loss='st', vae_decoder_loss_type='L1',
                vae_decoder_loss_weight=[1.0, 1.0], reg_uncertain=True, rev_noise_sup=True, rev_noise_end_iter=5000,
                rev_noise_gradually=True, denoise_timestep_range=[60, 61], max_iter=10000,
                pseudo_threshold=TRAIN_CASE["pseudo_threshold"], color_aug_flag=False)
    args.update(model_args("train_depth"))
    model = MTMADISE(backbone.cuda(), head.cuda(), CmdiseCriterion(num_classes=hu.K), **args).train()
    sc = train_dropout_scales(TRAIN_CASE["B"])
    model.sem_seg_head.dropout_scale_override = [sc[0], sc[1]] * n_steps
    model.ema_sem_seg_head.dropout_scale_override = [sc[2]] * n_steps
    random.seed(TRAIN_CASE["py_seed"])
    np.random.seed(TRAIN_CASE["np_seed"])
    return model


def test_training_step_with_a_flagged_head_is_reproducible(cuda):
    """One MTMADISE step at the size of test_train_step_matches_fixture: it runs, leaves a gradient on every trainable
    parameter (the EMA teacher carries the new parameters too), and under deterministic=True a second model built the same
    way reproduces every loss and gradient bit for bit."""
    from golden_util import TRAIN_CASE, train_inputs
    from madm_amd import ops

    def step():
        model = _train_model(torch.float16)
        losses = model(train_inputs(**TRAIN_CASE))
        (sum(losses.values()) * 4096.0).backward()
        torch.cuda.synchronize()
        return model, {k: v.detach().clone() for k, v in losses.items()}

    with ops.deterministic():
        m1, l1 = step()
        names = {n for n, _ in m1.sem_seg_head.named_parameters()}
        assert {n for n in names if n.startswith("vae_decoder_feat_proj.0.")} and len(names) == 46
        assert {n for n, _ in m1.ema_sem_seg_head.named_parameters()} == names
        missing = [n for n, p in m1.named_parameters() if p.requires_grad and p.grad is None]
        assert not missing, missing[:8]
        for n, p in m1.sem_seg_head.named_parameters():
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
        g1 = {n: p.grad.clone() for n, p in m1.named_parameters() if p.grad is not None}
        del m1
        m2, l2 = step()
    assert all(torch.equal(l1[k], l2[k]) for k in l1), (l1, l2)
    bad = [n for n, p in m2.named_parameters() if p.grad is not None and not torch.equal(p.grad, g1[n])]
    assert not bad, bad[:8]


def test_trainer_steps_move_the_new_parameters_and_their_derived_operands(cuda):
    """MadmTrainer (flat optimizer storage, AdamW, EMA update) over a flagged head: the twelve new tensors and the 320-wide
    classifier are stepped like every other head parameter, the teacher's copies follow through the EMA, the model's
    state_dict carries them for both heads, and the operands derived from them (the padded twin of the narrow bottleneck, the
    packed classifier) are re-derived after the step: an eval forward equals that of a fresh head loaded with the stepped
    state."""
    from golden_util import TRAIN_CASE, train_inputs
    from madm_amd.train import MadmTrainer
    model = _train_model(torch.float32, n_steps=2)
    trainer = MadmTrainer(model, lr=1e-3, weight_decay=0.05, grad_clip=None, amp=False)
    head, ema = model.sem_seg_head, model.ema_sem_seg_head
    new = [n for n, _ in head.named_parameters() if n.startswith(("vae_decoder_feat_proj.0.", "conv_seg."))]
    assert len(new) == 14
    before = {n: p.detach().clone() for n, p in head.named_parameters()}
    ema_before = {n: p.detach().clone() for n, p in ema.named_parameters()}
    for _ in range(2):
        losses, norm, stepped = trainer.run_step(train_inputs(**TRAIN_CASE))
        assert stepped and norm > 0 and all(np.isfinite(v) for v in losses.values())
    torch.cuda.synchronize()
    now, ema_now = dict(head.named_parameters()), dict(ema.named_parameters())
    for n in new:
        assert not torch.equal(now[n].detach(), before[n]), f"not stepped: {n}"
        assert not torch.equal(ema_now[n].detach(), ema_before[n]), f"the teacher's copy did not follow: {n}"
    sd = model.state_dict()
    for pre in ("sem_seg_head.", "ema_sem_seg_head."):
        assert all(pre + n in sd for n in new), pre
    feats = hu.case_feats("headfuse_eval")
    toks = _toks(feats, torch.float32)
    fresh = _flagged_head().cuda()
    fresh.load_state_dict(head.state_dict())
    with torch.no_grad():
        got = head.eval().forward_tokens(toks).t
        want = fresh.eval().forward_tokens(toks).t
    assert head.last_route == fresh.last_route == "fused" and torch.equal(got, want)


def test_graphed_inference_with_a_flagged_head_equals_the_synchronous_forward(cuda):
    """MadmInference with a flagged head through GraphedInference: every slot bit-identical to forward() under the throughput
    profile, and the head took the fused kernel."""
    from golden_util import init_eval_params
    from madm_amd import ops
    from madm_amd.meta_arch import MadmInference
    from madm_amd.pipeline import GraphedInference
    size = 64
    backbone, head = _backbone(torch.float16, size, finetune_unet="no"), _flagged_head()
    init_eval_params(backbone, head)
    model = MadmInference(backbone.cuda(), head.cuda(), target_modality="Depth").eval()
    imgs = [255.0 * torch.rand((3, size, size), generator=torch.Generator().manual_seed(40 + i)).cuda() for i in range(3)]
    with torch.no_grad():
        with ops.tuning_profile("throughput", pin=True):
            want = [model([{'target_second_modality': im}])[0]['sem_seg'].clone() for im in imgs]
        assert head.last_route == "fused"
        runner = GraphedInference(model, [{'target_second_modality': imgs[0]}], streams=2)
        got = []
        for im in imgs:
            outs, done, _slot = runner.submit([{'target_second_modality': im}])
            done.synchronize()
            got.append(outs[0]['sem_seg'].clone())
        runner.drain()
    for a, b in zip(got, want):
        assert a.shape == b.shape == (1, hu.K, size, size) and torch.equal(a, b)
