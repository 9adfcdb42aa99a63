"""Host-side checks of ``DAFormerHead(final_fuse_vae_decoder_feat=True)`` and of libmadm_headfuse.so (include/madm_headfuse.h,
madm_amd/_lib_headfuse.py): the float64 restatement against the fixtures the reference's class produced, the exactness
conditions and negative controls of the lattice inputs tests/test_head_fuse_gpu.py compares with torch.equal, the header and the
exports, argument checks without a GPU, lazy loading, the state-dict contract, and the two static scans tests/test_host.py runs
over the main library.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_fuse_util as hu
import sidelib_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madm_headfuse.h")


# ---- the restatement and the fixtures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hu.CASES))
def test_restatement_reproduces_the_reference_fixture(name):
    """FlaggedOracleHead in float64 against what the reference's DAFormerHead(final_fuse_vae_decoder_feat=True) gave in float32:
    logits to 2e-5 of their range, every sampled gradient to 1e-3 of the tensor's range and its norm to 1e-4 (float32 autograd
    through ReLU kinks on the reference's side)."""
    gold = hu.load_fixture(name)
    out = hu.run_case(hu.init_head_(hu.FlaggedOracleHead()).double(), name)
    assert set(out) == set(gold)
    for k in sorted(gold):
        a, b = torch.from_numpy(np.asarray(out[k], dtype=np.float64)), torch.from_numpy(np.asarray(gold[k], dtype=np.float64))
        assert a.shape == b.shape, k
        if k.startswith(("gnorm:", "dfnorm:")):
            assert abs(float(a) - float(b)) <= 1e-4 * float(b), (k, float(a), float(b))
        else:
            d = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
            assert d < (2e-5 if k in ("logits",) or k.startswith("bn:") else 1e-3), (k, d)
    if hu.CASES[name][2]:
        assert sum(k.startswith("grad:") for k in gold) == 46 and sum(k.startswith("dfeat:") for k in gold) == 4



def test_state_dict_keys_and_shapes_are_the_references():
    from madm_amd.head import DAFormerHead
    from oracle import madm_path
    head = DAFormerHead(in_channels=list(hu.CHANNELS), in_keys=list(hu.KEYS), in_index=[0, 1, 2, 3], channels=256, num_classes=hu.K,
                        norm_cfg=dict(type='BN'), decoder_params=madm_path.head_decoder_params(), final_fuse_vae_decoder_feat=True)
    with np.load(os.path.join(hu.GOLDEN, "headfuse_state.npz")) as z:
        want = {str(k): tuple(int(d) for d in str(s).split(",") if d) for k, s in zip(z["keys"], z["shapes"])}
    got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert got == want, (sorted(set(got) ^ set(want)), [k for k in got if k in want and got[k] != want[k]])
    assert len(list(head.named_parameters())) == 46 and tuple(head.conv_seg.weight.shape) == (hu.K, 320, 1, 1)
    new = {k for k in got if k.startswith("vae_decoder_feat_proj.0.")}
    assert new == {f"vae_decoder_feat_proj.0.{c}.{p}" for c in ("conv1", "conv2", "conv3", "shortcut")
                   for p in ("weight", "norm.weight", "norm.bias")}
    # the restatement the GPU tests compare with has the same contract
    assert {k: tuple(v.shape) for k, v in hu.FlaggedOracleHead().state_dict().items()} == want
    # a deep copy (the EMA teacher) carries the new parameters and no derived operand
    import copy
    twin = copy.deepcopy(head)
    assert set(twin.state_dict()) == set(got) and "_wide_cache" not in twin.vae_decoder_feat_proj[0].__dict__


def test_flag_off_head_is_unchanged_and_the_other_flag_is_still_refused():
    from madm_amd.head import DAFormerHead
    from oracle import madm_path
    kw = dict(in_channels=list(hu.CHANNELS), in_keys=list(hu.KEYS), in_index=[0, 1, 2, 3], channels=256, num_classes=hu.K,
              norm_cfg=dict(type='BN'), decoder_params=madm_path.head_decoder_params())
    plain = DAFormerHead(**kw)
    assert not plain.final_fuse_vae_decoder_feat and not hasattr(plain, "vae_decoder_feat_proj")
    assert tuple(plain.conv_seg.weight.shape) == (hu.K, 256, 1, 1) and len(list(plain.named_parameters())) == 34
    with pytest.raises(NotImplementedError):
        DAFormerHead(concat_attention_to_conv_seg=True, **kw)
    with pytest.raises(NotImplementedError):
        DAFormerHead(concat_attention_to_conv_seg=True, final_fuse_vae_decoder_feat=True, **kw)


# ---- the lattice inputs of the kernel tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", hu.KERNEL_KS)
@pytest.mark.parametrize("hw", hu.KERNEL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lattice_cases_are_exact_and_the_comparison_rejects_mutants(hw, k):
    """The exactness conditions of every lattice case, and: the float64 reference changes under every mutant that is
    visible at the case's size (the three spatial mutants need two source rows and columns; a 1 x 1 map has no neighbour to
    confuse)."""
    h, w = hw
    data = hu.lattice_case(h, w, k)
    ref = hu.check_exact(*data)
    assert ref.shape == (hu.KERNEL_B, 2 * h, 2 * w, hu.kp_of(k)) and not ref[..., k:].any() and bool(ref[..., :k].any())
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(hu.classify_ref(*data, dt), ref)            # the one rounding is a no-op on the lattice
    for m in hu.MUTANTS:
        mh, mw = hu.SPATIAL_MUTANTS.get(m, (1, 1))
        if h < mh or w < mw:
            continue
        assert not torch.equal(hu.classify_ref(*data, torch.float32, mutant=m), ref), f"{m}: the reference does not change"


def test_every_mutant_is_exercised_and_the_reference_is_torchs_interpolate():
    seen = {m for (h, w) in hu.KERNEL_SIZES for m in hu.MUTANTS if (h, w) >= hu.SPATIAL_MUTANTS.get(m, (1, 1))}
    assert seen == set(hu.MUTANTS) and len(hu.MUTANTS) >= 6
    import torch.nn.functional as F
    for h, w in hu.KERNEL_SIZES:
        x = torch.randn((2, h, w, 5), dtype=torch.float64, generator=torch.Generator().manual_seed(h))
        want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert float((hu.up2x(x) - want).abs().max()) < 1e-14


def test_bound_is_small_and_positive():
    """The per-element bound is a rounding bound, not a tolerance: a few 1e-3 of the output's scale in bf16, 1e-6 in f32."""
    for dt, cap in ((torch.float32, 2e-4), (torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)):
        data = hu.random_case(17, 9, 11, dt)
        b = hu.classify_bound(*data, dt)[..., :11]
        ref = hu.classify_ref(*data, dt)[..., :11]
        assert float(b.min()) > 0 and float(b.max()) < cap * float(ref.abs().max()), (dt, float(b.max()), float(ref.abs().max()))


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_header_declares_only_its_own_names():
    from madm_amd import _cabi
    abi = _cabi.parse(HEADER)
    names = [n for n, _r, _p in abi.prototypes]
    assert names == ["mhf_abi_version", "mhf_last_error", "mhf_upsample_cat_classify"]
    assert abi.constants and all(k.startswith("MHF_") for k in abi.constants) and not abi.structs
    assert abi.prototypes[2][2][-1][0] == "stream"
    main = _cabi.parse(os.path.join(ROOT, "include", "madm_hip.h")).constants
    assert [abi.constants[k] for k in ("MHF_F32", "MHF_BF16", "MHF_F16")] == [main[k] for k in ("MADM_F32", "MADM_BF16", "MADM_F16")]


def test_library_exports_exactly_the_header():
    path = os.environ.get("MADM_HEADFUSE_LIB") or os.path.join(ROOT, "madm_amd", "libmadm_headfuse.so")
    su.assert_exports_exactly(path, "madm_headfuse.h")


def test_import_does_not_load_the_library():
    code = ("import sys, madm_amd, madm_amd.ops as ops, madm_amd.head as head\n"
            "from oracle import madm_path\n"
            "assert 'madm_amd._lib_headfuse' not in sys.modules\n"
            "h = head.DAFormerHead(in_channels=[128, 512, 512, 512], in_keys=['s0', 's3', 's4', 's5'], in_index=[0, 1, 2, 3],\n"
            "                      channels=256, num_classes=11, decoder_params=madm_path.head_decoder_params(),\n"
            "                      final_fuse_vae_decoder_feat=True)\n"
            "assert 'madm_amd._lib_headfuse' not in sys.modules\n"
            "assert 'libmadm_headfuse' not in open('/proc/self/maps').read()\n"
            "from madm_amd import _lib_headfuse\n"
            "assert 'libmadm_headfuse' in open('/proc/self/maps').read() and _lib_headfuse.lib.mhf_abi_version() == 1\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_bad_arguments_are_refused_without_a_gpu():
    """INVALID_ARG before any launch: null and misaligned pointers, unknown dtype, unsupported widths, H != 2h, W != 2w, row
    strides too small or off the chunk, Kp off its range -- each with the entry point's name in the message."""
    from madm_amd import _lib_headfuse as L
    m = su.Host()
    p = lambda i: m.at(4096 * i)      # noqa: E731
    #        dtype hd   ldh  proj  ldp w     ldw  bias  out   ldo B  h  w  H  W   C1   C2  Kp  stream
    good = [1, p(0), 256, p(1), 64, p(2), 320, p(3), p(4), 12, 2, 3, 5, 6, 10, 256, 64, 12, None]
    idx = dict(dtype=0, hd=1, ldh=2, proj=3, ldp=4, w=5, ldw=6, bias=7, out=8, ldo=9, B=10, h=11, w_lo=12, H=13, W=14, C1=15,
               C2=16, Kp=17)

    def refused(what, **change):
        args = list(good)
        for k, v in change.items():
            args[idx[k]] = v
        rc = L.lib.mhf_upsample_cat_classify(*args)
        assert rc == L.MHF_ERR_INVALID_ARG, f"{what} was not refused (status {rc})"
        assert "upsample_cat_classify:" in L.last_error(), (what, L.last_error())

    for k in ("hd", "proj", "w", "bias", "out"):
        refused(f"null {k}", **{k: None})
        refused(f"{k} off a 16-byte boundary", **{k: ctypes.c_void_p(good[idx[k]].value + 4)})
    refused("unknown dtype", dtype=3)
    refused("C1 no multiple of 32", C1=48, ldh=48, ldw=112)
    refused("C1 wider than the LDS tile", C1=1024, ldh=1024, ldw=1088)
    refused("f32 C1 wider than the LDS tile", dtype=0, C1=512, ldh=512, ldw=576)
    refused("C2 no multiple of 32", C2=40, ldp=40, ldw=296)
    refused("C2 zero", C2=0)
    refused("H != 2h", H=7)
    refused("H = h", H=3)
    refused("W != 2w", W=11)
    refused("ldh too small", ldh=248)
    refused("ldh off the chunk", ldh=260)
    refused("ldp too small", ldp=56)
    refused("ldw too small", ldw=312)
    refused("ldo too small", ldo=8)
    refused("ldo no multiple of 4", ldo=14)
    refused("Kp no multiple of 4", Kp=11)
    refused("Kp too large", Kp=68, ldo=68)
    for k in ("B", "h", "w_lo"):
        for z in (0, -1):
            refused(f"{k} = {z}", **{k: z})
    refused("tensor too large", B=40000, h=200, H=400, w_lo=200, W=400)


def test_headfuse_kernels_use_no_scratch_and_no_packed_fp32():
    from madm_amd._lib_headfuse import LIB_PATH
    rows = su.scan_kernels(LIB_PATH)
    assert len(rows) == 9 and all("upsample_cat_classify_kernel" in k for k in rows), sorted(rows)    # 3 dtypes x 3 class-tile counts
