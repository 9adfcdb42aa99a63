"""Exact and per-element tests of the kernels through which an image enters the model: madm_stem_conv3x3 (both kernels),
madm_image_to_im2col3x3, madm_image_to_nhwc / madm_nchw_f32_to_nhwc, the range probe behind their ``minmax`` argument, the other
glue kernels of csrc/misc.hip and the colour augmentation kernels of csrc/train.hip.  Data, references, bounds and mutants:
tests/frontend_util.py, proved on the host by test_frontend_exact_host.py.

Layer 1 asserts bit patterns (outputs), exact float64 statistics and the probe's exact pair; layer 2 asserts a counted tolerance
per element against float64, nothing excluded.  Every launch is a legal call; the NaN and -0.0 inputs are ordinary data."""
import os
import random

import numpy as np
import pytest
import torch

import frontend_util as U
from frontend_util import F32, BF16, F16, DT3, ID3, assert_within, rounded, same_bits, epc

pytestmark = pytest.mark.gpu


def _lib():
    from madm_amd._lib import lib
    from madm_amd.ops import check, _stream, dtype_code
    return lib, check, _stream, dtype_code


def _fresh_minmax():
    return torch.tensor([float("inf"), float("-inf")], device="cuda")


# ---- A. stem ------------------------------------------------------------------------------------------------------------------------
def _stem(img, w, bias, dtype, mean, std, route, stats=True, minmax=True):
    """-> (tokens [B * H * W, 128] on the CPU, stats or None, (lo, hi) or None, the columns beyond 128 or None)"""
    from madm_amd import ops
    lib, check, stream, code = _lib()
    B, _c, H, W = img.shape
    wT, bs, im = U.to_wT(w).float().cuda(), bias.float().cuda(), img.cuda()
    st = torch.zeros((B, U.STEM_N, 2), dtype=torch.float64, device="cuda") if stats else None
    mm = _fresh_minmax() if minmax else None
    rest = None
    old = os.environ.get("MADM_STEM_KERNEL")
    if route == "env_fma":
        os.environ["MADM_STEM_KERNEL"] = "1"
    try:
        if route == "ldo_odd":
            buf = torch.full((B * H * W, U.STEM_LDO_ODD), 3.0, dtype=dtype, device="cuda")
            check(lib.madm_stem_conv3x3(code(dtype), im.data_ptr(), wT.data_ptr(), bs.data_ptr(), buf.data_ptr(), U.STEM_LDO_ODD, B, H, W,
                                        U.STEM_N, float(mean), float(std), None if st is None else st.data_ptr(),
                                        None if mm is None else mm.data_ptr(), stream()), "madm_stem_conv3x3")
            out, rest = buf[:, :U.STEM_N], buf[:, U.STEM_N:]
        else:
            out = ops.stem_conv3x3(im, wT, bs, dtype, mean, std, stats=st, minmax=mm)
    finally:
        if route == "env_fma":
            if old is None:
                del os.environ["MADM_STEM_KERNEL"]
            else:
                os.environ["MADM_STEM_KERNEL"] = old
    torch.cuda.synchronize()
    return (out.cpu(), None if st is None else st.cpu(), None if mm is None else tuple(mm.tolist()),
            None if rest is None else rest.cpu())


STEM_ROUTES = [(dt, r) for dt in DT3 for r in (["default", "ldo_odd"] if dt == F32 else ["default", "env_fma", "ldo_odd"])]
STEM_ROUTE_IDS = [f"{ID3[DT3.index(dt)]}-{r}" for dt, r in STEM_ROUTES]


@pytest.mark.parametrize("H", U.STEM_H)
@pytest.mark.parametrize("dtype,route", STEM_ROUTES, ids=STEM_ROUTE_IDS)
def test_stem_lattice(cuda, dtype, route, H):
    """Bit-equal tokens, exactly equal f64 statistics [B][128][2] and the probe's exact pair for every width, under both
    normalisations; (0, 1) runs once without statistics and once without the probe"""
    for W in U.STEM_W:
        for ni, (mean, std) in enumerate(U.NORMS):
            ns = U.stem_case(H, W, ni)
            want = rounded(ns.tok, dtype)
            for stats, minmax in ([(True, True)] if ni == 0 else [(False, True), (True, False)]):
                what = f"{H} x {W}, mean {mean}, std {std}, stats {stats}, minmax {minmax}"
                out, st, mm, rest = _stem(ns.img, ns.w, ns.bias, dtype, mean, std, route, stats, minmax)
                assert same_bits(out.contiguous(), want), f"{what}: {int((out.double() != want.double()).sum())} outputs differ"
                if st is not None:
                    assert torch.equal(st, ns.stats), f"{what}: statistics differ by up to {float((st - ns.stats).abs().max())}"
                if mm is not None:
                    assert mm == (ns.lo, ns.hi), f"{what}: probe {mm}, expected {(ns.lo, ns.hi)}"
                if rest is not None:
                    assert bool((rest.float() == 3.0).all()), f"{what}: columns beyond 128 were written"


@pytest.mark.parametrize("shape", U.STEM_REAL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype,route", STEM_ROUTES, ids=STEM_ROUTE_IDS)
def test_stem_per_element(cuda, dtype, route, shape):
    """Random image: every output within half an ulp plus the counted accumulation term; the statistics against the float64
    sums of the unrounded values; the probe against the f32 normalisation"""
    kind = "mfma" if (dtype != F32 and route == "default") else "fma"
    ns = U.stem_real_case(shape[0], shape[1], dtype, kind)
    out, st, mm, _rest = _stem(ns.img, ns.w.double(), ns.bias.double(), dtype, ns.mean, ns.std, route)
    r1 = assert_within(out, ns.tok, ns.tol, "stem output")
    r2 = assert_within(st, ns.stats, ns.tol_stats, "stem statistics")
    print(f"   stem {route} {shape}: worst error / bound {r1:.3f} (outputs) {r2:.3f} (statistics)")
    assert mm == (float(ns.n32.min()), float(ns.n32.max()))


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_im2col_bits(cuda, dtype):
    """Lattice and random images: every stored element is the f32 normalisation rounded once, the columns k >= 27 are +0"""
    from madm_amd import ops
    for W in U.IM2COL_W:
        for Kpad in U.IM2COL_KPAD:
            for ni, (mean, std) in enumerate(U.NORMS):
                img, n = U.lattice_image(U.STEM_B, 3, U.IM2COL_H, W, (mean, std), 1500 + W + ni)
                rnd = U.uniform((U.STEM_B, 3, U.IM2COL_H, W), 1600 + W)
                for im, nn in ((img, n), (rnd, U.normalise32(rnd, mean, std).double())):
                    mm = _fresh_minmax()
                    got = ops.image_to_im2col3x3(im.cuda(), dtype, Kpad, mean, std, mm).cpu()
                    want = rounded(U.im2col_reference(nn, Kpad), dtype)
                    assert same_bits(got, want), f"W {W} Kpad {Kpad} mean {mean}: {int((got.double() != want.double()).sum())} differ"
                    assert tuple(mm.tolist()) == (float(nn.min()), float(nn.max()))


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_image_to_nhwc_bits(cuda, dtype):
    """C = 1, 3, 4 with one and two chunks per pixel; the padding channels are +0; madm_nchw_f32_to_nhwc is the (0, 1) case"""
    from madm_amd import ops
    H, W = U.NHWC_HW
    for C in U.NHWC_C:
        for chunks in (1, 2):
            Cpad = chunks * epc(dtype)
            if Cpad < C:
                continue
            for ni, (mean, std) in enumerate(U.NORMS):
                img, n = U.lattice_image(U.STEM_B, C, H, W, (mean, std), 1700 + C + ni)
                rnd = U.uniform((U.STEM_B, C, H, W), 1750 + C)
                for im, nn in ((img, n), (rnd, U.normalise32(rnd, mean, std).double())):
                    got = ops.image_to_nhwc(im.cuda(), dtype, Cpad, mean, std, None).cpu()
                    assert same_bits(got, rounded(U.nhwc_reference(nn, Cpad), dtype)), f"C {C} Cpad {Cpad} mean {mean}"
            got = ops.nchw_to_nhwc(rnd.cuda(), dtype, Cpad).cpu()
            assert same_bits(got, rounded(U.nhwc_reference(rnd.double(), Cpad), dtype)), f"nchw_to_nhwc C {C} Cpad {Cpad}"


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_image_to_nhwc_second_trip(cuda, dtype):
    """B HW = 2048 * 256 + 37 pixels: the pixels past the grid cap are written by a second trip of the loop"""
    from madm_amd import ops
    img = U.uniform((1, 1, 1, U.NHWC_BIG_W), 1800)
    mm = _fresh_minmax()
    got = ops.image_to_nhwc(img.cuda(), dtype, epc(dtype), 0.5, 0.5, mm).cpu()
    n32 = U.normalise32(img, 0.5, 0.5)
    assert same_bits(got, rounded(U.nhwc_reference(n32.double(), epc(dtype)), dtype))
    assert tuple(mm.tolist()) == (float(n32.min()), float(n32.max()))


# ---- B. range probe ------------------------------------------------------------------------------------------------------------------
def _probe(x, mean, std, entry="nhwc"):
    """The published pair for the flat f32 data x, through the ``minmax`` argument of one of the three entries"""
    from madm_amd import ops
    mm = _fresh_minmax()
    n = x.numel()
    if entry == "nhwc":
        shape = (1, 3, 419, 419) if n == 3 * 419 * 419 else (1, 1, 1, n)
        ops.image_to_nhwc(x.view(shape).cuda(), F32, 4, mean, std, mm)
    elif entry == "im2col":
        ops.image_to_im2col3x3(x.view(1, 3, 1, n // 3).cuda(), F32, 32, mean, std, mm)
    else:
        w, bias = U.stem_weights()
        ops.stem_conv3x3(x.view(1, 3, 1, n // 3).cuda(), U.to_wT(w).float().cuda(), bias.float().cuda(), F32, mean, std, minmax=mm)
    return tuple(mm.tolist())


@pytest.mark.parametrize("sign", U.PROBE_SIGNS)
@pytest.mark.parametrize("n", U.PROBE_SIZES)
def test_range_probe_value(cuda, n, sign):
    """The pair equals torch.min / torch.max of the f32-normalised data with the minimum, then the maximum, in the first element,
    the last element of the float4 body, the scalar tail and a block other than 0"""
    mean, std = U.probe_norm(sign)
    for what, x in U.probe_rows(n, sign):
        got, want = _probe(x, mean, std), U.probe_expected(x, mean, std)
        assert got == want, f"n {n} {sign} {what}: probe {got}, torch {want}"


@pytest.mark.parametrize("entry", ["im2col", "stem"])
def test_range_probe_other_entries(cuda, entry):
    for sign in ("mixed", "neg_zero_max"):
        n = 3 * 2391                                 # float4 body and a tail, one block
        mean, std = U.probe_norm(sign)
        for what, x in U.probe_rows(n, sign):
            got, want = _probe(x, mean, std, entry), U.probe_expected(x, mean, std)
            assert got == want, f"{entry} {sign} {what}: probe {got}, torch {want}"


@pytest.mark.parametrize("where", U.PROBE_NAN_WHERE)
@pytest.mark.parametrize("n", U.PROBE_NAN_SIZES)
def test_range_probe_nan_fails_the_check(cuda, n, where):
    """The reference's assert fires for a batch with a NaN (torch.min propagates it): the published pair must not pass the
    Python-side check, directly and through DeferredRangeCheck"""
    from madm_amd.pipeline import DeferredRangeCheck
    x = U.probe_nan_row(n, where)
    assert not bool(-1 <= torch.min(x) and torch.max(x) <= 1)
    from madm_amd import ops
    mm = _fresh_minmax()
    shape = (1, 3, 419, 419) if n == 3 * 419 * 419 else (1, 1, 1, n)
    ops.image_to_nhwc(x.view(shape).cuda(), F32, 4, 0.0, 1.0, mm)
    lo, hi = mm.tolist()
    assert not U.in_range(lo, hi), f"n {n}, NaN at {where}: the probe published ({lo}, {hi}), which passes -1 <= lo and hi <= 1"
    rc = DeferredRangeCheck(torch.device("cuda"), depth=2)
    rc.make_room()
    rc.push(mm, torch.cuda.current_stream(), 0)
    with pytest.raises(AssertionError, match="input range check"):
        rc.drain()


def test_trainer_range_assert_fires_for_a_nan_pixel(cuda):
    """test_trainer_range_assert_fires_before_the_optimizer_step with a batch that holds ONE NaN pixel: the same AssertionError,
    bit-unchanged parameters, moments, step counts and loss scale"""
    from madm_amd.train import MadmTrainer
    from golden_util import TRAIN_CASE, train_inputs
    from test_train_gpu import build_product_train
    model = build_product_train(torch.float32, "train_depth_lora_only")
    trainer = MadmTrainer(model, lr=1e-3, weight_decay=0.05, grad_clip=None, amp=False)
    random.seed(1)
    np.random.seed(2)
    good = train_inputs(**TRAIN_CASE)
    trainer.run_step(good)
    torch.cuda.synchronize()
    flat0, m0, v0 = trainer.opt.flat.flat.clone(), trainer.opt.m.clone(), trainer.opt.v.clone()
    steps0, scale0, it0 = list(trainer.opt.steps), trainer.scale, trainer.iter
    bad = train_inputs(**TRAIN_CASE)
    rgb = bad[1]["source_rgb"].float().clone()
    rgb.view(-1)[rgb.numel() // 2 + 1] = float("nan")
    bad[1]["source_rgb"] = rgb
    with pytest.raises(AssertionError, match="input range check"):
        trainer.run_step(bad)
    torch.cuda.synchronize()
    assert torch.equal(trainer.opt.flat.flat, flat0) and torch.equal(trainer.opt.m, m0) and torch.equal(trainer.opt.v, v0)
    assert list(trainer.opt.steps) == steps0 and trainer.scale == scale0 and trainer.iter == it0
    losses, _norm, stepped = trainer.run_step(good)
    assert stepped and all(np.isfinite(v) for v in losses.values())


# ---- C. the rest of misc.hip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", U.NCHW_ROWS, ids=lambda r: f"c{r[0]}_hw{r[1]}")
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_nhwc_to_nchw_bits(cuda, dtype, row):
    """ld > C, c_off = 2, Ctot > c_off + C, B = 2: the window equals x[:, :C].float() permuted and the rest keeps its prefill"""
    lib, check, stream, code = _lib()
    ns = U.nchw_case(row[0], row[1], dtype)
    x = ns.x.cuda()
    out = torch.full((ns.B, ns.Ctot, ns.HW), U.NCHW_PREFILL, dtype=F32, device="cuda")
    check(lib.madm_nhwc_to_nchw_f32(code(dtype), x.data_ptr(), ns.ld, out.data_ptr(), ns.B, ns.C, ns.c_off, ns.Ctot, ns.HW, stream()),
          "madm_nhwc_to_nchw_f32")
    assert same_bits(out.cpu(), ns.want)


def _latents_add_noise(ns, dtype, Cpad):
    from madm_amd import ops
    lat, noisy = ops.latents_add_noise(ns.m.to(dtype).cuda(), ns.scaling, ns.noise.float().cuda(), ns.sa.float().cuda(),
                                       ns.sn.float().cuda(), ns.ts.cuda(), U.LAN_B, U.LAN_HW, Cpad, 1, U.LAN_HW)
    return lat.cpu().view(U.LAN_B, 4, U.LAN_HW), noisy.cpu()


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_latents_add_noise(cuda, dtype):
    """Timesteps {0, 999} in one batch, ldm = 8.  Lattice: bit-equal noisy latents; real scaling and schedule: 4 counted
    roundings; latents_nchw is the single f32 product in both; the padding columns are +0"""
    for chunks in (1, 2):
        Cpad = chunks * epc(dtype)
        ns = U.lan_case("lattice", dtype)
        lat, noisy = _latents_add_noise(ns, dtype, Cpad)
        assert same_bits(lat, ns.lat.float()) and same_bits(noisy[:, :4].contiguous(), rounded(ns.noisy, dtype))
        assert int((U.bits(noisy[:, 4:]) != 0).sum()) == 0
        ns = U.lan_case("real", dtype)
        lat, noisy = _latents_add_noise(ns, dtype, Cpad)
        assert same_bits(lat, ns.lat32), "latents_nchw is not the f32 product m * scaling"
        r = assert_within(noisy[:, :4], ns.noisy, ns.tol, "noisy latents")
        print(f"   latents_add_noise Cpad {Cpad}: worst error / bound {r:.3f}")
        assert int((U.bits(noisy[:, 4:]) != 0).sum()) == 0


@pytest.mark.parametrize("dim", U.TE_DIMS)
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_timestep_embedding(cuda, dtype, dim):
    from madm_amd import ops
    ts, freqs = torch.tensor(U.TE_T, dtype=torch.int64), U.te_freqs(dim)
    got = ops.timestep_embedding(ts.cuda(), freqs.cuda(), dtype).cpu()
    ref, tol = U.te_reference(ts, freqs, dtype)
    half = dim // 2
    assert same_bits(got[0, :half].contiguous(), torch.ones(half, dtype=dtype)) and same_bits(got[0, half:].contiguous(), torch.zeros(half, dtype=dtype))
    r = assert_within(got, ref, tol, "timestep embedding")
    print(f"   timestep_embedding dim {dim}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("n", U.FLAT_SIZES)
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_flat_kernels(cuda, dtype, n):
    """silu per element; rows_to_f32 (with and without ``add``), cast_from_f32 and copy_columns bit for bit"""
    from madm_amd import ops
    x, y, tol = U.silu_case(n, dtype)
    assert_within(ops.silu(x.cuda()).cpu(), y, tol, "silu")
    assert same_bits(ops.rows_to_f32(x.cuda()).cpu(), x.float())
    add = U.gen((n,), 830 + n % 999)
    assert same_bits(ops.rows_to_f32(x.cuda(), add.cuda()).cpu(), x.float() + add)
    xf = U.cast_input(n)
    assert same_bits(ops.cast_from_f32(xf.cuda(), dtype).cpu(), rounded(xf, dtype))
    C, lds, ldd = 3, 5, 4
    rows = -(-n // C)
    src = rounded(U.gen((rows, lds), 840 + n % 999).double(), dtype)
    dst = torch.full((rows, ldd), 9.0, dtype=dtype)
    want = dst.clone()
    want[:, :C] = src[:, :C]
    got = ops.copy_columns(src.cuda(), dst.cuda(), C).cpu()
    assert same_bits(got, want)


@pytest.mark.parametrize("n", U.FLAT_SIZES)
def test_clamp_f32(cuda, n):
    """lo = hi, infinite bounds and inputs, -0.0: the values of torch.clamp; the bit patterns where no bound is a zero"""
    from madm_amd import ops
    x = U.clamp_input(n)
    for lo, hi in U.CLAMP_BOUNDS:
        got, want = ops.clamp_f32(x.cuda(), lo, hi).cpu(), torch.clamp(x, lo, hi)
        assert torch.equal(got, want), f"clamp({lo}, {hi})"
        if lo != 0.0 and hi != 0.0:
            assert same_bits(got, want), f"clamp({lo}, {hi}): bit patterns"


# ---- D. colour augmentation ----------------------------------------------------------------------------------------------------------
def _gray_sum(img):
    lib, check, stream, _c = _lib()
    x = img.contiguous().cuda()
    gs = torch.zeros(1, dtype=torch.float64, device="cuda")
    check(lib.madm_gray_sum(x.data_ptr(), x.shape[1], gs.data_ptr(), stream()), "madm_gray_sum")
    return float(gs.item())


def _jitter(img, op, f, gs=None, in_place=False):
    lib, check, stream, _c = _lib()
    x = img.contiguous().cuda()
    out = x if in_place else torch.full_like(x, -7.0)
    g = None if gs is None else torch.tensor([gs], dtype=torch.float64, device="cuda")
    check(lib.madm_color_jitter_step(x.data_ptr(), out.data_ptr(), x.shape[1], int(op), float(f), None if g is None else g.data_ptr(),
                                     stream()), "madm_color_jitter_step")
    return out.cpu()


@pytest.mark.parametrize("HW", U.GRAY_HW)
def test_gray_sum(cuda, HW):
    """One non-zero channel of powers of two pins each coefficient bit for bit and counts every pixel once; then a random image
    against the float64 sum with 5 roundings per pixel"""
    for ch in range(3):
        img, want = U.gray_exact_case(HW, ch)
        got = _gray_sum(img)
        assert got == want, f"channel {ch}: {got!r} != {want!r}"
    img = U.uniform((3, HW), 1900 + HW % 999)
    ref, tol = U.gray_sum_bound(img)
    got = _gray_sum(img)
    assert abs(got - ref) <= tol, f"{got!r} vs {ref!r}: error {abs(got - ref):.3e}, bound {tol:.3e}"


def test_color_jitter_exact_selectors(cuda):
    HW = 257
    x = (torch.randint(0, 17, (3, HW), generator=torch.Generator().manual_seed(5)).float() / 16)
    for f in (0.5, 1.0, 1.5, 2.0):
        want = (x.double() * f).clamp(0, 1).float()
        assert f <= 1.0 or bool((x.double() * f > 1).any())             # (values that clamp)
        assert same_bits(_jitter(x, 0, f), want), f"brightness {f}"
    img = U.jitter_image(HW)
    gs = float(U.gray_of64(img.double()).sum())
    assert same_bits(_jitter(img, 1, 1.0, gs), img), "contrast 1 changed bits"
    assert same_bits(_jitter(img, 2, 1.0), img), "saturation 1 changed bits"
    v = torch.cat([U.uniform((HW - 2,), 6), torch.tensor([0.0, 1.0])])
    grey = v.view(1, HW).expand(3, HW).contiguous()
    for f in (-0.2, 0.0, 0.2, 1.3, -3.0):
        assert same_bits(_jitter(grey, 3, f), grey), f"hue {f} moved a grey pixel"
    for op, f in ((0, 1.3), (1, 0.8), (2, 1.2), (3, 0.2), (3, -0.2)):
        assert same_bits(_jitter(img, op, f, gs, in_place=True), _jitter(img, op, f, gs)), f"op {op}: in place differs"


@pytest.mark.parametrize("HW", U.JIT_HW)
def test_color_jitter_per_element(cuda, HW):
    """Every element within the counted bound of the float64 restatement of oracle/augment.py's formulas"""
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    for op, fs in ((0, (0.8, 1.2)), (1, (0.8, 1.2)), (2, (0.8, 1.2, 0.0)), (3, U.JIT_HUE_F)):
        for f in fs:
            img = U.jitter_image(HW, f if op == 3 else 0.0)
            gs = float(U.gray_of64(img.double()).sum())
            ref, tol = U.jitter_reference(img.double(), op, f32(f), gs)
            r = assert_within(_jitter(img, op, f, gs), ref, tol, f"color_jitter op {op} f {f}")
            print(f"   color_jitter HW {HW} op {op} f {f}: worst error / bound {r:.3f}")


def _blur(x, axis, w):
    lib, check, stream, _c = _lib()
    xi, wt = x.float().contiguous().cuda(), w.float().contiguous().cuda()
    out = torch.full_like(xi, -7.0)
    P, H, W = xi.shape
    check(lib.madm_blur_axis_f32(xi.data_ptr(), out.data_ptr(), P, H, W, axis, len(w), wt.data_ptr(), stream()), "madm_blur_axis_f32")
    return out.cpu()


@pytest.mark.parametrize("row", U.BLUR_ROWS, ids=U.blur_id)
def test_blur_axis(cuda, row):
    ns = U.blur_case(row, "lattice")
    assert same_bits(_blur(ns.x, row[3], ns.w), ns.out.float()), "lattice"
    ns = U.blur_case(row, "real")
    assert_within(_blur(ns.x, row[3], ns.w), ns.out, ns.tol, "blur")
