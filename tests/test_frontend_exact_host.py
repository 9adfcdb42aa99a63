"""The utilities of tests/frontend_util.py, proved on the CPU: every lattice condition the builders assert holds on every row, every
mutant differs from its reference on every row it applies to (one is equivalent, and shown to be), a plain float32 restatement of
each kernel's expression stays inside the layer-2 bound of the float64 reference -- so the bounds hold for the reference arithmetic
alone, before any kernel is judged by them -- and the reference's range assert fails for a batch that holds a NaN."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_util as U
from frontend_util import F32, BF16, F16, DT3, ID3, assert_within, rounded


# ---- A. stem ------------------------------------------------------------------------------------------------------------------------
def test_stem_weight_table():
    w, bias = U.stem_weights()
    wT = U.to_wT(w)
    assert U.weight_rows_ok(wT) and float(w.abs().max()) == 2 and float(bias.abs().min()) >= 1
    for dt in DT3:
        assert torch.equal(w.to(dt).double(), w) and torch.equal(bias.float().double(), bias)
    assert torch.equal(wT[(1 * 3 + 2) * 3 + 1], w[:, 1, 1, 2])             # k = (r * 3 + s) * 3 + c
    bad = wT.clone()
    bad[5, :16] = bad[9, :16]
    assert not U.weight_rows_ok(bad)
    bad = wT.clone()
    bad[:, 17] = bad[:, 16]
    assert not U.weight_rows_ok(bad)


@pytest.mark.parametrize("H", U.STEM_H)
def test_stem_lattice_rows_and_mutants(H):
    """The builder's assertions on every row, the conv against F.conv2d, and every mutant that applies changes the outputs or the
    statistics"""
    for W in U.STEM_W:
        for ni, (mean, std) in enumerate(U.NORMS):
            ns = U.stem_case(H, W, ni)
            assert torch.equal(ns.out, F.conv2d(ns.n, ns.w, ns.bias, padding=1))
            assert (ns.lo, ns.hi) == (float(U.normalise32(ns.img, mean, std).min()), float(U.normalise32(ns.img, mean, std).max()))
            assert torch.equal(ns.stats[0, :, 0], ns.out[0].sum((1, 2))) and not torch.equal(ns.stats[0], ns.stats[1])
            for mut in U.STEM_MUTANTS:
                out, st = U.stem_reference(ns.n, ns.w, ns.bias, mut, border=(0.0 - mean) / std)
                differs = not (torch.equal(out, ns.out) and torch.equal(st, ns.stats))
                assert differs == U.stem_mutant_applies(mut, H, W, mean), f"{mut} at {H} x {W}, mean {mean}: differs = {differs}"


def test_normalisation_has_one_bit_pattern():
    """(x - mean) * fl(1 / std) in f32 against float64: off by at most the two roundings, and the image entries' references are
    that f32 value rounded once"""
    x = U.uniform((4096,), 1)
    for mean, std in U.NORMS + [(0.125, -1.25)]:
        n32 = U.normalise32(x, mean, std).double()
        n64 = (x.double() - mean) / std
        assert bool(((n32 - n64).abs() <= 3 * U.U32 * (x.double().abs() + abs(mean)) / abs(std)).all())


@pytest.mark.parametrize("shape", U.STEM_REAL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_stem_bounds_hold_for_f32_arithmetic(dtype, shape):
    for route in (["fma"] if dtype == F32 else ["fma", "mfma"]):
        ns = U.stem_real_case(shape[0], shape[1], dtype, route)
        v = U.stem_emulate(ns, route)                                       # f32 values before rounding
        r = assert_within(U.tokens(rounded(v.double(), dtype)), ns.tok, ns.tol, f"stem {route}")
        assert r > 0.05, f"the bound is {1 / r:.0f} x what f32 arithmetic needs: too loose to say anything"
        # the statistics as the kernel forms them: f32 sums per 4 x 128 block (here: per image row band), f64 across
        st = torch.stack([v.double().sum((2, 3)), (v * v).double().sum((2, 3))], -1)
        assert_within(st, ns.stats, ns.tol_stats, f"stem statistics {route}")
        st32 = torch.stack([v.sum((2, 3)).double(), (v * v).sum((2, 3)).double()], -1)
        assert_within(st32, ns.stats, ns.tol_stats * max(1.0, shape[0] * shape[1] / U.STEM_BLOCK_PIXELS), "one f32 sum per image")


def test_im2col_and_nhwc_references():
    img, n = U.lattice_image(2, 3, 3, 5, U.NORMS[0], 7)
    rows = U.im2col_reference(n, 32)
    xp = F.pad(n, (1, 1, 1, 1))
    for (b, y, x, r, s, c) in [(0, 0, 0, 0, 0, 0), (1, 2, 4, 2, 2, 2), (1, 1, 3, 0, 2, 1), (0, 2, 0, 1, 0, 2)]:
        assert float(rows[(b * 3 + y) * 5 + x, (r * 3 + s) * 3 + c]) == float(xp[b, c, y + r, x + s])
    assert float(rows[:, 27:].abs().max()) == 0.0
    assert not torch.equal(U.im2col_reference(n, 32, "k_channel_major"), rows)
    t = U.nhwc_reference(n, 8)
    assert float(t[(1 * 3 + 2) * 5 + 4, 1]) == float(n[1, 1, 2, 4]) and float(t[:, 3:].abs().max()) == 0.0


# ---- B. range probe ------------------------------------------------------------------------------------------------------------------
def test_nan_semantics_of_the_range_assert():
    """ldm_diffusers.py:147: ``-1 <= torch.min(images) and torch.max(images) <= 1`` is False for a batch with a NaN, and so is the
    Python-side check for (NaN, NaN); the pair fminf / fmaxf leave behind, and the initial pair, would pass"""
    for n in U.PROBE_NAN_SIZES[:2]:
        for where in U.PROBE_NAN_WHERE:
            x = U.probe_nan_row(n, where)
            assert bool(torch.isnan(x).any()) and not bool(-1 <= torch.min(x) and torch.max(x) <= 1)
    assert not U.in_range(float("nan"), float("nan")) and not U.in_range(float("nan"), 0.5) and not U.in_range(-0.5, float("nan"))
    assert U.in_range(float("inf"), float("-inf"))          # what an all-NaN batch left before the flag: it passed
    assert U.in_range(-0.0, 0.0)


def test_probe_rows_reach_every_position():
    assert U.probe_blocks(3 * 419 * 419) == 64 and U.probe_blocks(4 * 1791 + 3) == 1 and U.probe_blocks(4 * 2049 + 2) == 2
    n = 3 * 419 * 419
    stride = 64 * 256
    assert n // 4 - U.PROBE_TRIP > 0 and n // 4 - U.PROBE_TRIP < stride          # one unrolled trip, then the remainder loop
    assert (4 * 1791 + 3) // 4 <= 7 * 256                                        # no unrolled trip at all
    for n in U.PROBE_SIZES:
        for sign in U.PROBE_SIGNS:
            mean, std = U.probe_norm(sign)
            names = [w for w, _x in U.probe_rows(n, sign)]
            want = [p for p in U.PROBE_POSITIONS if U.probe_position(n, p) is not None]
            assert names == [f"min_{p}" for p in want] + [f"max_{p}" for p in want]
            for what, x in U.probe_rows(n, sign):
                lo, hi = U.probe_expected(x, mean, std)
                assert U.in_range(lo, hi)
                i = U.probe_position(n, what.split("_", 1)[1])
                n32 = U.normalise32(x, mean, std)
                want_v = (lo if what.startswith("min") else hi) if std > 0 else (hi if what.startswith("min") else lo)
                assert float(n32[i]) == want_v, f"{n} {sign} {what}: the placed value is not the extreme"
                if n > 1:
                    assert int((n32 == want_v).sum()) == 1
    x = dict(U.probe_rows(4 * 1791 + 3, "neg_zero_max"))["max_tail"]
    assert np.signbit(x[-1].item()) and float(x.max()) == 0.0 and float(x[:-1].max()) < 0


# ---- C. the rest of misc.hip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_latents_add_noise_rows(dtype):
    ns = U.lan_case("lattice", dtype)
    got = U.lan_emulate(ns)
    assert torch.equal(got.double(), ns.noisy), "the lattice row is not exact in unfused f32"
    for kind in ("lattice", "real"):
        ns = U.lan_case(kind, dtype)
        for mut in U.LAN_MUTANTS:
            lat, noisy, _m = U.lan_reference(ns.m, ns.scaling, ns.noise, ns.sa, ns.sn, ns.ts, mut)
            assert not torch.equal(noisy, ns.noisy), f"{kind}: {mut} is not distinguishable"
            assert bool(((noisy - ns.noisy).abs() > ns.tol).any())
    ns = U.lan_case("real", dtype)
    r = assert_within(rounded(U.lan_emulate(ns).double(), dtype), ns.noisy, ns.tol, "latents_add_noise in f32")
    assert r > 0.05
    assert bool(((ns.lat32.double() - ns.lat).abs() <= U.half_ulp(ns.lat, F32)).all())      # the f32 product: one rounding


@pytest.mark.parametrize("dim", U.TE_DIMS)
def test_timestep_embedding_rows(dim):
    ts, freqs = torch.tensor(U.TE_T, dtype=torch.int64), U.te_freqs(dim)
    arg = ts.float().view(-1, 1) * freqs.view(1, -1)
    emu = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    for dt in DT3:
        ref, tol = U.te_reference(ts, freqs, dt)
        assert float(ref[0, 0]) == 1.0 and float(ref[0, dim // 2]) == 0.0
        assert_within(rounded(emu.double(), dt), ref, tol, "timestep embedding in f32")
        for mut in U.TE_MUTANTS:
            bad, _t = U.te_reference(ts, freqs, dt, mut)
            applies = not (mut == "freq_of_next" and dim == 2)              # one frequency: the next one is the same
            assert bool(((bad - ref).abs() > tol).any()) == applies, mut


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_flat_rows(dtype):
    x, y, tol = U.silu_case(4099, dtype)
    z = x.float()
    assert_within(rounded((z / (1.0 + torch.exp(-z))).double(), dtype), y, tol, "silu in f32")
    xf = U.cast_input(64)
    got = rounded(xf, dtype)
    assert bool(torch.isfinite(got.float()).all()) == (dtype != F16)        # 1e30 and 65520 overflow f16 alone
    assert float(rounded(torch.tensor([1.0 + 2.0 ** -8]), BF16)) == 1.0 and float(rounded(torch.tensor([1.0 + 3 * 2.0 ** -8]), BF16)) == 1.0 + 2.0 ** -6
    c = U.clamp_input(64)
    assert bool(torch.isinf(c).any()) and bool((c == 0).any())
    for lo, hi in U.CLAMP_BOUNDS:
        assert lo <= hi
    ns = U.nchw_case(3, 33, dtype)
    assert float(ns.want[1, 2, 5]) == float(ns.x[33 + 5, 0]) and float(ns.want[0, 0, 0]) == U.NCHW_PREFILL and float(ns.want[1, 5, 32]) == U.NCHW_PREFILL


# ---- D. colour augmentation ----------------------------------------------------------------------------------------------------------
def test_gray_rows():
    for HW in U.GRAY_HW:
        for ch in range(3):
            img, want = U.gray_exact_case(HW, ch)
            prod = (torch.tensor(np.float32([0.299, 0.587, 0.114][ch])) * img[ch])         # f32 products: exact
            assert torch.equal(prod.double(), U.GRAY[ch] * img[ch].double())
            assert float(prod.double().sum()) == want and float(prod.double().flip(0).cumsum(0)[-1]) == want
    img = U.uniform((3, 65536 + 257), 3)
    ref, tol = U.gray_sum_bound(img)
    g32 = torch.tensor(np.float32(0.299)) * img[0] + torch.tensor(np.float32(0.587)) * img[1] + torch.tensor(np.float32(0.114)) * img[2]
    err = abs(float(g32.double().sum()) - ref)
    assert err <= tol          # (a worst-case count over 65 793 pixels: the roundings of a sum cancel like a random walk)


def test_color_jitter_oracle_and_mutants():
    """The float64 restatement is oracle/augment.py's (up to the f32 constants), every mutant lies outside the bound somewhere, and
    "last maximum wins" is equivalent: identical on every pixel, ties included"""
    from oracle import augment as OA
    HW = 257
    for f in U.JIT_HUE_F:
        img = U.jitter_image(HW, f)
        x = img.double()
        gs = float(U.gray_of64(x).sum())
        fr = float(np.float32(f))
        for op, fo in ((0, 1.2), (1, 1.2), (2, 1.2), (3, fr)):
            ref, tol = U.jitter_reference(x, op, fo, gs)
            if op == 0:
                orc = torch.clamp(x * fo, 0, 1)
            elif op == 1:
                orc = torch.clamp(x * fo + OA.rgb_to_grayscale(x.view(3, 1, HW)).mean() * (1 - fo), 0, 1)
            elif op == 2:
                orc = torch.clamp((1 - fo) * OA.rgb_to_grayscale(x.view(3, 1, HW)).view(1, HW) + fo * x, 0, 1)
            else:
                orc = OA.color_jitter_image(x.view(3, 1, HW), 1.0, 1.0, fo / (2 * np.pi), 1.0, [3]).view(3, HW)
            assert float((orc - ref).abs().max()) < 3e-7, (op, f, float((orc - ref).abs().max()))
            r = assert_within(U.jitter_emulate(img, op, fo, gs), ref, tol, f"color_jitter op {op} in f32")
            assert r > 0.02, (op, f, r)
        applies = {"gray_rb_swapped": (1, 2), "contrast_mean_per_channel": (1,), "clamp_missing": (0, 1, 2), "hue_in_turns": (3,)}
        for mut, ops_ in applies.items():
            for op in ops_:
                fo = {0: 1.2, 1: 1.2, 2: 1.2, 3: fr}[op]
                ref, tol = U.jitter_reference(x, op, fo, gs)
                bad, _t = U.jitter_reference(x, op, fo, gs, mut)
                differs = bool(((bad - ref).abs() > tol).any())
                assert differs == (not (mut == "hue_in_turns" and fo == 0.0)), f"{mut} op {op} f {f}"
        same, _t = U.jitter_reference(x, 3, fr, gs, "last_max_wins")
        ref, _t = U.jitter_reference(x, 3, fr, gs)
        assert torch.equal(same, ref), "last maximum wins is expected to be equivalent"
        mx = x.max(0).values
        assert int(((x == mx).sum(0) >= 2).sum()) >= 10                     # (the image does hold ties)


def test_color_jitter_exact_rows():
    img = U.jitter_image(257)
    x = img.double()
    gs = float(U.gray_of64(x).sum())
    assert same(U.jitter_emulate(img, 1, 1.0, gs), img) and same(U.jitter_emulate(img, 2, 1.0), img)
    v = U.uniform((64,), 6)
    grey = v.view(1, 64).expand(3, 64).contiguous()
    for f in (-0.2, 0.0, 0.2, 1.3, -3.0):
        assert same(U.jitter_emulate(grey, 3, f), grey)
        assert torch.equal(U.jitter_reference(grey.double(), 3, f)[0], grey.double())
    hand = U.jitter_hand_pixels(0.2).double()
    assert float(hand.min()) >= 0 and float(hand.max()) <= 1
    # the border pixels do land within 1e-6 of a turn of a sector border after the shift
    b = hand[:, -12:]
    mxv, mnv = b.max(0).values, b.min(0).values
    assert bool(((mxv - 0.8).abs() < 1e-6).all()) and bool(((mnv - 0.4).abs() < 1e-6).all())


def same(a, b):
    return U.same_bits(a.contiguous(), b.contiguous())


@pytest.mark.parametrize("row", U.BLUR_ROWS, ids=U.blur_id)
def test_blur_rows(row):
    P, H, W, axis, ks = row
    assert ks // 2 < (W if axis else H)
    ns = U.blur_case(row, "lattice")
    assert torch.equal(U.blur_emulate(ns.x, axis, ns.w).double(), ns.out), "the lattice row is not exact in f32"
    if ks % 2 == 1:                                                         # the reference's statement: F.pad(reflect) + conv
        xp = F.pad(ns.x.unsqueeze(0), (ks // 2, ks // 2, 0, 0) if axis else (0, 0, ks // 2, ks // 2), mode="reflect")
        k = ns.w.view(1, 1, 1, ks) if axis else ns.w.view(1, 1, ks, 1)
        assert torch.equal(F.conv2d(xp.view(P, 1, xp.shape[2], xp.shape[3]), k).view(P, H, W), ns.out)
    for mut in U.BLUR_MUTANTS:
        bad, _m = U.blur_reference(ns.x, axis, ns.w, mut)
        assert (not torch.equal(bad, ns.out)) == U.blur_mutant_applies(mut, row), mut
    ns = U.blur_case(row, "real")
    assert_within(U.blur_emulate(ns.x, axis, ns.w), ns.out, ns.tol, "blur in f32")


def test_blur_rows_cover_the_edges():
    rows = U.BLUR_ROWS
    assert any(ks // 2 + 1 == (W if axis else H) and ks >= 7 for _p, H, W, axis, ks in rows if axis == 1)
    assert any(ks // 2 + 1 == (W if axis else H) and ks >= 7 for _p, H, W, axis, ks in rows if axis == 0)
    assert any(ks == 3 and (W if axis else H) == 2 for _p, H, W, axis, ks in rows) and any(ks == 1 for r in rows for ks in [r[4]])
    assert any(r[4] % 2 == 0 for r in rows) and {r[0] for r in rows} == {1, 6} and all(r[1] != r[2] for r in rows)
    for ks in (1, 2, 3, 4, 5, 7, 9):
        w = U.dyadic_weights(ks)
        assert float(w.sum()) == 1.0 and float(w.min()) > 0 and torch.equal(w.float().double(), w)
