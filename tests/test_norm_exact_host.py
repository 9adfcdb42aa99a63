"""Host-side checks of tests/norm_util.py, which tests/test_norm_exact_gpu.py relies on: the float64 references are
F.group_norm / F.layer_norm and their autograd gradients; every exact row meets the exactness conditions (the builders assert
them on every intermediate) and has the block structure its name promises; the layer-2 bounds accept the reference rounded once
to the dtype and a float32 torch evaluation; and every mutated reference -- a bug a kernel of this family could have -- differs
from the exact one, or leaves the bound in at least one element.  No kernel is involved."""
import pytest
import torch
import torch.nn.functional as F

import norm_util as N
from norm_util import F32, BF16, F16, DT3, ID3


def _tok(x_nchw):
    B, C, H, W = x_nchw.shape
    return x_nchw.permute(0, 2, 3, 1).reshape(B, H * W, C)


# ---- references ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_groupnorm_references_are_torch_in_float64(act):
    g = torch.Generator().manual_seed(1)
    B, C, H, W, G, eps = 2, 48, 3, 5, 4, 1e-5
    x = torch.randn((B, C, H, W), generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    res, dy = (torch.randn((B, C, H, W), generator=g, dtype=torch.float64) for _ in range(2))
    y = N.act_f(F.group_norm(x, G, gamma, beta, eps) + res, act)
    y.backward(dy)
    xt = _tok(x.detach())
    mean, var, rstd = N.real_stats(xt, G, eps)
    sums = [torch.stack([xt.sum(1), (xt * xt).sum(1)], -1)]
    m2, r2 = N.fold_sums(sums, H * W, G, eps)
    assert float((m2 - mean).abs().max()) < 1e-13 and float((r2 / rstd - 1).abs().max()) < 1e-12
    got = N.gn_forward(xt, mean, rstd, gamma.detach(), beta.detach(), act, _tok(res))
    assert float((got - _tok(y.detach())).abs().max()) < 1e-12
    # the backward is stated without the residual input: z + res enters through beta-like shifts only via act', so compare with res = 0
    x.grad = gamma.grad = beta.grad = None
    N.act_f(F.group_norm(x, G, gamma, beta, eps), act).backward(dy)
    bw = N.gn_backward(xt, _tok(dy), mean, rstd, gamma.detach(), beta.detach(), act, dres=_tok(res))
    assert float((bw.dx - _tok(x.grad + res)).abs().max()) < 1e-11
    assert float((bw.dgamma - gamma.grad).abs().max()) < 1e-11 and float((bw.dbeta - beta.grad).abs().max()) < 1e-11
    assert torch.equal(bw.bsums[..., 0].sum(0), bw.dbeta) and torch.equal(bw.bsums[..., 1].sum(0), bw.dgamma)


def test_layernorm_references_are_torch_in_float64():
    g = torch.Generator().manual_seed(2)
    M, C, eps = 7, 40, 1e-5
    x = torch.randn((M, C), generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dy, dres = (torch.randn((M, C), generator=g, dtype=torch.float64) for _ in range(2))
    y = F.layer_norm(x, (C,), gamma, beta, eps)
    y.backward(dy)
    assert float((N.ln_forward(x.detach(), gamma.detach(), beta.detach(), eps) - y.detach()).abs().max()) < 1e-12
    bw = N.ln_backward(x.detach(), dy, gamma.detach(), eps, dres)
    assert float((bw.dx - (x.grad + dres)).abs().max()) < 1e-11
    assert float((bw.dgamma - gamma.grad).abs().max()) < 1e-11 and float((bw.dbeta - beta.grad).abs().max()) < 1e-11


# ---- exactness conditions on every row ----------------------------------------------------------------------------------------------
def test_stats_rows_have_the_blocks_their_names_promise():
    assert N.stats_blocks(1, 9) == (1, 9)
    assert N.stats_blocks(3, 37) == (1, 37)              # 5 chunks: 51 row lanes, thread 255 idle
    assert 256 // 5 == 51 and 51 * 5 == 255
    assert N.stats_blocks(1, 130) == (3, 44) and 130 - 2 * 44 == 42
    assert N.stats_blocks(2, 601) == (10, 61) and 601 - 9 * 61 == 52


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", N.STATS_ROWS, ids=[r[0] for r in N.STATS_ROWS])
def test_stats_rows_are_exact(row, dtype):
    ns = N.stats_case(row[0], row[3] * N.epc(dtype))     # (the builder asserts the partial sums)
    s = N.stats_sums(ns)
    assert torch.equal(s[..., 0], ns.x.sum(1)) and torch.equal(s[..., 1], (ns.x ** 2).sum(1))
    assert N.quantum_exp(ns.x) == 3 and float(ns.x.abs().max()) <= 2.0
    w = torch.ones((ns.B, ns.HW), dtype=torch.float64)
    w[ns.B - 1, ns.HW // 2] = 0.0
    assert not torch.equal(N.stats_sums(ns, w), s), "one row dropped goes unseen"


def test_apply_rows_have_the_structure_their_names_promise():
    rows = {r[0]: r for r in N.GN_ROWS}
    assert 320 // 32 == 10 and 10 % 4 != 0                               # 16-byte chunks of four / eight straddle groups
    assert 128 // 1 > 80                                                 # the fold's tail loop
    _n, B, HW, cins, G = rows["straddle4"]
    cpg = sum(cins) // G
    assert cpg < cins[0] < 2 * cpg                                       # group 1 holds channels of both sources
    assert rows["g64_per_channel"][4] == 64 and sum(rows["g64_per_channel"][3]) == 64
    for name in ("one_group_tail", "pow2_count"):
        _n, B, HW, cins, G = rows[name]
        assert N.is_pow2(HW * sum(cins) // G)
    for dt in DT3:
        B, HW, cins, G = N.gn_row(N.BIG_ROW[0], dt)
        strips, total = N.apply_strips(B, HW, cins[0] // N.epc(dt))
        assert (strips, total) == (8, 8320) and total > strips * 256 * 4 and B * HW * cins[0] <= 17_100_000


@pytest.mark.parametrize("row", N.GN_ROWS, ids=[r[0] for r in N.GN_ROWS])
def test_groupnorm_rows_are_exact(row):
    """forward in both orders of evaluation, finalize, backward: every intermediate representable (f16 for the forward, whose
    fused form runs in packed f16), every partial sum below 2^24, forward outputs representable in all three dtypes"""
    name = row[0]
    ns = N.gn_case(name)
    N.check_handed(ns)
    for t in (ns.x, ns.res, ns.dy, ns.dres, ns.gamma, ns.beta):
        N.need(t, BF16, "input")
    for act in N.ACTS:
        for with_res in (False, True):
            y = N.gn_forward_case(ns, act, with_res)
            for dt in DT3:
                N.need(y, dt, f"{name} {act} output")
            assert L_nonzero(y) >= (0.3 if act == "relu" else 0.85)
    sc, sh = N.finalize_reference(ns)
    N.need(sc, F32, "scale"), N.need(sh, F32, "shift")
    nb = N.gn_case(name, paired=True)
    N.check_handed(nb)
    for act in N.ACTS:
        bw = N.gn_backward_case(nb, act, True)            # (asserts)
        assert L_nonzero(bw.dx) >= 0.5
        if nb.cpg > 1:      # (one channel per group: the pixel pairs that clear A_g and B_g clear the channel's own sums too)
            assert L_nonzero(bw.dgamma) >= 0.5 and L_nonzero(bw.dbeta) >= 0.5
        if nb.coarse:
            assert L_nonzero(bw.kA) >= 0.5 and L_nonzero(bw.kB) >= 0.5
        else:
            assert float(bw.kA.abs().max()) == 0.0 and float(bw.kB.abs().max()) == 0.0


def L_nonzero(t):
    return float((t != 0).double().mean())


@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("row", N.CONV_GN_ROWS, ids=[r[0] for r in N.CONV_GN_ROWS])
def test_fused_conv_rows_are_exact(row, act):
    ref = N.conv_gn_reference(row[0], act)                # (asserts Kred amp_a amp_b < 2^24 and the intermediates)
    N.check_handed(ref)
    assert row[5] <= 128 and all(t in N.HALO_NAMES for t in row[6])
    assert L_nonzero(ref.out) >= 0.5
    border = ref.out[:, :, 0, :]
    assert not torch.equal(N.conv_gn_reference(row[0], act, "pad_before_act").out[:, :, 0, :], border)
    inner = slice(1, -1)
    assert torch.equal(N.conv_gn_reference(row[0], act, "pad_before_act").out[:, :, inner, inner], ref.out[:, :, inner, inner])


def test_fused_conv_rows_cover_every_halo_tile():
    assert {t for r in N.CONV_GN_ROWS for t in r[6]} == set(N.HALO_NAMES)
    assert any(len(r[2]) == 2 for r in N.CONV_GN_ROWS if 12 in r[6])


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_layernorm_rows_are_exact(dtype):
    for C in N.ln_widths(dtype):
        for M in N.LN_M:
            ns = N.ln_case(M, C)
            y, bw = N.ln_exact(ns)                        # (asserts)
            ref = F.layer_norm(ns.x, (C,), ns.gamma, ns.beta, 0.0)
            assert float((y - ref).abs().max()) < 1e-12
            assert bool((bw.m1 != 0).any()) == ns.pow2
    ns = N.ln_case(N.LN_STRIDE_ROW, 2 * N.epc(dtype))
    N.ln_exact(ns)
    assert -(-N.LN_STRIDE_ROW // 4) > 128
    r = N.ln_fold_reference()
    assert L_nonzero(r.out) >= 0.5


# ---- layer 2: the bounds accept the reference rounded once and a float32 torch evaluation -------------------------------------------
def _l2_data(dtype, B=2, HW=35, C=64, seed=5):
    x = N.quantised((B, HW, C), seed, dtype, 1.5, 0.3)
    res = N.quantised((B, HW, C), seed + 1, dtype)
    dy = N.quantised((B, HW, C), seed + 2, dtype)
    g = torch.Generator().manual_seed(seed + 3)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).float().double()
    beta = (0.3 * torch.randn(C, generator=g)).float().double()
    return x, res, dy, gamma, beta


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_forward_bound_accepts_rounding_and_float32(dtype, act):
    G, eps = 32, 1e-5
    x, res, dy, gamma, beta = _l2_data(dtype)
    mean, var, rstd = N.real_stats(x, G, eps)
    ref = N.gn_forward(x, mean, rstd, gamma, beta, act, res)
    tol = N.gn_forward_bound(x, gamma, beta, G, eps, act, res, dtype, n_terms=x.shape[1])
    assert N.assert_within(N.rounded(ref, dtype), ref, tol, "rounded once") <= 1.0
    y32 = N.act_f(F.group_norm(x.float().permute(0, 2, 1), G, gamma.float(), beta.float(), eps).permute(0, 2, 1) + res.float(), act)
    N.assert_within(y32.to(dtype), ref, tol, "float32 torch")
    big = ref.abs() > 0.1                                   # no slack beyond the stated terms
    if dtype == F32:
        assert float((tol / ref.abs())[big].median()) < 3e-5
    else:
        assert float((tol / N.half_ulp(ref, dtype))[big].median()) < 1.1


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", ["none", "silu"])
def test_backward_bound_accepts_rounding_and_float32(dtype, act):
    G, eps = 32, 1e-5
    x, res, dy, gamma, beta = _l2_data(dtype)
    bd = N.gn_backward_bound(x, dy, gamma, beta, G, eps, act, res, dtype, n_terms=x.shape[1], n_sum=x.shape[1])
    N.assert_within(N.rounded(bd.out, dtype), bd.out, bd.tol_dx, "dx rounded once")
    N.assert_within(bd.ref.dgamma.float(), bd.ref.dgamma, bd.tol_dgamma, "dgamma rounded once")
    xr = x.float().permute(0, 2, 1).clone().requires_grad_(True)
    g32, b32 = gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    N.act_f(F.group_norm(xr, G, g32, b32, eps), act).backward(dy.float().permute(0, 2, 1))
    N.assert_within((xr.grad.permute(0, 2, 1) + res.float()).to(dtype), bd.out, bd.tol_dx, "dx float32 torch")
    N.assert_within(g32.grad, bd.ref.dgamma, bd.tol_dgamma, "dgamma float32 torch")
    N.assert_within(b32.grad, bd.ref.dbeta, bd.tol_dbeta, "dbeta float32 torch")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_layernorm_and_softmax_bounds_accept_rounding_and_float32(dtype):
    x = N.quantised((9, 320), 9, dtype, 1.5, 0.5)
    _x, _r, _d, gamma, beta = _l2_data(dtype, C=320)
    ref = N.ln_forward(x, gamma, beta, 1e-5)
    tol = N.ln_forward_bound(x, gamma, beta, 1e-5, dtype)
    N.assert_within(N.rounded(ref, dtype), ref, tol, "rounded once")
    N.assert_within(F.layer_norm(x.float(), (320,), gamma.float(), beta.float(), 1e-5).to(dtype), ref, tol, "float32 torch")
    for L_ in N.SOFTMAX_L:
        for scale in (1.0, 512 ** -0.5):
            s = N.softmax_case(L_, scale)
            p, tol, rel = N.softmax_bound(s, scale, dtype)
            N.assert_within(N.rounded(p, dtype), p, tol, "softmax rounded once")
            N.assert_within(torch.softmax(s * scale, 1).to(dtype), p, tol, "softmax float32 torch")
            assert float(rel.max()) < 1e-4


def test_half_ulp():
    v = torch.tensor([1.0, 1.5, 2.0, 0.0, 3e-6, 300.0], dtype=torch.float64)
    assert N.half_ulp(v, BF16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -134, 2.0 ** -27, 1.0]
    assert N.half_ulp(v, F16)[:5].tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25]
    assert N.half_ulp(v, F32)[:3].tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23]
    for dt in (BF16, F16):       # the worst rounding error of a random tensor IS within half an ulp, and reaches 90 % of it
        x = torch.randn(100000, generator=torch.Generator().manual_seed(3)).double()
        r = ((x.to(dt).double() - x).abs() / N.half_ulp(x, dt)).max()
        assert 0.9 < float(r) <= 1.0


# ---- negative controls --------------------------------------------------------------------------------------------------------------
FWD_MUTANTS = ["group_off_by_one", "c_off_ignored", "next_image", "second_source_offset", "count_from_c1", "no_eps", "res_after_act"]


def _mutated_forward(ns, act, mut):
    if mut in ("second_source_offset", "count_from_c1", "no_eps"):
        mean, rstd = N.fold_sums(ns.sums, ns.HW, ns.G, ns.eps, mut)
        return N.gn_forward(ns.x, mean, rstd, ns.gamma, ns.beta, act, ns.res)
    return N.gn_forward_case(ns, act, True, mut, exact=False)


@pytest.mark.parametrize("mut", FWD_MUTANTS)
def test_layer1_forward_negative_controls(mut):
    """On the exact rows every mutant changes the f32 bit pattern of at least one output (of EVERY row it applies to)."""
    seen = 0
    for row in N.GN_ROWS:
        ns = N.gn_case(row[0])
        two = len(ns.cins) == 2
        if (mut in ("c_off_ignored", "second_source_offset", "count_from_c1") and not two) or (mut == "next_image" and ns.B < 2) \
                or (mut == "group_off_by_one" and ns.G == 1):
            continue
        for act in N.ACTS:
            want = N.gn_forward_case(ns, act, True)
            got = _mutated_forward(ns, act, mut)
            if mut == "res_after_act" and act == "none":
                assert torch.equal(got, want)
                continue
            assert not torch.equal(got.float(), want.float()), (row[0], act, mut)
            seen += 1
    assert seen >= 2


@pytest.mark.parametrize("mut", ["A_dropped", "B_dropped", "dgamma_dbeta_swapped", "row_dropped"])
def test_layer1_backward_negative_controls(mut):
    seen = 0
    for row in N.GN_ROWS:
        ns = N.gn_case(row[0], paired=True)
        if mut in ("A_dropped", "B_dropped") and not ns.coarse:
            continue                                      # (A_g = B_g = 0 there by construction)
        if mut not in ("A_dropped", "B_dropped") and ns.cpg == 1:
            continue                                      # (pixel pairs: the channel's own sums are zero too)
        want = N.gn_backward_case(ns, "relu", True)
        if mut == "row_dropped":
            w = torch.ones((ns.B, ns.HW), dtype=torch.float64)
            w[ns.B - 1, ns.HW // 2] = 0.0
            got = N.gn_backward_case(ns, "relu", True, weight=w)
            assert not torch.equal(got.bsums, want.bsums) and not torch.equal(got.dgamma.float(), want.dgamma.float())
        else:
            got = N.gn_backward_case(ns, "relu", True, mut=mut)
            if mut == "dgamma_dbeta_swapped":
                assert not torch.equal(got.dgamma.float(), want.dgamma.float())
            else:
                assert not torch.equal(got.dx.float(), want.dx.float())
        seen += 1
    assert seen >= 2
    ns = N.ln_case(5, 512)
    y, want = N.ln_exact(ns)
    if mut != "row_dropped":
        _y, got = N.ln_exact(ns, mut=mut)
        assert not (torch.equal(got.dx, want.dx) and torch.equal(got.dgamma, want.dgamma))


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_layer2_negative_controls_leave_the_bound(dtype):
    """On random data each of these mutants is outside the per-element bound somewhere, in every dtype."""
    G, eps = 4, 1e-5
    x, res, dy, gamma, beta = _l2_data(dtype, B=2, HW=35, C=64 + 128, seed=21)
    HW, C1 = x.shape[1], 64
    mean, var, rstd = N.real_stats(x, G, eps)
    sums = list(torch.split(torch.stack([x.sum(1), (x * x).sum(1)], -1), [C1, 128], 1))
    for act in ("relu", "silu"):
        ref = N.gn_forward(x, mean, rstd, gamma, beta, act, res)
        tol = N.gn_forward_bound(x, gamma, beta, G, eps, act, res, dtype, n_terms=HW)
        muts = {m: N.gn_forward(x, mean, rstd, gamma, beta, act, res, m, C1=C1)
                for m in ("group_off_by_one", "c_off_ignored", "next_image", "res_after_act")}
        for m in ("second_source_offset", "count_from_c1"):
            mm, rr = N.fold_sums(sums, HW, G, eps, m)
            muts[m] = N.gn_forward(x, mm, rr, gamma, beta, act, res)
        xd = x.clone()
        xd[1, HW // 2] = 0.0                                # one row dropped from the sums: count unchanged
        mm, rr = N.fold_sums([torch.stack([xd.sum(1), (xd * xd).sum(1)], -1)], HW, G, eps)
        muts["row_dropped"] = N.gn_forward(x, mm, rr, gamma, beta, act, res)
        for m, got in muts.items():
            with pytest.raises(AssertionError):
                N.assert_within(got, ref, tol, m)
    for act in ("none", "silu"):
        bd = N.gn_backward_bound(x, dy, gamma, beta, G, eps, act, res, dtype, n_terms=HW, n_sum=HW)
        for m in ("A_dropped", "B_dropped"):
            got = N.gn_backward(x, dy, mean, rstd, gamma, beta, act, res, m)
            with pytest.raises(AssertionError):
                N.assert_within(got.dx, bd.out, bd.tol_dx, m)
        sw = N.gn_backward(x, dy, mean, rstd, gamma, beta, act, res, "dgamma_dbeta_swapped")
        with pytest.raises(AssertionError):
            N.assert_within(sw.dgamma, bd.ref.dgamma, bd.tol_dgamma, "swapped")
    # eps omitted: visible where the output type resolves it (f32), and in every dtype on the exact rows (above)
    if dtype == F32:
        xs = x * 0.01                                       # variance 2e-4: eps = 1e-5 is 5 % of it
        ms, vs, rs = N.real_stats(xs, G, eps)
        ref = N.gn_forward(xs, ms, rs, gamma, beta, "none")
        tol = N.gn_forward_bound(xs, gamma, beta, G, eps, "none", None, dtype, n_terms=HW)
        with pytest.raises(AssertionError):
            N.assert_within(N.gn_forward(xs, ms, vs ** -0.5, gamma, beta, "none"), ref, tol, "no eps")
