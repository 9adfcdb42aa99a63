"""Exact and per-element tests of the kernels between the UNet features and the loss: madm_dwconv3x3 (all four variants and the
unforced launch), madm_dwconv3x3_wgrad (plain, lattice, unforced), madm_resize_bilinear / _nchw_f32 / _bwd, madm_softmax_ce,
madm_masked_l1, madm_slide_merge.  Data, references and bounds: tests/spatial_util.py, checked on the host by
test_spatial_exact_host.py, which also holds every row to the variant and tile its name promises.

Layer 1 asserts torch.equal with the exact result rounded once to the dtype; every variant equals it, hence each other.
Layer 2 asserts a tolerance per element against float64, nothing excluded."""
import pytest
import torch

import lattice_util as L
import norm_util as N
import spatial_util as S
from spatial_util import F32, F16, DT3, ID3

pytestmark = pytest.mark.gpu
SENTINEL = -777.0                 # what an output holds before the launch: an element the kernel skips keeps it


def _force(monkeypatch, force):
    if force:
        monkeypatch.setenv("MADM_DWCONV_KERNEL", str(force))
    else:
        monkeypatch.delenv("MADM_DWCONV_KERNEL", raising=False)


def _tokens(t, dtype, pad=0, fill=SENTINEL):
    """[..., C] float64 / int -> [rows, C] device tensor of dtype; ``pad`` > 0: a column window (16-byte aligned) of rows that
    are 2 * pad elements longer and hold ``fill`` around it"""
    r = t.reshape(-1, t.shape[-1]).to(dtype)
    if not pad:
        return r.contiguous().cuda()
    buf = torch.full((r.shape[0], r.shape[1] + 2 * pad), fill, dtype=dtype, device="cuda")
    buf[:, pad:pad + r.shape[1]] = r
    return buf[:, pad:pad + r.shape[1]]


def _same(got, want_dev, want_f64, dtype, what):
    if not torch.equal(got, want_dev):
        L.assert_exact(got.contiguous(), want_f64.reshape(got.shape).double(), dtype, what)


# ---- 1. depthwise conv forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("row", S.DW_ROWS, ids=[r[0] for r in S.DW_ROWS])
def test_depthwise_exact(cuda, monkeypatch, dtype, act, row):
    """Every forced variant and the unforced launch give the exact result rounded once"""
    from madm_amd import ops
    name, B, H, W, d, kind, _tile, variants = row
    C = S.dw_width(kind, dtype)
    ns = S.dw_case(name, C)
    want = S.dw_expected(name, C, act)
    want_dev = want.to(dtype).cuda()
    x = _tokens(ns.x, dtype)
    w, scale, shift = ns.w.float().cuda(), (ns.scale2.float() / 2).cuda(), ns.shift.float().cuda()
    window = name == S.WINDOW_ROW
    for force in S.FORCES:
        _force(monkeypatch, force)
        assert S.dw_plan(dtype, B, H, W, C, d)[0] == variants[force]
        buf = torch.zeros((B * H * W, 3 * C if window else C), dtype=dtype, device="cuda")
        out = buf[:, C:2 * C] if window else buf
        out.fill_(SENTINEL)
        ops.dwconv3x3(x, w, scale, shift, B, H, W, d, act=ops._act_code(act=act), out=out)
        _same(out, want_dev, want, dtype, f"{name} {act} MADM_DWCONV_KERNEL={force} (variant {variants[force]})")
        if window:
            assert float(buf[:, :C].float().abs().sum()) == 0.0 and float(buf[:, 2 * C:].float().abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", S.DW_REAL_ROWS)
def test_depthwise_per_element(cuda, monkeypatch, dtype, name):
    from madm_amd import ops
    ns = S.dw_real_case(name, dtype)
    x = _tokens(ns.x, dtype)
    outs = []
    for force in S.FORCES:
        _force(monkeypatch, force)
        got = ops.dwconv3x3(x, ns.w.float().cuda(), ns.scale.float().cuda(), ns.shift.float().cuda(), ns.B, ns.H, ns.W, ns.d,
                            act=ops._act_code(act="silu"))
        worst = S.assert_within(got.view(ns.B, ns.H, ns.W, ns.C), ns.y, ns.tol, f"{name} MADM_DWCONV_KERNEL={force}")
        print(f"DWCONV {name} {dtype} force {force}: worst error / bound {worst:.3f}")
        outs.append(got)
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "the variants do not give identical bits"


# ---- 2. depthwise weight gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.WG_ROWS, ids=[r[0] for r in S.WG_ROWS])
def test_depthwise_wgrad_exact(cuda, monkeypatch, dtype, row):
    """The default (atomic) weight gradient: plain kernel, lattice kernel forced, unforced launch; into a zero dw and on top of
    an integer-filled one"""
    from madm_amd import ops
    name, B, H, W, d, kind, _tile, variants = row
    C = S.dw_width(kind, dtype)
    ns = S.wgrad_case(name, C)
    x = _tokens(ns.x4, dtype)
    dy = _tokens(ns.dy4, dtype, pad=S.epc(dtype) if name == S.WG_STRIDED_ROW else 0, fill=3.0)
    for force in S.WG_FORCES:
        _force(monkeypatch, force)
        assert S.dw_plan(dtype, B, H, W, C, d, wgrad=True)[0] == variants[force]
        for old in (torch.zeros_like(ns.old), ns.old):
            dw = old.float().cuda()
            ops.dwconv3x3_wgrad(x, dy, B, H, W, d, dw=dw)
            L.assert_exact(dw, old + ns.dw, F32, f"{name} MADM_DWCONV_KERNEL={force} prefilled={bool(old.abs().sum() > 0)}")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", S.DW_REAL_ROWS)
def test_depthwise_wgrad_per_element(cuda, monkeypatch, dtype, name):
    from madm_amd import ops
    ns = S.wgrad_real_case(name, dtype)
    x, dy = _tokens(ns.x, dtype), _tokens(ns.dy, dtype)
    for force in S.WG_FORCES:
        _force(monkeypatch, force)
        got = ops.dwconv3x3_wgrad(x, dy, ns.B, ns.H, ns.W, ns.d)
        worst = S.assert_within(got, ns.ref, ns.tol, f"{name} MADM_DWCONV_KERNEL={force}")
        print(f"DWCONV_WGRAD {name} {dtype} force {force}: worst error / bound {worst:.4f}")


# ---- 3. bilinear resize and its adjoint -------------------------------------------------------------------------------------------------
def _resize(x, row, pad_out=0):
    from madm_amd import ops
    (ih, iw), (oh, ow) = row
    C = x.shape[1]
    buf = torch.full((S.RS_B * oh * ow, C + 2 * pad_out), SENTINEL, dtype=x.dtype, device="cuda")
    out = buf[:, pad_out:pad_out + C]
    ops.resize_bilinear(x, S.RS_B, ih, iw, oh, ow, out=out)
    if pad_out:
        assert bool((buf[:, :pad_out] == SENTINEL).all()) and bool((buf[:, pad_out + C:] == SENTINEL).all())
    return out


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.RS_EXACT, ids=S.rs_id)
def test_resize_exact(cuda, dtype, row):
    """Power-of-two ratios on integer data: forward, NCHW forward (f32) and adjoint equal the exact result rounded once; the
    adjoint identity <resize(x), dy> = <x, bwd(dy)> holds exactly in f32"""
    from madm_amd import ops
    (ih, iw), (oh, ow) = row
    pad = S.epc(dtype) if row == S.RS_WINDOW_ROW else 0
    for C in S.rs_widths(dtype):
        ns = S.rs_exact_case(row, C)
        got = _resize(_tokens(ns.x, dtype, pad), row, pad)
        L.assert_exact(got.contiguous(), ns.y.reshape(-1, C), dtype, f"resize {S.rs_id(row)} C={C}")
        din = ops.resize_bilinear_backward(_tokens(ns.dy, dtype, pad, fill=5.0), S.RS_B, ih, iw, oh, ow)
        L.assert_exact(din, ns.dx.reshape(-1, C), dtype, f"resize adjoint {S.rs_id(row)} C={C}")
        lhs = float((got.double().cpu() * ns.dy.reshape(-1, C)).sum())
        rhs = float((din.double().cpu() * ns.x.reshape(-1, C)).sum())
        if dtype == F32:
            assert lhs == rhs, (lhs, rhs)
            nchw = ops.resize_bilinear_nchw(ns.x.permute(0, 3, 1, 2).float().contiguous().cuda(), oh, ow)
            L.assert_exact(nchw, ns.y.permute(0, 3, 1, 2).contiguous(), F32, f"resize NCHW {S.rs_id(row)}")
        else:                      # the stored halves are rounded: the identity holds up to those roundings
            slack = float((N.half_ulp(ns.y, dtype) * ns.dy.abs()).sum() + (N.half_ulp(ns.dx, dtype) * ns.x.abs()).sum())
            assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.RS_REAL, ids=S.rs_id)
def test_resize_per_element(cuda, dtype, row):
    from madm_amd import ops
    (ih, iw), (oh, ow) = row
    for C in S.rs_widths(dtype):
        x = S.rs_real_input(row, C, dtype)
        ref, tol = S.resize_bound(row, x, dtype)
        worst = S.assert_within(_resize(_tokens(x, dtype), row).view(ref.shape), ref, tol, f"resize {S.rs_id(row)} C={C}")
        dy = S.rs_real_input(row, C, dtype, adjoint=True)
        bref, btol = S.resize_bwd_bound(row, dy, dtype)
        din = ops.resize_bilinear_backward(_tokens(dy, dtype), S.RS_B, ih, iw, oh, ow)
        bworst = S.assert_within(din.view(bref.shape), bref, btol, f"resize adjoint {S.rs_id(row)} C={C}")
        print(f"RESIZE {S.rs_id(row)} {dtype} C={C}: worst error / bound {worst:.3f}, adjoint {bworst:.3f}")
        if dtype == F32 and row == S.RS_NCHW_REAL:
            nchw = ops.resize_bilinear_nchw(x.permute(0, 3, 1, 2).float().contiguous().cuda(), oh, ow)
            S.assert_within(nchw.permute(0, 2, 3, 1), ref, tol, f"resize NCHW {S.rs_id(row)}")


# ---- 4. softmax_ce --------------------------------------------------------------------------------------------------------------------
def _ce(ns, dtype, coef, g, loss=True, grad=True, labels=None, ldd=None):
    """One call: (loss_sum - CE_PREFILL as a float, or None; dlogits [M, ldd] or None)"""
    from madm_amd import ops
    ls = torch.tensor([S.CE_PREFILL], dtype=torch.float64, device="cuda") if loss else None
    gs = torch.tensor([g], dtype=torch.float32, device="cuda") if g is not None else None
    lab = (ns.labels if labels is None else labels).cuda()
    _l, dl = ops.softmax_ce(ns.x.cuda(), ns.K, lab, None if ns.weight is None else ns.weight.cuda(), S.IGNORE, ls, gs, coef,
                            grad_dtype=dtype if grad else None, ldd=ldd)
    return (float(ls.cpu()[0]) - S.CE_PREFILL if loss else None), dl


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("K", S.CE_EXACT_K)
@pytest.mark.parametrize("kind", ["equal", "onehot"])
def test_softmax_ce_exact(cuda, dtype, kind, K):
    """Equal logits: the gradient is coef g w (1 / K - onehot) exactly; one-hot logits: gradient and loss exactly zero.  Columns
    K .. ldd - 1, ignored pixels and labels outside [0, K) are exactly zero; with every pixel ignored loss_sum stays as it was."""
    ns = S.ce_exact_case(kind, K)
    ldd = K + 3
    loss, dl = _ce(ns, dtype, S.CE_COEF, S.CE_G, ldd=ldd)
    L.assert_exact(dl[:, :K].contiguous(), ns.grad, dtype, f"softmax_ce {kind} K={K}")
    assert float(dl[:, K:].float().abs().sum()) == 0.0, "columns K .. ldd - 1"
    if kind == "onehot" or K == 1:
        assert loss == 0.0, loss
    else:
        want, tol, _g, _t = S.ce_bounds(ns, S.CE_COEF, S.CE_G, dtype)
        assert abs(loss - want) <= tol + 2.0 ** -40 * S.CE_PREFILL, (loss, want, tol)
    none = torch.full_like(ns.labels, S.IGNORE)
    loss, dl = _ce(ns, dtype, S.CE_COEF, S.CE_G, labels=none, ldd=ldd)
    assert loss == 0.0 and float(dl.float().abs().sum()) == 0.0, "every pixel ignored"


def _check_ce(ns, dtype, coef, g, what):
    want, tol_l, grad, tol_g = S.ce_bounds(ns, coef, g, dtype)
    loss, dl = _ce(ns, dtype, coef, g, ldd=ns.K + 5)
    slack = 2.0 ** -40 * (S.CE_PREFILL + abs(want))          # the f64 sum on top of the old content of loss_sum
    assert abs(loss - want) <= tol_l + slack, (what, loss, want, tol_l)
    worst = S.assert_within(dl[:, :ns.K], grad, tol_g, what)
    assert float(dl[:, ns.K:].float().abs().sum()) == 0.0
    print(f"SOFTMAX_CE {what}: loss error {abs(loss - want):.3e} of {tol_l + slack:.3e}, gradient worst error / bound {worst:.3f}")
    return loss, dl


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", [r[0] for r in S.CE_REAL_ROWS])
def test_softmax_ce_per_element(cuda, dtype, name):
    """Loss and gradient in one call on a pre-filled loss_sum; the separate calls give the same bits; in f16 also with
    coef * gscale = 2^-16, where the gradients are f16 subnormals and must be the correctly rounded ones"""
    ns = S.ce_real_case(name)
    loss, dl = _check_ce(ns, dtype, ns.coef, ns.g, f"{name} {dtype}")
    only_loss, _n = _ce(ns, dtype, ns.coef, ns.g, grad=False)
    _n, only_grad = _ce(ns, dtype, ns.coef, ns.g, loss=False, ldd=ns.K + 5)
    assert torch.equal(only_grad, dl)
    assert abs(only_loss - loss) <= 2.0 ** -40 * (S.CE_PREFILL + abs(loss))     # (the blocks' atomics land in any order)
    if dtype == F16:
        _check_ce(ns, dtype, S.CE_SUBNORMAL / (1.0 if ns.g is None else ns.g), ns.g, f"{name} f16 subnormal gradients")


def test_softmax_ce_second_grid_stride_trip(cuda):
    """M = 4096 * 256 + 3: the last three pixels are a second trip of the first block's threads"""
    ns = S.ce_real_case(S.CE_BIG_ROW[0])
    assert ns.M > 4096 * 256
    _check_ce(ns, F32, ns.coef, ns.g, S.CE_BIG_ROW[0])


# ---- 5. masked_l1, slide_merge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [False, True], ids=["l1", "l2"])
@pytest.mark.parametrize("row", S.ML_ROWS, ids=S.ml_id)
def test_masked_l1_exact(cuda, row, l2):
    """Dyadic data: the f64 loss sum (on top of a pre-filled value) and the gradient are bit-exact, in one call"""
    from madm_amd import ops
    ns = S.ml_case(row)
    want_l, want_g = ns.out[l2]
    ls = torch.tensor([1024.0], dtype=torch.float64, device="cuda")
    gs = torch.tensor([S.ML_G], dtype=torch.float32, device="cuda")
    mask = None if ns.mask is None else ns.mask.float().contiguous().cuda()
    _l, dp = ops.masked_l1(ns.pred.float().cuda(), ns.gt.float().cuda(), mask, l2=l2, loss_sum=ls, gscale=gs, coef=S.ML_COEF,
                           want_grad=True)
    assert float(ls.cpu()[0]) == 1024.0 + want_l, (float(ls.cpu()[0]) - 1024.0, want_l)
    L.assert_exact(dp, want_g, F32, f"masked_l1 {S.ml_id(row)} l2={l2}")
    assert bool((want_g == 0).any()) and float(dp[ns.d.cuda() == 0].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.SM_ROWS, ids=[r[0] for r in S.SM_ROWS])
def test_slide_merge_exact(cuda, dtype, row):
    """Columns covered 0 (a gap: exactly 0), 1, 2 or 4 times are exact; at 3 the two roundings of sum * fl(1 / 3)"""
    from madm_amd import ops
    for C in S.sm_widths(dtype):
        ns = S.sm_case(row[0], C)
        got = ops.slide_merge(_tokens(ns.win, dtype), ns.nW, ns.B, ns.h, ns.w, ns.Wc, ns.x1).view(ns.B, ns.h, ns.Wc, C)
        exact = ns.cnt != 3
        L.assert_exact(got[:, :, exact.cuda()].contiguous(), ns.ref[:, :, exact], dtype, f"slide_merge {row[0]} C={C}")
        if bool((~exact).any()):
            S.assert_within(got[:, :, (~exact).cuda()], ns.ref[:, :, ~exact], S.sm_tolerance(ns, dtype)[:, :, ~exact],
                            f"slide_merge {row[0]} C={C}, three windows")
