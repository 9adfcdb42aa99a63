"""Host-side half of the exact / per-element tests of the head's spatial and loss kernels (tests/spatial_util.py): no kernel runs.
It shows that every reference equals torch in float64, that the builders assert their exactness conditions, that
madm_dwconv3x3_plan -- the function both depthwise launchers call -- gives every named row the variant and tile its name
promises (the unforced rows included: a moved threshold fails here instead of silently testing another kernel), that every
mutant is rejected on every row it applies to, and that every layer-2 bound accepts a float32 torch evaluation and the
reference rounded once."""
import pytest
import torch
import torch.nn.functional as F

import norm_util as N
import spatial_util as S
from spatial_util import F32, BF16, F16, DT3, ID3


def _inside(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


# ---- 0. the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.DW_ROWS, ids=[r[0] for r in S.DW_ROWS])
def test_forward_rows_reach_the_variant_and_tile_they_promise(dtype, row):
    name, B, H, W, d, kind, tile, variants = row
    C = S.dw_width(kind, dtype)
    slabs = C // (8 * S.epc(dtype))
    for force in S.FORCES:
        p = S.dw_plan(dtype, B, H, W, C, d, force=force)
        assert p[0] == variants[force], (name, force, p)
        if p[0] == 4:
            assert p[1:5] == tile and p[5] == B * d * d * tile[0] * tile[1] * slabs, (name, force, p)
        elif p[0] in (2, 3):
            assert W >= 4 * d and p[1] == 0 and p[2] == -(-(-(-W // d)) // 4) and p[4] == 4, (name, force, p)
            assert p[0] == 2 or (C // S.epc(dtype)) % 8 == 0
        else:
            assert p[1:5] == (0, 0, 0, 0) and p[5] >= 1
    if tile is None:
        assert C % (8 * S.epc(dtype)) != 0 or d == 1, "the row says the lattice kernel does not fit"
    if name == "full_tile":
        assert S.dw_plan(dtype, B, H, W, C, d, force=4)[1:5] == (1, 1, 15, 15)
    if name == "auto_lattice":
        assert B * H * W * C // S.epc(dtype) == 1 << 21 and S.dw_plan(dtype, B, H, W, C, d, force=0)[0] == 4
    if name == "auto_comb_xcd":
        assert S.dw_plan(dtype, B, H, W, C, d, force=0)[0] == 3


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.WG_ROWS, ids=[r[0] for r in S.WG_ROWS])
def test_wgrad_rows_reach_the_variant_and_tile_they_promise(dtype, row):
    name, B, H, W, d, kind, tile, variants = row
    C = S.dw_width(kind, dtype)
    for force in S.WG_FORCES:
        p = S.dw_plan(dtype, B, H, W, C, d, wgrad=True, force=force)
        assert p[0] == variants[force], (name, force, p)
        if p[0] == 4:
            assert p[1:5] == tile and p[5] == B * d * d * (C // (8 * S.epc(dtype))), (name, force, p)
        else:
            assert p[1] == 0 and p[3:5] == (0, 0) and p[2] >= 64 and p[5] == -(-B * H * W // p[2]), (name, force, p)
    for force in (2, 3):                                       # any other value forbids the lattice kernel
        assert S.dw_plan(dtype, B, H, W, C, d, wgrad=True, force=force)[0] == 1
    if name == "auto_wgrad_lattice":
        p = S.dw_plan(dtype, B, H, W, C, d, wgrad=True, force=0)
        assert p[0] == 4 and p[1] * p[2] == 25


def test_plan_reads_the_environment_on_every_call(monkeypatch):
    args = (F16, 1, 30, 30, 128, 2)
    monkeypatch.delenv("MADM_DWCONV_KERNEL", raising=False)
    assert S.dw_plan(*args)[0] == 2
    monkeypatch.setenv("MADM_DWCONV_KERNEL", "4")
    assert S.dw_plan(*args)[:5] == (4, 1, 1, 15, 15)
    monkeypatch.setenv("MADM_DWCONV_KERNEL", "1")
    assert S.dw_plan(*args)[0] == 1
    from madm_amd._lib import lib
    assert lib.madm_dwconv3x3_plan(2, 1, 30, 30, 12, 2, (S.ctypes.c_int * 6)(), 0) < 0      # C no multiple of the chunk
    assert lib.madm_dwconv3x3_plan(7, 1, 30, 30, 128, 2, (S.ctypes.c_int * 6)(), 0) < 0


def test_production_shapes_take_the_full_tile():
    """The head's 512 x 512 maps, 2 x 1024 channels f16: th = tw = 15 at dilations 6, 12, 18 (ny = 2 with a last tile of 14 rows
    at 18), forward on the lattice at all three, the weight gradient only where a class has at least nine tiles"""
    for d, n, wg in ((6, 6, 4), (12, 3, 4), (18, 2, 1)):
        assert S.dw_plan(F16, 2, 512, 512, 1024, d, force=0)[:5] == (4, n, n, 15, 15)
        assert S.dw_plan(F16, 2, 512, 512, 1024, d, wgrad=True, force=0)[0] == wg
    assert -(-512 // 18) == 29 and S.dw_row("full_tile_seams")[6][:1] + S.dw_row("full_tile_seams")[6][2:3] == (2, 15)


# ---- 1. depthwise forward -------------------------------------------------------------------------------------------------------------
def _torch_dw(x, w, scale, shift, d, act):
    """x [B, H, W, C], w [9, C] -> [B, H, W, C] through F.conv2d in float64"""
    C = x.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2), w.t().reshape(C, 1, 3, 3), None, padding=d, dilation=d, groups=C)
    return N.act_f(y * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1), act).permute(0, 2, 3, 1)


@pytest.mark.parametrize("C", [128, 32, 4])
@pytest.mark.parametrize("name", S.DW_SMALL)
def test_depthwise_reference_equals_torch_and_rejects_every_mutant(name, C):
    kind = S.dw_row(name)[5]
    if (kind == "c128") != (C == 128) or (kind == "slab" and C != 32) or (kind == "chunk" and C != 4):
        return
    ns = S.dw_case(name, C)
    chs = 32
    for act in N.ACTS:
        want = S.dw_forward(ns, act).double()
        assert torch.equal(want, _torch_dw(ns.x.double(), ns.w.double(), ns.scale2.double() / 2, ns.shift.double(), ns.d, act))
        N.need(want, F16, "output")                          # half-integers below 2048; bf16 rounds them (once)
        for mut in S.DW_MUTANTS:
            if S.dw_mutant_applies(mut, ns, chs):
                assert not torch.equal(S.dw_forward(ns, act, mut, chs).double(), want), (name, act, mut)
    applied = [m for m in S.DW_MUTANTS if S.dw_mutant_applies(m, ns, chs)]
    assert applied, name


def test_every_depthwise_mutant_applies_somewhere_and_the_big_rows_share_the_statement():
    seen = set()
    for name in S.DW_SMALL:
        ns = S.dw_case(name, 128 if S.dw_row(name)[5] == "c128" else 32)
        seen |= {m for m in S.DW_MUTANTS if S.dw_mutant_applies(m, ns, 32)}
    assert seen == set(S.DW_MUTANTS)
    # the 16 M-element rows run the same statement; here at two slabs, with the mutants their tiles admit
    for name in ("auto_lattice", "auto_comb_xcd"):
        ns = S.dw_case(name, 64)
        want = S.dw_forward(ns, "none").double()
        assert torch.equal(want, _torch_dw(ns.x.double(), ns.w.double(), ns.scale2.double() / 2, ns.shift.double(), ns.d, "none"))
        for mut in S.DW_MUTANTS:
            if S.dw_mutant_applies(mut, ns, 32):
                assert not torch.equal(S.dw_forward(ns, "none", mut, 32).double(), want), (name, mut)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", S.DW_REAL_ROWS)
def test_depthwise_bound_accepts_float32_and_the_rounded_reference(name, dtype):
    ns = S.dw_real_case(name, dtype)
    assert torch.allclose(ns.y, _torch_dw(ns.x, ns.w, ns.scale, ns.shift, ns.d, "silu"), rtol=1e-12, atol=1e-13)
    y32 = _torch_dw(ns.x.float(), ns.w.float(), ns.scale.float(), ns.shift.float(), ns.d, "silu")
    assert _inside(N.rounded(y32.double(), dtype), ns.y, ns.tol) and _inside(N.rounded(ns.y, dtype), ns.y, ns.tol)
    assert float((ns.tol / (ns.y.abs() + 1)).max()) < (1e-4 if dtype == F32 else 1e-2), "the bound says nothing"
    wrong = ns.y.clone()
    wrong[0, 3, 5, 7] += 8 * float(ns.tol[0, 3, 5, 7])
    assert not _inside(wrong, ns.y, ns.tol)


# ---- 2. depthwise weight gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.WG_SMALL)
def test_wgrad_reference_and_mutants(name):
    kind = S.dw_row(name, S.WG_ROWS)[5]
    ns = S.wgrad_case(name, 128 if kind == "c128" else 32)
    x, dy = ns.x4.double(), ns.dy4.double()
    assert torch.equal(S.wgrad_sum(x, dy, ns.d), ns.dw)                                   # (det_util holds ns.dw to autograd)
    assert torch.equal(S.wgrad_sum_sliced(ns.x4.to(torch.int32), ns.dy4.to(torch.int32), ns.d).double(), ns.dw)
    assert float(ns.det.terms.abs().sum(2).max()) * 4 < S.ACC_MAX and bool(torch.equal(ns.old, ns.old.round()))
    for mut in S.WG_MUTANTS:
        if S.wgrad_mutant_applies(mut, ns):
            assert not torch.equal(S.wgrad_mutant(ns, mut), ns.dw), (name, mut)
    assert S.wgrad_mutant_applies("tile_skipped", ns)


def test_every_wgrad_mutant_applies_somewhere():
    seen = set()
    for name in S.WG_SMALL:
        _n, _B, H, W, d, _k, tile, _v = S.dw_row(name, S.WG_ROWS)
        seen |= {m for m in S.WG_MUTANTS if S.wgrad_mutant_applies(m, S.SimpleNamespace(tile=tile, H=H, W=W, d=d))}
    assert seen == set(S.WG_MUTANTS)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", S.DW_REAL_ROWS)
def test_wgrad_bound_accepts_float32(name, dtype):
    ns = S.wgrad_real_case(name, dtype)
    C = ns.C
    wr = torch.zeros((C, 1, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(ns.x.permute(0, 3, 1, 2), wr, padding=ns.d, dilation=ns.d, groups=C).backward(ns.dy.permute(0, 3, 1, 2))
    assert torch.allclose(wr.grad.reshape(C, 9).t(), ns.ref, rtol=1e-12, atol=1e-12)
    w32 = torch.zeros((C, 1, 3, 3), requires_grad=True)
    F.conv2d(ns.x.float().permute(0, 3, 1, 2), w32, padding=ns.d, dilation=ns.d, groups=C).backward(ns.dy.float().permute(0, 3, 1, 2))
    assert _inside(w32.grad.reshape(C, 9).t(), ns.ref, ns.tol) and _inside(ns.ref.float(), ns.ref, ns.tol)
    assert float((ns.tol / S.wgrad_sum(ns.x.abs(), ns.dy.abs(), ns.d)).max()) < 1e-3


# ---- 3. resize ----------------------------------------------------------------------------------------------------------------------
def _interp(x, oh, ow):
    """x [B, IH, IW, C] through F.interpolate in x's precision"""
    return F.interpolate(x.permute(0, 3, 1, 2), size=(oh, ow), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def _interp_adjoint(dy, ih, iw):
    B, oh, ow, C = dy.shape
    x = torch.zeros((B, ih, iw, C), dtype=dy.dtype, requires_grad=True)
    _interp(x, oh, ow).backward(dy)
    return x.grad


@pytest.mark.parametrize("row", S.RS_EXACT, ids=S.rs_id)
def test_exact_resize_rows_are_dyadic_and_equal_torch(row):
    (ih, iw), (oh, ow) = row
    for C in (12, 24):
        ns = S.rs_exact_case(row, C)
        assert S.quantum_exp(ns.My) <= 4 and S.quantum_exp(ns.Mx) <= 4                   # only dyadic entries
        assert torch.equal(ns.My.sum(1), torch.ones(oh).double()) and torch.equal(ns.Mx.sum(1), torch.ones(ow).double())
        assert torch.equal(ns.y, _interp(ns.x, oh, ow)) and torch.equal(ns.dx, _interp_adjoint(ns.dy, ih, iw))
        assert float((ns.y * ns.dy).sum()) == float((ns.x * ns.dx).sum())               # the adjoint identity, exactly
        assert float(ns.x.abs().max()) <= 64 and float(ns.dy.abs().max()) <= 8
        for mut in S.RS_MUTANTS + S.RS_ADJ_MUTANTS:
            if S.rs_mutant_applies(mut, row):
                My, Mx = S.rs_matrices(row, mut)
                if mut not in S.RS_ADJ_MUTANTS:
                    assert not torch.equal(S.rs_apply(My, Mx, ns.x), ns.y), (row, mut)
                assert not torch.equal(S.rs_adjoint(My, Mx, ns.dy), ns.dx), (row, mut)


def test_every_resize_mutant_applies_on_an_exact_and_on_a_real_row():
    for rows in (S.RS_EXACT, S.RS_REAL):
        assert all(any(S.rs_mutant_applies(m, r) for r in rows) for m in S.RS_MUTANTS + S.RS_ADJ_MUTANTS)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", S.RS_REAL, ids=S.rs_id)
def test_resize_bounds_accept_float32_interpolate(row, dtype):
    (ih, iw), (oh, ow) = row
    C = S.rs_widths(dtype)[0]
    x = S.rs_real_input(row, C, dtype)
    ref, tol = S.resize_bound(row, x, dtype)
    assert torch.allclose(ref, _interp(x, oh, ow), rtol=1e-12, atol=1e-13)
    assert _inside(N.rounded(_interp(x.float(), oh, ow).double(), dtype), ref, tol) and _inside(N.rounded(ref, dtype), ref, tol)
    for mut in S.RS_MUTANTS:
        if S.rs_mutant_applies(mut, row):
            assert not _inside(S.rs_apply(*S.rs_matrices(row, mut), x), ref, tol), (row, mut)
    dy = S.rs_real_input(row, C, dtype, adjoint=True)
    ref, tol = S.resize_bwd_bound(row, dy, dtype)
    assert torch.allclose(ref, _interp_adjoint(dy, ih, iw), rtol=1e-12, atol=1e-13)
    assert _inside(N.rounded(_interp_adjoint(dy.float(), ih, iw).double(), dtype), ref, tol) and _inside(N.rounded(ref, dtype), ref, tol)
    for mut in S.RS_MUTANTS + S.RS_ADJ_MUTANTS:
        if S.rs_mutant_applies(mut, row):
            assert not _inside(S.rs_adjoint(*S.rs_matrices(row, mut), dy), ref, tol), (row, mut)


def test_resize_float32_coordinates_differ_from_float64_by_design():
    """Why the layer-2 bound has a coordinate term: F.interpolate in float32 sits further from the float64 result than the
    f32 roundings of the weighted sum alone explain at 30 x 50 -> 61 x 67, and inside the bound with the term."""
    row = S.RS_NCHW_REAL
    x = S.rs_real_input(row, 12, F32)
    ref, tol = S.resize_bound(row, x, F32)
    err = (_interp(x.float(), *row[1]).double() - ref).abs()
    plain = N.half_ulp(ref, F32) + S.U32 * S.RESIZE_ROUNDINGS * S.rs_apply(*(m.abs() for m in S.rs_matrices(row)), x.abs())
    assert bool((err <= tol).all()) and float((err / plain).max()) > 1
    print(f"RESIZE f32 F.interpolate vs f64: max err {float(err.max()):.3e}, max err / plain bound {float((err / plain).max()):.2f}, "
          f"max err / full bound {float((err / tol).max()):.2f}")


# ---- 4. softmax_ce --------------------------------------------------------------------------------------------------------------------
def _torch_ce(x, K, labels, weight, coef, g):
    xk = x[:, :K].clone().requires_grad_(True)
    lab = torch.where((labels >= 0) & (labels < K), labels, torch.full_like(labels, S.IGNORE))     # torch refuses other labels
    per = F.cross_entropy(xk, lab, reduction="none", ignore_index=S.IGNORE)
    w = torch.ones_like(per) if weight is None else weight.to(per.dtype)
    loss = (per * w).sum()
    (loss * coef * g).backward()
    return float(loss.detach()), xk.grad


@pytest.mark.parametrize("name", [r[0] for r in S.CE_REAL_ROWS])
def test_ce_reference_equals_torch_and_bounds_accept_float32(name):
    ns = S.ce_real_case(name)
    g = 1.0 if ns.g is None else ns.g
    for dtype, cg in ((F32, None), (BF16, None), (F16, None), (F16, S.CE_SUBNORMAL)):
        coef, gg = (ns.coef, ns.g) if cg is None else (cg / g, ns.g)
        loss, tol_l, grad, tol_g = S.ce_bounds(ns, coef, gg, dtype)
        tl, tg = _torch_ce(ns.x.double(), ns.K, ns.labels, ns.weight, coef, g)
        assert abs(tl - loss) <= 1e-12 * max(1.0, abs(loss)) and torch.allclose(tg, grad, rtol=1e-11, atol=1e-30)
        l32, g32 = _torch_ce(ns.x, ns.K, ns.labels, ns.weight, coef, g)
        assert abs(l32 - loss) <= tol_l + 2.0 ** -22 * abs(loss), (name, l32, loss, tol_l)    # (torch sums the f32 terms in f32)
        assert _inside(N.rounded(g32.double(), dtype), grad, tol_g) and _inside(N.rounded(grad, dtype), grad, tol_g)
        if cg is not None and ns.weight is not None and float(ns.weight.abs().sum()) > 0:
            nz = grad[grad != 0].abs()
            frac = float((nz >= 2.0 ** -24).double().mean())
            assert float(nz.max()) <= 2.0 ** -15 and frac > 0.3, f"not in the f16 subnormal range: {float(nz.max())}, {frac}"
        if ns.weight is None or float(ns.weight.abs().sum()) > 0:
            for mut in S.CE_MUTANTS:
                if mut == "weight_of_previous_pixel" and (ns.weight is None or ns.M == 1):
                    continue
                if mut == "gscale_twice" and ns.g is None:
                    continue
                if mut == "mean_over_valid" and ns.M == 1:
                    continue
                ml, mg = S.ce_reference(ns.x.double(), ns.K, ns.labels, ns.weight, coef, g, mut)
                if mut == "max_not_subtracted":
                    offsets = float(ns.x.abs().max()) > 1e3
                    assert bool(torch.isnan(mg).any()) == offsets, (name, mut)           # must overflow on the offset rows
                    continue
                differs = not _inside(mg, grad, tol_g)
                if mut == "ignore_not_honoured" and ns.M == 1:
                    continue
                assert differs, (name, mut)


@pytest.mark.parametrize("K", S.CE_EXACT_K)
@pytest.mark.parametrize("kind", ["equal", "onehot"])
def test_ce_exact_cases_are_what_they_claim(kind, K):
    ns = S.ce_exact_case(kind, K)
    loss, grad = S.ce_reference(ns.x.double(), K, ns.labels, ns.weight, S.CE_COEF, S.CE_G)
    assert abs(loss - ns.loss) < 1e-9 and torch.allclose(grad, ns.grad, rtol=1e-12, atol=1e-80)
    lab = ns.labels
    assert bool((lab == S.IGNORE).any()) and bool((lab == -1).any()) and bool((lab == K).any()) and bool((lab == 254).any())
    dead = ~((lab >= 0) & (lab < K))
    assert float(ns.grad[dead].abs().sum()) == 0.0 and (K == 1 or float(ns.grad[~dead].abs().sum()) > 0 or kind == "onehot")
    for coefs in (S.CE_COEF, S.CE_G, S.CE_COEF * S.CE_G):
        assert S.quantum_exp(torch.tensor([coefs], dtype=torch.float64)) <= 3
    assert S.quantum_exp(ns.weight.double()) <= 2


# ---- 5. masked_l1, slide_merge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.ML_ROWS, ids=S.ml_id)
def test_masked_l1_reference_equals_torch(row):
    ns = S.ml_case(row)
    for l2 in (False, True):
        pred = ns.pred.clone().requires_grad_(True)
        m = ns.m.expand_as(pred)
        loss = (F.mse_loss(pred, ns.gt, reduction="none") if l2 else F.l1_loss(pred, ns.gt, reduction="none")).mul(m).sum()
        (loss * S.ML_COEF * S.ML_G).backward()
        want_l, want_g = ns.out[l2]
        assert float(loss.detach()) == want_l and torch.equal(pred.grad, want_g)
    if ns.mask is not None:                                  # the index map, from its definition
        Hm, Wm = ns.mask.shape[-2:]
        sy, sx = torch.tensor(Hm / ns.h, dtype=F32), torch.tensor(Wm / ns.w, dtype=F32)
        my = (torch.arange(ns.h, dtype=F32) * sy).floor().long().clamp_max(Hm - 1)
        mx = (torch.arange(ns.w, dtype=F32) * sx).floor().long().clamp_max(Wm - 1)
        assert torch.equal(ns.mask[:, :, my][:, :, :, mx], ns.m)
    assert 2 * 4 * 192 * 192 > 1024 * 256


@pytest.mark.parametrize("row", S.SM_ROWS, ids=[r[0] for r in S.SM_ROWS])
def test_slide_merge_reference(row):
    name, nW, w, Wc, x1, B, h = row
    ns = S.sm_case(name, 8)
    for X in range(Wc):
        cover = [k for k in range(nW) if 0 <= X - x1[k] < w]
        assert ns.cnt[X] == len(cover)
        want = sum(ns.win[k][:, :, X - x1[k]] for k in cover) / len(cover) if cover else torch.zeros((B, h, 8)).double()
        assert torch.equal(ns.ref[:, :, X], want)
    exact = ns.cnt != 3
    N.need(ns.ref[:, :, exact], F32, "merge at counts 0, 1, 2, 4")
    tol = S.sm_tolerance(ns, F32)
    assert _inside((ns.total.float() * torch.tensor(1 / 3, dtype=F32)).double()[:, :, ~exact], ns.ref[:, :, ~exact], tol[:, :, ~exact])


def test_slide_merge_rows_cover_the_counts():
    counts = set()
    for r in S.SM_ROWS:
        counts |= set(int(c) for c in S.sm_case(r[0], 8).cnt.tolist())
    assert counts == {0, 1, 2, 3, 4} and {r[1] for r in S.SM_ROWS} == {1, 2, 3, 4}
    assert any(list(r[4]) != sorted(r[4]) for r in S.SM_ROWS)
