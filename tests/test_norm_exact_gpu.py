"""Exact and per-element tests of the GroupNorm / LayerNorm / row-softmax kernels of the default library and of the GroupNorm
fusions of the conv kernels (data, references and bounds: tests/norm_util.py, checked on the host by test_norm_exact_host.py).

Layer 1 asserts torch.equal on handed statistics that fold to a lattice mean and a power-of-two rstd: the first test measures
that v_rsq_f32 is exact at var + eps = 4^k, k = -4 .. 4 (with the dyadic eps of the rows and with eps = 0), which the rows --
they use k = -1, 0, 1 -- rely on; 1 / sqrtf in the LayerNorm kernels is relied on at k = -2 .. 2 and measured by its own rows.
Layer 2 asserts a tolerance per element against float64 with real statistics end to end, nothing excluded.
Layer 3 measures max |y - y64| of stats -> apply at growing mean / sigma next to F.group_norm in float32."""
import pytest
import torch

import lattice_util as L
import norm_util as N
from norm_util import F32, DT3, ID3

pytestmark = pytest.mark.gpu


def _dev(t, dtype):
    return t.to(dtype).contiguous().cuda()


def _rows(t, dtype, ld=None, fill=0.0):
    """[B, HW, C] float64 -> [B * HW, C] device tensor of dtype; ``ld``: a column window of a row-strided buffer filled with ``fill``"""
    r = t.reshape(-1, t.shape[-1])
    if ld is None:
        return _dev(r, dtype)
    buf = torch.full((r.shape[0], ld), fill, dtype=dtype, device="cuda")
    buf[:, :r.shape[1]] = r.to(dtype)
    return buf


def _equal(got, want_f64, dtype, what):
    L.assert_exact(got.contiguous(), want_f64.reshape(got.shape), dtype, what)


def _f32(t):
    return t.float().cuda()


def _sums(ns):
    return [s.contiguous().cuda() for s in ns.sums]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _apply(dtype, x, y, B, HW, c_off, Ctot, G, sums, gamma, beta, eps, act, res=None):
    from madm_amd import ops
    from madm_amd._lib import lib
    ops.check(lib.madm_groupnorm_apply(ops.dtype_code(dtype), x.data_ptr(), y.data_ptr(), y.stride(0), B, HW, x.shape[1], c_off, Ctot,
                                       G, sums[0].data_ptr(), sums[0].shape[1], sums[1].data_ptr() if len(sums) > 1 else None,
                                       gamma.data_ptr(), beta.data_ptr(), float(eps), ops._act_code(act=act), _ptr(res),
                                       res.stride(0) if res is not None else 0, ops._stream()), "madm_groupnorm_apply")


# ---- the probe -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [N.EPS_LATTICE, 0.0], ids=["dyadic_eps", "eps0"])
def test_rsq_is_exact_at_powers_of_four(cuda, eps):
    """madm_groupnorm_finalize with gamma = 1, beta = 0 returns scale = rsq(var + eps): 2^-k at var + eps = 4^k, k = -4 .. 4"""
    from madm_amd import ops
    ks = torch.tensor(N.RSQ_PROBE_K, dtype=torch.float64)
    HW, n = 4, len(ks)
    sums = torch.stack([torch.zeros(n, dtype=torch.float64), HW * (4.0 ** ks - eps)], -1).view(1, n, 2).cuda()
    scale, shift = ops.groupnorm_finalize([sums], 1, HW, n, torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), eps)
    got = scale.cpu().double().view(-1)
    bad = [int(k) for k, g, w in zip(ks, got, 2.0 ** -ks) if g != w]
    print(f"RSQ probe eps={eps}: scale {got.tolist()} inexact k {bad}")
    assert not bad, f"v_rsq_f32 is inexact at 4^k for k in {bad}: {got.tolist()}"
    assert float(shift.abs().max()) == 0.0


# ---- 1. statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", N.STATS_ROWS, ids=[r[0] for r in N.STATS_ROWS])
def test_groupnorm_stats_exact(cuda, dtype, row):
    from madm_amd import ops
    ns = N.stats_case(row[0], row[3] * N.epc(dtype))
    want = N.stats_sums(ns)
    x = _rows(ns.x, dtype)
    st = torch.zeros((ns.B, ns.C, 2), dtype=torch.float64, device="cuda")
    ops.groupnorm_stats(x, ns.B, ns.HW, st)
    _equal(st.cpu(), want, torch.float64, f"{row[0]}: chsums")
    ops.groupnorm_stats(x, ns.B, ns.HW, st)
    _equal(st.cpu(), 2 * want, torch.float64, f"{row[0]}: accumulating second call")


# ---- 2. apply, apply_cat, finalize with handed statistics ------------------------------------------------------------------------------
def _check_apply(ns, dtype, act, with_res, exact=True):
    want = N.gn_forward_case(ns, act, with_res, exact=exact)
    sums, gamma, beta = _sums(ns), _f32(ns.gamma), _f32(ns.beta)
    ldy = ns.Ctot + (16 if with_res else 0)                     # dense, or a column window of longer rows
    y = torch.zeros((ns.B * ns.HW, ldy), dtype=dtype, device="cuda")
    res = _rows(ns.res, dtype, ld=ns.Ctot + 24, fill=7.0) if with_res else None
    off = 0
    for C in ns.cins:                                           # c_off = 0, and c_off = C1 for a second source
        _apply(dtype, _rows(ns.x[..., off:off + C], dtype), y, ns.B, ns.HW, off, ns.Ctot, ns.G, sums, gamma, beta, ns.eps, act, res)
        off += C
    torch.cuda.synchronize()
    _equal(y[:, :ns.Ctot], want, dtype, f"{ns.name} {act} res={with_res}")
    assert float(y[:, ns.Ctot:].float().abs().sum()) == 0.0, "wrote behind the channel window"
    return want, sums, gamma, beta


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("row", N.GN_ROWS, ids=[r[0] for r in N.GN_ROWS])
def test_groupnorm_apply_exact(cuda, dtype, act, row):
    from madm_amd import ops
    ns = N.gn_case(row[0])
    _check_apply(ns, dtype, act, True)
    want, sums, gamma, beta = _check_apply(ns, dtype, act, False)
    xs = [_rows(t, dtype) for t in torch.split(ns.x, list(ns.cins), 2)]
    if len(xs) == 2:                                            # both sources in one launch
        y = ops.groupnorm(xs, ns.B, ns.HW, ns.G, gamma, beta, ns.eps, act=act, stats=sums)
        _equal(y, want, dtype, f"{ns.name} {act}: apply_cat")
    if act == "none":
        scale, shift = ops.groupnorm_finalize(sums, ns.B, ns.HW, ns.G, gamma, beta, ns.eps)
        sc, sh = N.finalize_reference(ns)
        _equal(scale.cpu(), sc, F32, f"{ns.name}: finalize scale")
        _equal(shift.cpu(), sh, F32, f"{ns.name}: finalize shift")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_groupnorm_apply_exact_behind_the_prefetched_chunks(cuda, dtype):
    """B = 256, HW = 130, 64 chunks per row: 8320 chunks per image on 8 strips of 1024 threads-times-four"""
    B, HW, cins, G = N.gn_row(N.BIG_ROW[0], dtype)
    ns = N.gn_case(N.BIG_ROW[0], C_big=cins[0])
    _check_apply(ns, dtype, "relu", True)


# ---- 3. backward -----------------------------------------------------------------------------------------------------------------------
def _check_backward(ns, dtype, act):
    from madm_amd import ops
    from madm_amd._lib import lib
    want = N.gn_backward_case(ns, act, True)
    plain = N.gn_backward_case(ns, act, False)
    sums, gamma, beta = _sums(ns), _f32(ns.gamma), _f32(ns.beta)
    s2 = sums[1].data_ptr() if len(sums) > 1 else None
    B, HW, Ctot, G, C1 = ns.B, ns.HW, ns.Ctot, ns.G, ns.cins[0]
    dy = _rows(ns.dy, dtype, ld=Ctot + 16, fill=5.0)
    dres = _rows(ns.dres, dtype, ld=Ctot + 24, fill=3.0)
    xs = [_rows(t, dtype) for t in torch.split(ns.x, list(ns.cins), 2)]
    code, act_code = ops.dtype_code(dtype), ops._act_code(act=act)
    bsums = torch.zeros((B, Ctot, 2), dtype=torch.float64, device="cuda")
    off = 0
    for x in xs:
        ops.check(lib.madm_groupnorm_bwd_sums(code, x.data_ptr(), dy.data_ptr(), dy.stride(0), B, HW, x.shape[1], off, Ctot, G,
                                              sums[0].data_ptr(), C1, s2, gamma.data_ptr(), beta.data_ptr(), float(ns.eps), act_code,
                                              bsums.data_ptr(), ops._stream()), "madm_groupnorm_bwd_sums")
        off += x.shape[1]
    _equal(bsums.cpu(), want.bsums, torch.float64, f"{ns.name} {act}: bsums")
    g0, b0 = N.ints((Ctot,), 41, 3), N.ints((Ctot,), 42, 3)     # non-zero buffers to accumulate into
    dgamma, dbeta = _f32(g0), _f32(b0)
    for with_dres in (True, False):
        off = 0
        for x in xs:
            dx = torch.empty_like(x)
            ops.check(lib.madm_groupnorm_bwd_apply(code, x.data_ptr(), dy.data_ptr(), dy.stride(0), dx.data_ptr(), B, HW, x.shape[1],
                                                   off, Ctot, G, sums[0].data_ptr(), C1, s2, gamma.data_ptr(), beta.data_ptr(),
                                                   float(ns.eps), act_code, bsums.data_ptr(),
                                                   dgamma.data_ptr() if with_dres else None, dbeta.data_ptr() if with_dres else None,
                                                   dres.data_ptr() if with_dres else None, dres.stride(0) if with_dres else 0,
                                                   ops._stream()), "madm_groupnorm_bwd_apply")
            w = (want if with_dres else plain).dx[..., off:off + x.shape[1]]
            _equal(dx, w, dtype, f"{ns.name} {act}: dx at channel {off}, dres={with_dres}")
            off += x.shape[1]
    _equal(dgamma.cpu(), g0 + want.dgamma, F32, f"{ns.name} {act}: dgamma")
    _equal(dbeta.cpu(), b0 + want.dbeta, F32, f"{ns.name} {act}: dbeta")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("row", N.GN_ROWS, ids=[r[0] for r in N.GN_ROWS])
def test_groupnorm_backward_exact(cuda, dtype, act, row):
    _check_backward(N.gn_case(row[0], paired=True), dtype, act)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_groupnorm_backward_exact_on_the_large_row(cuda, dtype):
    B, HW, cins, G = N.gn_row(N.BIG_ROW[0], dtype)
    _check_backward(N.gn_case(N.BIG_ROW[0], C_big=cins[0], paired=True), dtype, "relu")


# ---- 4. the fused GroupNorm input of the halo convs --------------------------------------------------------------------------------------
CONV_LAUNCHES = [(r, t) for r in N.CONV_GN_ROWS for t in r[6]]


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("launch", CONV_LAUNCHES, ids=[f"{r[0]}-tile{t}" for r, t in CONV_LAUNCHES])
def test_conv_fused_groupnorm_input_exact(cuda, dtype, act, launch):
    """conv3x3(act(GroupNorm([x | skip]))) + bias with handed statistics and non-zero beta: a zero padding applied before the
    activation changes the border outputs (the host file holds that mutant against this reference)"""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    (name, B, cins, H, W, Cout, _tiles), tile = launch
    ref = N.conv_gn_reference(name, act)
    kt = ops.k_tile(dtype)
    assert all(c % kt == 0 for c in cins)
    toks = [_rows(t, dtype) for t in torch.split(ref.x, list(cins), 2)]
    wp = packing.pack_conv_weight(ref.w.float(), dtype, kt, splits=list(cins)).cuda()
    gn = (_sums(ref), _f32(ref.gamma), _f32(ref.beta), ref.G, ref.eps, act)
    lib.madm_debug_set_conv_tile(tile)
    ops.PROFILE = []
    try:
        out = ops.conv2d(toks[0], wp, B, H, W, N=Cout, x2=toks[1] if len(toks) > 1 else None, KH=3, KW=3, pad_t=1, pad_l=1,
                         bias=_f32(ref.bias), gn=gn, splitk=1)
        torch.cuda.synchronize()
        kernel = ops.PROFILE[0][0]
    finally:
        ops.PROFILE = None
        lib.madm_debug_set_conv_tile(0)
    assert kernel.startswith(N.HALO_NAMES[tile]), f"tile {tile} was forced, {kernel} ran"
    L.assert_exact(out, ref.out, dtype, f"{name} tile {tile} {act}")


# ---- 5. LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _check_layernorm(ns, dtype):
    from madm_amd import ops
    y_want, bw = N.ln_exact(ns)
    _y, plain = N.ln_exact(ns, with_dres=False)
    x, dy, dres = _dev(ns.x, dtype), _dev(ns.dy, dtype), _dev(ns.dres, dtype)
    gamma, beta = _f32(ns.gamma), _f32(ns.beta)
    what = f"LayerNorm M {ns.M} C {ns.C}"
    _equal(ops.layernorm(x, gamma, beta, 0.0), y_want, dtype, what + ": y")
    g0, b0 = N.ints((ns.C,), 43, 3), N.ints((ns.C,), 44, 3)
    dgamma, dbeta = _f32(g0), _f32(b0)
    dx, _g, _b = ops.layernorm_backward(x, dy, gamma, 0.0, dgamma=dgamma, dbeta=dbeta, dres=dres)
    _equal(dx, bw.dx, dtype, what + ": dx + dres")
    _equal(dgamma.cpu(), g0 + bw.dgamma, F32, what + ": dgamma")
    _equal(dbeta.cpu(), b0 + bw.dbeta, F32, what + ": dbeta")
    dx2, g2, b2 = ops.layernorm_backward(x, dy, gamma, 0.0)
    _equal(dx2, plain.dx, dtype, what + ": dx")
    _equal(g2.cpu(), bw.dgamma, F32, what + ": dgamma from zero")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("M", N.LN_M)
def test_layernorm_exact(cuda, dtype, M):
    for C in N.ln_widths(dtype):
        _check_layernorm(N.ln_case(M, C), dtype)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_layernorm_exact_rows_strided_over_the_grid(cuda, dtype):
    _check_layernorm(N.ln_case(N.LN_STRIDE_ROW, 2 * N.epc(dtype)), dtype)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("tile", N.LN_FOLD_ROW[3], ids=["apanel", "reg64x64"])
def test_linear_with_folded_layernorm_exact(cuda, dtype, tile):
    """Linear(LayerNorm(x)) on rows of mean 0 and variance 1 is the plain exact linear x (W gamma)^T + (W beta + b)"""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    r = N.ln_fold_reference()
    kt = ops.k_tile(dtype)
    wp, bp, cs = packing.fold_layernorm(r.w.float(), r.b.float(), r.gamma.float(), r.beta.float(), dtype, kt)
    lib.madm_debug_set_conv_tile(tile)
    ops.PROFILE = []
    try:
        out = ops.linear(_dev(r.x, dtype), wp.cuda(), bias=bp.cuda(), ln=(cs.cuda(), N.LN_FOLD_EPS))
        torch.cuda.synchronize()
        kernel = ops.PROFILE[0][0]
    finally:
        ops.PROFILE = None
        lib.madm_debug_set_conv_tile(0)
    assert tile != 13 or kernel.startswith("igemm_apanel"), kernel
    L.assert_exact(out, r.out, dtype, f"folded LayerNorm, tile {tile}")


# ---- layer 2: per-element bounds against float64, real statistics end to end ---------------------------------------------------------------
# name, B, HW, sources: the shapes of test_groupnorm / _two_sources / _backward cut to HW <= 64 and C <= 640; 32 groups
L2_ROWS = [("c64", 2, 64, (64,)), ("c320", 2, 64, (320,)), ("ragged", 1, 63, (128,)), ("c640_hw4", 2, 4, (640,)),
           ("cat_320_320", 2, 64, (320, 320)), ("cat_64_128", 1, 15, (64, 128)), ("cat_straddle", 2, 16, (384, 256))]
L2_G, L2_EPS = 32, 1e-5


def _l2_case(row, dtype):
    name, B, HW, cins = row
    C = sum(cins)
    seed = 500 + 10 * [r[0] for r in L2_ROWS].index(name)
    x = N.quantised((B, HW, C), seed, dtype, 2.0, 0.5)
    res, dy, dres = (N.quantised((B, HW, C), seed + i, dtype) for i in (1, 2, 3))
    g = torch.Generator().manual_seed(seed + 4)
    gamma, beta = torch.randn(C, generator=g).float().double(), torch.randn(C, generator=g).float().double()
    return x, res, dy, dres, gamma, beta


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", L2_ROWS, ids=[r[0] for r in L2_ROWS])
def test_groupnorm_forward_within_the_element_bounds(cuda, dtype, row):
    """SiLU (two sources: apply_cat), and the residual added before a ReLU (two sources: one apply per source)"""
    from madm_amd import ops
    name, B, HW, cins = row
    x, res, dy, dres, gamma, beta = _l2_case(row, dtype)
    xs = [_rows(t, dtype) for t in torch.split(x, list(cins), 2)]
    mean, _v, rstd = N.real_stats(x, L2_G, L2_EPS)
    for act, r in (("silu", None), ("relu", res), ("none", None)):
        y = ops.groupnorm(xs, B, HW, L2_G, _f32(gamma), _f32(beta), L2_EPS, act=act, residual=None if r is None else _rows(r, dtype))
        ref = N.gn_forward(x, mean, rstd, gamma, beta, act, r).reshape(B * HW, -1)
        tol = N.gn_forward_bound(x, gamma, beta, L2_G, L2_EPS, act, r, dtype, n_terms=HW).reshape(B * HW, -1)
        worst = N.assert_within(y, ref, tol, f"{name} {act}")
        print(f"L2 forward {name} {act} {dtype}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("act", ["silu", "none"])
@pytest.mark.parametrize("row", L2_ROWS, ids=[r[0] for r in L2_ROWS])
def test_groupnorm_backward_within_the_element_bounds(cuda, dtype, act, row):
    from madm_amd import ops
    name, B, HW, cins = row
    x, res, dy, dres, gamma, beta = _l2_case(row, dtype)
    xs = [_rows(t, dtype) for t in torch.split(x, list(cins), 2)]
    stats = []
    for t in xs:
        st = torch.zeros((B, t.shape[1], 2), dtype=torch.float64, device="cuda")
        ops.groupnorm_stats(t, B, HW, st)
        stats.append(st)
    dxs, dg, db = ops.groupnorm_backward(xs, _rows(dy, dtype), B, HW, L2_G, _f32(gamma), _f32(beta), L2_EPS, stats, act=act,
                                         dres=_rows(dres, dtype))
    bd = N.gn_backward_bound(x, dy, gamma, beta, L2_G, L2_EPS, act, dres, dtype, n_terms=HW, n_sum=HW)
    w = [N.assert_within(torch.cat(dxs, 1), bd.out.reshape(B * HW, -1), bd.tol_dx.reshape(B * HW, -1), f"{name} {act}: dx"),
         N.assert_within(dg, bd.ref.dgamma, bd.tol_dgamma, f"{name} {act}: dgamma"),
         N.assert_within(db, bd.ref.dbeta, bd.tol_dbeta, f"{name} {act}: dbeta")]
    print(f"L2 backward {name} {act} {dtype}: worst error / bound dx {w[0]:.3f} dgamma {w[1]:.3f} dbeta {w[2]:.3f}")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_batchnorm_form_within_the_element_bounds(cuda, dtype):
    """G = C over one image of all the rows: ops.batch_stats -> batchnorm_train / batchnorm_backward"""
    from madm_amd import ops
    M, C, eps = 60, 72, 1e-5
    x, res, dy, dres, gamma, beta = _l2_case(("c64", 1, M, (C,)), dtype)
    xd = _rows(x, dtype)
    st = ops.batch_stats(xd)
    y = ops.batchnorm_train(xd, st, _f32(gamma), _f32(beta), eps, act="relu")
    mean, _v, rstd = N.real_stats(x, C, eps)
    N.assert_within(y, N.gn_forward(x, mean, rstd, gamma, beta, "relu")[0],
                    N.gn_forward_bound(x, gamma, beta, C, eps, "relu", None, dtype, n_terms=M)[0], "BatchNorm form")
    dx, dg, db = ops.batchnorm_backward(xd, st, _rows(dy, dtype), _f32(gamma), _f32(beta), eps, act="none")
    bd = N.gn_backward_bound(x, dy, gamma, beta, C, eps, "none", None, dtype, n_terms=M, n_sum=M)
    N.assert_within(dx, bd.out[0], bd.tol_dx[0], "BatchNorm form: dx")
    N.assert_within(dg, bd.ref.dgamma, bd.tol_dgamma, "BatchNorm form: dgamma")
    N.assert_within(db, bd.ref.dbeta, bd.tol_dbeta, "BatchNorm form: dbeta")


# name, B, Cin, H, W, Cout, splitk, tile: rows of POST_GN_CASES cut to HW <= 64 and C <= 640
POST_GN_ROWS = [("unet8_640", 2, 64, 8, 8, 640, 4, 3), ("ragged_map", 3, 64, 5, 7, 128, 5, 3), ("ten_channel_groups", 2, 64, 8, 8, 320, 9, 3)]


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", POST_GN_ROWS, ids=[r[0] for r in POST_GN_ROWS])
def test_splitk_groupnorm_within_the_element_bounds(cuda, dtype, row):
    """The conv runs on the integer lattice, so the values the reduction normalises are the exact integers of lattice_util's
    reference and only the norm arithmetic is measured.  The group's statistics are f32 partial sums of the V ceil(units / 1024)
    values a thread holds (V = 4 floats per unit where the group's channels allow, else 2), f64 across threads."""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    from util import to_tokens
    name, B, Cin, H, W, Cout, splitk, tile = row
    ref = L.exact_reference("conv", B, (Cin,), H, W, Cout, 3, 1, "same", False, dtype=F32, with_res=False, seed=8)
    kt = ops.k_tile(dtype)
    g = torch.Generator().manual_seed(60)
    gamma, beta = (1 + 0.2 * torch.randn(Cout, generator=g)).float().double(), (0.3 * torch.randn(Cout, generator=g)).float().double()
    wp = packing.pack_conv_weight(ref.w.float(), dtype, kt).cuda()
    lib.madm_debug_set_conv_tile(tile)
    try:
        out, applied = ops.conv2d(to_tokens(ref.xs[0], dtype), wp, B, H, W, N=Cout, KH=3, KW=3, pad_t=1, pad_l=1, bias=_f32(ref.bias),
                                  rowvec=_f32(ref.rowvec), splitk=splitk, post_gn=(_f32(gamma), _f32(beta), L2_G, L2_EPS, "silu"))
        torch.cuda.synchronize()
    finally:
        lib.madm_debug_set_conv_tile(0)
    assert applied, name
    v = ref.out.permute(0, 2, 3, 1).reshape(B, H * W, Cout)
    cpg = Cout // L2_G
    V = 4 if cpg % 4 == 0 else 2
    n_terms = V * -(-(H * W * cpg // V) // 1024)
    mean, _v, rstd = N.real_stats(v, L2_G, L2_EPS)
    want = N.gn_forward(v, mean, rstd, gamma, beta, "silu").reshape(B * H * W, Cout)
    tol = N.gn_forward_bound(v, gamma, beta, L2_G, L2_EPS, "silu", None, dtype, n_terms=n_terms).reshape(B * H * W, Cout)
    print(f"L2 split-K GroupNorm {name} {dtype}: worst error / bound {N.assert_within(out, want, tol, name):.3f}")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_layernorm_forward_within_the_element_bounds(cuda, dtype):
    from madm_amd import ops
    for M, C in ((9, 320), (5, 640), (64, 2 * N.epc(dtype))):
        x = N.quantised((M, C), 70 + M, dtype, 1.5, 0.5)
        g = torch.Generator().manual_seed(71)
        gamma, beta = torch.randn(C, generator=g).float().double(), torch.randn(C, generator=g).float().double()
        y = ops.layernorm(_dev(x, dtype), _f32(gamma), _f32(beta), 1e-5)
        N.assert_within(y, N.ln_forward(x, gamma, beta, 1e-5), N.ln_forward_bound(x, gamma, beta, 1e-5, dtype), f"LayerNorm {M} x {C}")


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("scale", [1.0, 512 ** -0.5], ids=["scale1", "scale512"])
@pytest.mark.parametrize("L_", N.SOFTMAX_L)
def test_softmax_rows_within_the_element_bounds(cuda, dtype, scale, L_):
    from madm_amd import ops
    s = N.softmax_case(L_, scale)
    p = ops.softmax_rows(s.cuda(), dtype, scale)
    ref, tol, rel = N.softmax_bound(s, scale, dtype)
    N.assert_within(p, ref, tol, f"softmax L {L_}")
    got = p.cpu().double()
    assert float((got[3] - got[3, 0]).abs().max()) == 0.0, "a row of equal logits must give equal p"
    # every p_i is within half an ulp of the output type of the f32 quotient, whose sum is 1 up to the f32 relative error
    slack = N.half_ulp(ref, dtype).sum(1) + rel.max(1).values
    assert bool(((got.sum(1) - 1).abs() <= slack).all()), (got.sum(1) - 1, slack)
    assert bool((slack <= L_ * N.half_ulp(ref.max(1).values, dtype) + 1e-4).all())


# ---- layer 3: conditioning (f32) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", N.COND_MU)
@pytest.mark.parametrize("row", N.COND_ROWS, ids=[r[0] for r in N.COND_ROWS])
def test_groupnorm_conditioning_next_to_float32_torch(cuda, row, mu):
    """stats -> apply with gamma = 1, beta = 0 on x ~ N(mu, 1): E = max |y - y64| stays within 4 x that of F.group_norm in float32"""
    from madm_amd import ops
    c = N.cond_case(row[0], mu)
    y = ops.groupnorm(c.x.reshape(-1, c.C).cuda(), c.B, c.HW, c.G, torch.ones(c.C, device="cuda"), torch.zeros(c.C, device="cuda"), 1e-5)
    e = float((y.cpu().double().view(c.B, c.HW, c.C) - c.y64).abs().max())
    print(f"COND groupnorm {row[0]} mu={mu}: E_kernel {e:.3e} E_torch32 {c.e_torch:.3e} ratio {e / c.e_torch:.2f}")
    assert e <= N.COND_FACTOR * c.e_torch, f"E_kernel {e:.3e} > 4 x E_torch32 {c.e_torch:.3e}"


@pytest.mark.parametrize("mu", N.COND_MU)
def test_layernorm_conditioning_next_to_float32_torch(cuda, mu):
    from madm_amd import ops
    c = N.cond_ln_case(mu)
    y = ops.layernorm(c.x.cuda(), torch.ones(c.C, device="cuda"), torch.zeros(c.C, device="cuda"), 1e-5)
    e = float((y.cpu().double() - c.y64).abs().max())
    print(f"COND layernorm mu={mu}: E_kernel {e:.3e} E_torch32 {c.e_torch:.3e} ratio {e / c.e_torch:.2f}")
    assert e <= N.COND_FACTOR * c.e_torch, f"E_kernel {e:.3e} > 4 x E_torch32 {c.e_torch:.3e}"
