"""The fixed-order reductions of libmadm_det.so on the GPU (include/madm_det.h), entry point by entry
point in f32 / bf16 / f16:

1. exact on an integer lattice: torch.equal against the float64 reference of tests/det_util.py (tests/test_det_host.py
   checks the exactness conditions and the negative controls of the same inputs on the CPU);
2. random data: the op's existing dense test, run again with the deterministic mode on and the replaced entry points of the
   main library made to raise -- the same reference and the same tolerance, nothing retyped; colsum and groupnorm_stats (no
   such test) against the float64 sum of the rounded inputs, within the worst-case bound of recursive f32 summation;
3. the same bits every time: alone, behind a side stream kept busy with queued matmuls, and with output and workspace at
   other addresses;
4. containment: outputs, strided operands and a workspace of exactly the queried size inside NaN canaries
   (tests/window_util.py), accumulation into a non-zero output with one rounding, bit-equal to the dense run;
5. ops.conv2d_wgrad under ops.deterministic(): the lattice cases of tests/test_lattice_gpu.py stay exact and two runs into a
   non-zero dw / dbias are equal.
"""
import ctypes

import pytest
import torch

import det_util as du
from window_util import Guarded, guarded_flat

pytestmark = pytest.mark.gpu
DT3, ID3 = du.DT3, du.ID3
OUT_ACC = {"colsum": 1, "groupnorm_stats": 2, "groupnorm_bwd_sums": 2, "layernorm_bwd_params": 2, "dwconv3x3_wgrad": 9}


def _lib():
    from madm_amd import _lib_det
    return _lib_det


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cases(dtype):
    """(id, builder, slices the case is meant to have) of every lattice case of one dtype"""
    e = du.epc(dtype)
    rows = []
    for fam in du.FAMILIES[:4]:
        rows += [(f"{fam}-{c[0]}", lambda fam=fam, c=c: du.row_case(fam, c[0], c[3] * e), c[4]) for c in du.ROW_CASES]
    rows += [(f"groupnorm_bwd_sums-two_source-{c[0]}", lambda c=c: du.row_case("groupnorm_bwd_sums", c[0], c[3] * e, True), c[4])
             for c in du.ROW_CASES[1:3]]
    rows += [(f"dwconv3x3_wgrad-{c[0]}", lambda c=c: du.dw_case(c[0], c[3] * e), c[6]) for c in du.DW_CASES]
    return rows


ALL = [(f"{cid}-{dn}", dt, build, slices) for dt, dn in zip(DT3, ID3) for cid, build, slices in _cases(dt)]
# a subset for the repeat / containment tests: every family, one-slice and many-slice, one and two column trips, two sources
PICK = ("one_slice_one_chunk-", "ragged3_b3-", "past_two_slices", "13x13_d6-", "20x20_d18-", "20x20_d6_two")
SOME = [r for r in ALL if any(p in r[0] for p in PICK)]


def _out_shape(ns):
    f = ns.family
    if f == "colsum":
        return (ns.B, ns.C), torch.float32
    if f == "groupnorm_stats":
        return (ns.B, ns.C, 2), torch.float64
    if f == "groupnorm_bwd_sums":
        return (ns.B, ns.Ctot, 2), torch.float64
    return (OUT_ACC[f], ns.C), torch.float32


def _expected(ns, old):
    """old (CPU) + the reference sum, as the fold updates the output: f64 outputs exactly, f32 outputs with one rounding"""
    s = du.reduce(ns)                                  # [NACC][B][C]
    f = ns.family
    if f == "colsum":
        return du.expected_f32(old, s[0])
    if f == "groupnorm_stats":
        return old + torch.stack([s[0], s[1]], -1)
    if f == "groupnorm_bwd_sums":
        out = old.clone()                              # the other channels of bsums stay as they are
        out[:, ns.c_off:ns.c_off + ns.C, :] += torch.stack([s[0], s[1]], -1)
        return out
    return du.expected_f32(old, s[:, 0, :])


def _ws_bytes(ns):
    q = _lib().lib
    f = ns.family
    if f == "layernorm_bwd_params":
        return q.mdet_layernorm_bwd_params_workspace_bytes(ns.R, ns.C)
    if f == "dwconv3x3_wgrad":
        return q.mdet_dwconv3x3_wgrad_workspace_bytes(ns.images, ns.H, ns.W, ns.C)
    return getattr(q, f"mdet_{f}_workspace_bytes")(ns.B, ns.R, ns.C)


def _operands(ns, dtype, strided=False):
    """Device operands; ``strided``: x / dy inside canary windows, with ld > C where the entry point takes a row stride"""
    f = ns.family
    e = du.epc(dtype)
    t = {"guards": []}

    def put(name, src, ld_ok):
        if not strided:
            t[name] = src.to(dtype).cuda().contiguous()
            return
        rows, cols = src.shape
        g = Guarded(rows, cols, dtype, ld=cols + 2 * e, c0=e) if ld_ok else Guarded(rows, cols, dtype)
        t[name] = g.load(src)
        t["guards"].append((name, g))

    put("x", ns.x, f == "colsum")
    if hasattr(ns, "dy"):
        put("dy", ns.dy, f in ("groupnorm_bwd_sums", "dwconv3x3_wgrad"))
    if f == "groupnorm_bwd_sums":
        t["sums1"] = ns.sums1.cuda()
        t["sums2"] = ns.sums2.cuda() if ns.sums2 is not None else None
        t["gamma"], t["beta"] = ns.gamma.float().cuda(), ns.beta.float().cuda()
    return t


def _launch(ns, dtype, t, out, ws, ws_bytes):
    L = _lib()
    q, code, s = L.lib, du.DTYPE_CODE[dtype], _stream()
    f = ns.family
    x = t["x"]
    if f == "colsum":
        rc = q.mdet_colsum(code, x.data_ptr(), x.stride(0), ns.B, ns.R, ns.C, out.data_ptr(), ws.data_ptr(), ws_bytes, s)
    elif f == "groupnorm_stats":
        rc = q.mdet_groupnorm_stats(code, x.data_ptr(), ns.B, ns.R, ns.C, out.data_ptr(), ws.data_ptr(), ws_bytes, s)
    elif f == "groupnorm_bwd_sums":
        rc = q.mdet_groupnorm_bwd_sums(code, x.data_ptr(), t["dy"].data_ptr(), t["dy"].stride(0), ns.B, ns.R, ns.C, ns.c_off,
                                       ns.Ctot, ns.G, t["sums1"].data_ptr(), ns.C1,
                                       t["sums2"].data_ptr() if t["sums2"] is not None else None, t["gamma"].data_ptr(),
                                       t["beta"].data_ptr(), 0.0, 0, out.data_ptr(), ws.data_ptr(), ws_bytes, s)
    elif f == "layernorm_bwd_params":
        rc = q.mdet_layernorm_bwd_params(code, x.data_ptr(), t["dy"].data_ptr(), ns.R, ns.C, 0.0, out[0].data_ptr(),
                                         out[1].data_ptr(), ws.data_ptr(), ws_bytes, s)
    else:
        rc = q.mdet_dwconv3x3_wgrad(code, x.data_ptr(), t["dy"].data_ptr(), t["dy"].stride(0), out.data_ptr(), ns.images, ns.H,
                                    ns.W, ns.C, ns.dil, ws.data_ptr(), ws_bytes, s)
    L.check(rc, f"mdet_{f}")


def _slices(ns):
    q = _lib().lib
    return q.mdet_dwconv3x3_wgrad_slices(ns.images, ns.H, ns.W) if ns.family == "dwconv3x3_wgrad" else q.mdet_slices(ns.B, ns.R)


def _run_dense(ns, dtype, old=None):
    shape, odt = _out_shape(ns)
    out = torch.zeros(shape, dtype=odt, device="cuda") if old is None else old.cuda()
    n = _ws_bytes(ns)
    ws = torch.full((n // 4,), float("nan"), dtype=torch.float32, device="cuda")
    _launch(ns, dtype, _operands(ns, dtype), out, ws, n)
    torch.cuda.synchronize()
    return out, ws


# ---- 1. exact on the lattice ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ALL, ids=[r[0] for r in ALL])
def test_exact_on_the_lattice(cuda, row):
    cid, dtype, build, want_slices = row
    ns = build()
    assert _slices(ns) == want_slices, "the case does not have the slice count it is meant to have"
    out, ws = _run_dense(ns, dtype)
    shape, odt = _out_shape(ns)
    want = _expected(ns, torch.zeros(shape, dtype=odt))
    got = out.cpu()
    assert not bool(torch.isnan(ws).any()), "part of the workspace was never written"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i0 = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{cid}: {bad.shape[0]} of {want.numel()} outputs differ from the exact sum; first at {i0}: "
                             f"got {float(got[i0])!r}, want {float(want[i0])!r}")


@pytest.mark.parametrize("B", [1, 3])
def test_groupnorm_bwd_params_adds_the_images_in_order(cuda, B):
    """dgamma / dbeta = old + the f64 sum over images with one rounding; exact on integers, and on values whose f32 sum
    would depend on the order (1e8, 1, -1e8: the f64 sum keeps the 1)."""
    L = _lib()
    Ctot = 40
    bs = du.ints((B, Ctot, 2), 7, 1000)
    if B == 3:
        bs[0, :, :] = 1.0e8
        bs[1, :, :] = du.ints((Ctot, 2), 8, 3)
        bs[2, :, :] = -1.0e8
    old = torch.randn((2, Ctot), generator=torch.Generator().manual_seed(9))
    g = guarded_flat(2 * Ctot, torch.float32)
    g.flat.copy_(old.reshape(-1))
    dgamma, dbeta = g.flat[:Ctot], g.flat[Ctot:]
    bsd = bs.cuda()
    L.check(L.lib.mdet_groupnorm_bwd_params(bsd.data_ptr(), B, Ctot, dgamma.data_ptr(), dbeta.data_ptr(), _stream()),
            "mdet_groupnorm_bwd_params")
    torch.cuda.synchronize()
    g.check("dgamma / dbeta")
    s = bs[0].clone()
    for b in range(1, B):
        s = s + bs[b]
    assert torch.equal(dgamma.cpu(), du.expected_f32(old[0], s[:, 1])) and torch.equal(dbeta.cpu(), du.expected_f32(old[1], s[:, 0]))


# ---- 2. random data: the existing dense tests, with the mode on ------------------------------------------------------------------

def _cases_of(fn):
    """the ``case`` list of an existing parametrised test, read from its marks"""
    return next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "case")


class _Forbidden:
    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise AssertionError(f"{self.name} was launched in deterministic mode")


def _forbid(monkeypatch, *names):
    from madm_amd import ops
    for n in names:
        monkeypatch.setattr(ops.lib, n, _Forbidden(n), raising=False)


import test_ops_gpu as _T      # noqa: E402
import test_train_gpu as _TT   # noqa: E402


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", _cases_of(_T.test_groupnorm_backward), ids=lambda c: f"{c[1]}-{c[2]}x{c[3]}-{c[4]}")
def test_groupnorm_backward_within_the_dense_tolerance(cuda, monkeypatch, dtype, case):
    from madm_amd import ops
    _forbid(monkeypatch, "madm_groupnorm_stats", "madm_groupnorm_bwd_sums")
    with ops.deterministic():
        _T.test_groupnorm_backward(cuda, dtype, case)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", _cases_of(_T.test_layernorm_backward), ids=lambda c: f"m{c[0]}-c{c[1]}")
def test_layernorm_backward_within_the_dense_tolerance(cuda, monkeypatch, dtype, case):
    from madm_amd import ops
    if dtype == torch.float32 and case[1] > 1280:
        return      # the row the dense test skips: madm_layernorm_bwd (still the dx kernel) takes no f32 row that wide
    L = _lib()
    calls, real = [], L.lib.mdet_layernorm_bwd_params
    monkeypatch.setattr(L.lib, "mdet_layernorm_bwd_params", lambda *a: (calls.append(1), real(*a))[1])
    with ops.deterministic():
        _T.test_layernorm_backward(cuda, dtype, case)
    assert len(calls) == 2      # the gradient and the accumulating second call


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_dwconv_wgrad_within_the_dense_tolerance(cuda, monkeypatch, dtype):
    from madm_amd import ops
    _forbid(monkeypatch, "madm_dwconv3x3_wgrad")
    with ops.deterministic():
        _TT.test_dropout_relu_dwconv_grad_kernels(cuda, dtype)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_batchnorm_backward_within_the_dense_tolerance(cuda, monkeypatch, dtype):
    """ops.batchnorm_backward sits on ops.groupnorm_backward: B = 1 image of all the pixels"""
    from madm_amd import ops
    _forbid(monkeypatch, "madm_groupnorm_bwd_sums")
    with ops.deterministic():
        _TT.test_batchnorm_train_is_groupnorm_over_the_batch(cuda, dtype)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("shape", [(2, 37, 5), (3, 600, 257), (1, 5000, 16)], ids=lambda s: f"b{s[0]}-hw{s[1]}-q{s[2]}")
def test_colsum_and_stats_on_random_data(cuda, monkeypatch, dtype, shape):
    """Through ops, mode on.  Reference: the float64 sum of the ROUNDED inputs.  Bound: recursive f32 summation of n terms
    in any order is off by at most (n - 1) u sum|term| (u = 2^-24; Higham, Accuracy and Stability, eq. 4.4, first order), the
    f64 fold adds nothing visible, and the f32 output of colsum is rounded once more (u |result|); the squares of
    groupnorm_stats carry one more rounding each (u |term|).  HW terms per column."""
    from madm_amd import ops
    _forbid(monkeypatch, "madm_colsum", "madm_groupnorm_stats")
    B, HW, chunks = shape
    C = chunks * du.epc(dtype)
    u = 2.0 ** -24
    x = (torch.randn((B * HW, C), generator=torch.Generator().manual_seed(HW)) * 2 + 0.5).to(dtype)
    xd = x.double().view(B, HW, C)
    wide = torch.zeros((B * HW, C + 2 * du.epc(dtype)), dtype=dtype, device="cuda")
    win = wide[:, du.epc(dtype):du.epc(dtype) + C]
    win.copy_(x)
    old = torch.randn((B, C), generator=torch.Generator().manual_seed(1))
    st = torch.zeros((B, C, 2), dtype=torch.float64, device="cuda")
    with ops.deterministic():
        got = ops.colsum(win, B, HW, out=old.cuda())
        xdev = x.cuda()
        ops.groupnorm_stats(xdev, B, HW, st)
    torch.cuda.synchronize()
    mag = xd.abs().sum(1)
    ref = old.double() + xd.sum(1)
    err = (got.cpu().double() - ref).abs()
    bound = (HW - 1) * u * mag + u * ref.abs() + 1e-30
    print(f"colsum: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    st = st.cpu()
    e1 = (st[..., 0] - xd.sum(1)).abs()
    e2 = (st[..., 1] - (xd * xd).sum(1)).abs()
    print(f"stats: worst error / bound {float((e1 / ((HW - 1) * u * mag + 1e-30)).max()):.3f} "
          f"{float((e2 / (HW * u * (xd * xd).sum(1) + 1e-30)).max()):.3f}")
    assert bool((e1 <= (HW - 1) * u * mag + 1e-30).all()) and bool((e2 <= HW * u * (xd * xd).sum(1) + 1e-30).all())


# ---- 3. the same bits every time ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", SOME, ids=[r[0] for r in SOME])
def test_same_bits_alone_beside_a_busy_stream_and_at_other_addresses(cuda, row):
    cid, dtype, build, _slices_meant = row
    ns = build()
    shape, odt = _out_shape(ns)
    g = torch.Generator().manual_seed(11)
    # random (not lattice) operands of the same shapes: sums whose f32 bits do depend on the order
    rnd = type(ns)(**vars(ns))
    rnd.x = torch.randn(tuple(ns.x.shape), generator=g, dtype=torch.float64)
    if hasattr(ns, "dy"):
        rnd.dy = torch.randn(tuple(ns.dy.shape), generator=g, dtype=torch.float64)
    old = torch.randn(shape, generator=g, dtype=torch.float64).to(odt)
    t = _operands(rnd, dtype)
    n = _ws_bytes(ns)

    def run(out, ws):
        out.copy_(old)
        _launch(rnd, dtype, t, out, ws, n)

    out1 = torch.empty(shape, dtype=odt, device="cuda")
    ws1 = torch.empty(n // 4, dtype=torch.float32, device="cuda")
    run(out1, ws1)
    torch.cuda.synchronize()
    first = out1.clone()
    assert not bool(torch.isnan(first).any())
    # behind a side stream kept busy with queued matmuls
    side = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device="cuda")
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a) * 1e-3
    run(out1, ws1)
    torch.cuda.synchronize()
    assert torch.equal(out1, first), "the result changed beside a busy stream"
    # output and workspace at other addresses (other offsets inside larger buffers; still 16-byte aligned)
    big_out = torch.empty(old.numel() + 64, dtype=odt, device="cuda")
    out2 = big_out[36:36 + old.numel()].view(shape)
    big_ws = torch.empty(n // 4 + 4096, dtype=torch.float32, device="cuda")
    ws2 = big_ws[1028:1028 + n // 4]
    assert out2.data_ptr() != out1.data_ptr() and ws2.data_ptr() != ws1.data_ptr() and ws2.data_ptr() % 16 == 0
    run(out2, ws2)
    torch.cuda.synchronize()
    assert torch.equal(out2, first), "the result changed with the buffers' addresses"


# ---- 4. containment ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", SOME, ids=[r[0] for r in SOME])
def test_containment_and_accumulation(cuda, row):
    cid, dtype, build, _slices_meant = row
    ns = build()
    shape, odt = _out_shape(ns)
    old = (du.ints(shape, 5, 50) * 0.5).to(odt)                     # non-zero, not integers
    dense, _ws = _run_dense(ns, dtype, old=old.clone())
    want = _expected(ns, old)
    assert torch.equal(dense.cpu(), want), "accumulation into a non-zero output: not old + sum with one rounding"

    n = _ws_bytes(ns)
    gw = guarded_flat(n // 4, torch.float32)                         # exactly the queried size, NaN-filled, guards around it
    go = guarded_flat(old.numel(), odt)
    go.flat.copy_(old.reshape(-1))
    out = go.flat.view(shape)
    t = _operands(ns, dtype, strided=True)
    _launch(ns, dtype, t, out, gw.flat, n)
    torch.cuda.synchronize()
    go.check("output")
    gw.check("workspace")
    for name, g in t["guards"]:
        g.check(name)
    assert not bool(torch.isnan(out).any()), "a NaN reached the output: something outside the operands was read"
    assert not bool(torch.isnan(gw.flat).any()), "part of the workspace was never written"
    assert torch.equal(out, dense), "the windowed run differs from the dense run"


# ---- 5. the weight gradient with one slice ------------------------------------------------------------------------------------------

import test_lattice_gpu as _TL      # noqa: E402
import lattice_util as _LU          # noqa: E402


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", _LU.WGRAD_CASES, ids=[c[0] for c in _LU.WGRAD_CASES])
def test_conv2d_wgrad_stays_exact(cuda, dtype, case):
    from madm_amd import ops
    with ops.deterministic():
        _TL.test_conv2d_wgrad_exact(cuda, dtype, case)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_conv2d_wgrad_twice_into_nonzero_gradients(cuda, dtype):
    """Random data, enough pixels for several slices in the default mode (B OH OW = 2 x 48 x 48), a non-zero dw and dbias."""
    from madm_amd import ops
    B, H, W, Cin, Cout = 2, 48, 48, 64, 64
    g = torch.Generator().manual_seed(21)
    x = torch.randn((B * H * W, Cin), generator=g).to(dtype).cuda()
    dy = torch.randn((B * H * W, Cout), generator=g).to(dtype).cuda()
    dw0 = torch.randn((Cout, 9 * Cin), generator=g).cuda()
    db0 = torch.randn((Cout,), generator=g).cuda()
    outs = []
    with ops.deterministic():
        for _ in range(2):
            dw, db = dw0.clone(), db0.clone()
            ops.conv2d_wgrad(x, dy, B, H, W, KH=3, KW=3, pad_t=1, pad_l=1, dw=dw, dbias=db)
            outs.append((dw, db))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], dw0) and bool(torch.isfinite(outs[0][0]).all())
