"""The ordered-slab weight gradient of libmadm_wslab.so on the GPU (include/madm_wslab.h), in f32 /
bf16 / f16:

1. exact on the integer lattice of tests/lattice_util.py: every row of WGRAD_CASES at the rule's slice count and at 1, 2 and 7
   forced slices, dw and dbias, into zero and into non-zero integer gradients, bit-equal to the one-slice path
   (tests/test_wslab_host.py checks the exactness conditions and the negative controls of the same inputs on the CPU);
2. the fold adds the slabs in f64 and rounds once: 2^24 + 1 + 1 is 16 777 218, not the 16 777 216 of a chain of f32 adds;
3. random data: every element within (n + 1) 2^-24 sum|t| of the float64 sum of the rounded inputs;
4. the same bits every time: twice, beside a busy stream, at other addresses, with a NaN- and a 1e30-filled workspace, and
   nothing behind workspace_bytes touched;
5. operands in strided windows between NaN canaries: bit-equal to the dense run;
6. ops.conv2d_wgrad takes the path the mode names.
"""
import ctypes

import pytest
import torch

import lattice_util as L
import wslab_util as wu
from util import to_tokens
from window_util import Guarded, guarded_flat
from test_det_gpu import _forbid

pytestmark = pytest.mark.gpu
F32, DT3, ID3 = wu.F32, wu.DT3, wu.ID3
U = 2.0 ** -24


def _lib():
    from madm_amd import _lib_wslab
    return _lib_wslab


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case(name):
    return next(c for c in wu.WGRAD_CASES if c[0] == name)


def _operands(case, dtype, xs, dy):
    """the launch's device operands of NCHW CPU tensors: ([source tokens padded to the K tile], dout tokens)"""
    d = wu.case_dims(case, dtype)
    return [to_tokens(x.float(), dtype, cp) for x, cp in zip(xs, d["C"])], to_tokens(dy.float(), dtype)


def _ops_kw(case, dtype, toks):
    d = wu.case_dims(case, dtype)
    return dict(x2=toks[1] if len(toks) > 1 else None, KH=d["KH"], KW=d["KH"], stride=d["stride"], pad_t=d["pad"], pad_l=d["pad"],
                OH=d["OH"], OW=d["OW"], upsample=d["ups"])


def _raw(d, dtype, toks, dy, dw, db, ws, ws_bytes, slices):
    """mws_conv2d_wgrad itself on the sizes ``d`` (wslab_util.case_dims), with the caller's workspace"""
    Lw = _lib()
    ptrs = dict(in1=toks[0].data_ptr(), ld1=toks[0].stride(0), dout=dy.data_ptr(), ldd=dy.stride(0), dw=dw.data_ptr(),
                dbias=None if db is None else db.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    if len(toks) > 1:
        ptrs.update(in2=toks[1].data_ptr(), ld2=toks[1].stride(0))
    a = wu.fill_args(Lw, dtype, d, slices, ptrs)
    Lw.check(Lw.lib.mws_conv2d_wgrad(ctypes.byref(a), _stream()), "mws_conv2d_wgrad")


def _unpack(dw, case, dtype):
    from madm_amd import packing
    cins, KH = case[2], case[6]
    return packing.unpack_conv_weight_grad(dw.cpu(), sum(cins), KH, KH, wu.k_tile(dtype), splits=cins).contiguous()


# ---- 1. exact on the lattice ---------------------------------------------------------------------------------------------------

EXACT = wu.exact_params()


@pytest.mark.parametrize("row", EXACT, ids=[r[0] for r in EXACT])
def test_exact_on_the_lattice(cuda, row):
    from madm_amd import ops
    cid, case, dtype, slices, eff = row
    Lw = _lib()
    d = wu.case_dims(case, dtype)
    ref = L.ref_wgrad_row(case, dtype)
    toks, dy = _operands(case, dtype, ref.xs, ref.dy)
    kw = _ops_kw(case, dtype, toks)
    a = wu.fill_args(Lw, dtype, d, slices)
    assert wu.query(Lw, a) == wu.case_geometry(case, dtype, slices) and wu.query(Lw, a)[0] == eff
    N, K = d["N"], d["K"]

    def run(dw, db, mode, slabs):
        with ops.deterministic(mode):
            ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], dw=dw, dbias=db, slabs=slabs, **kw)
        torch.cuda.synchronize()

    # slices == 0: the rule, reached through the mode; a forced count through slabs=, whatever the mode
    mode, slabs = ("slabs", None) if slices == 0 else (False, slices)
    dw, db = torch.zeros((N, K), device="cuda"), torch.zeros(N, device="cuda")
    run(dw, db, mode, slabs)
    L.assert_exact(db, ref.dbias, F32, f"{cid}: bias gradient")
    L.assert_exact(_unpack(dw, case, dtype), ref.out, F32, f"{cid}: weight gradient")
    # the gradient of the padding channels is exactly zero: nothing of dw lies outside the unpacked part
    assert float(dw.double().abs().sum()) == float(ref.out.abs().sum()), f"{cid}: padding channels are not zero"
    # into non-zero integer gradients: one update per element, the padding channels keep what they held
    dw0, db0 = wu.ints((N, K), 5, 3).float().cuda(), wu.ints((N,), 6, 3).float().cuda()
    dw1, db1 = dw0.clone(), db0.clone()
    run(dw1, db1, mode, slabs)
    L.assert_exact(db1 - db0, ref.dbias, F32, f"{cid}: bias gradient into a non-zero dbias")
    L.assert_exact(_unpack(dw1 - dw0, case, dtype), ref.out, F32, f"{cid}: weight gradient into a non-zero dw")
    assert float((dw1 - dw0).double().abs().sum()) == float(ref.out.abs().sum()), f"{cid}: padding channels after accumulation"
    # the one-slice path of the deterministic mode, same inputs: bit for bit
    dw2, db2 = dw0.clone(), db0.clone()
    run(dw2, db2, True, None)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2), f"{cid}: differs from the one-slice path"


# ---- 2. one rounding, not a chain -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("variant", ["three_slices_into_zero", "two_slices_into_one"])
def test_fold_rounds_once(cuda, dtype, variant):
    """A 1 x 1 layer (N = 4, C = 8).  Slice 0 holds 2^24 for dw[0][0] (one pixel, 4096 x 4096) and for dbias[0] (4096 pixels
    of dout = 4096: every partial sum a multiple of 4096, exact); each later slice holds 1.  Exact sums: 2^24 + 2 (three
    slices into 0) and 1 + 2^24 + 1 (two slices into 1) = 16 777 218, a float32.  A chain of f32 adds in slice order stays at
    2^24 = 16 777 216 both times (2^24 + 1 is a tie and rounds to even)."""
    Lw = _lib()
    nsl, old = (3, 0.0) if variant == "three_slices_into_zero" else (2, 1.0)
    M = nsl * 4096 - 7
    d = dict(B=1, H=M, W=1, OH=M, OW=1, pad=0, C=[8], N=4, K=8, M=M, KH=1, stride=1, ups=False)
    sl, per, ws_bytes = wu.query(Lw, wu.fill_args(Lw, dtype, d, nsl))
    first = [z * per * wu.px(dtype) for z in range(sl)]                  # the slices' first pixels, from the geometry query
    assert sl == nsl and first[1] >= 4096 and first[-1] < M
    x = torch.zeros((M, 8))
    dy = torch.zeros((M, 4))
    dy[:4096, 0] = 4096.0
    x[0, 0] = 4096.0
    for z in range(1, sl):
        x[first[z], 0] = 1.0
        dy[first[z], 0] = 1.0
    assert float((x.double()[:, 0] * dy.double()[:, 0]).sum()) + old == 16777218.0 == float(dy.double()[:, 0].sum()) + old
    chain = torch.tensor(old)
    for z in range(sl):
        last = first[z + 1] if z + 1 < sl else M
        chain = chain + (x[first[z]:last, 0].double() * dy[first[z]:last, 0].double()).sum().float()
    assert float(chain) == 16777216.0                                    # what this test tells apart from the fold
    xd, dyd = x.to(dtype).cuda(), dy.to(dtype).cuda()
    dw, db = torch.full((4, 8), old, device="cuda"), torch.full((4,), old, device="cuda")
    ws = torch.empty(ws_bytes // 4, device="cuda")
    _raw(d, dtype, [xd], dyd, dw, db, ws, ws_bytes, nsl)
    torch.cuda.synchronize()
    assert float(dw[0, 0]) == 16777218.0, f"dw[0][0] = {float(dw[0, 0])!r}"
    assert float(db[0]) == 16777218.0, f"dbias[0] = {float(db[0])!r}"
    want = torch.full((4, 8), old)
    want[0, 0] = 16777218.0
    assert torch.equal(dw.cpu(), want) and torch.equal(db.cpu(), torch.tensor([16777218.0, old, old, old]))


# ---- 3. random data, per element ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name", wu.RANDOM_ROWS)
def test_random_data_per_element(cuda, dtype, name):
    """Reference: float64 autograd of the dtype-rounded inputs.  Bound per element with n products t: (n - 1) u sum|t| for f32
    additions in any order (u = 2^-24), u sum|t| for the fold's rounding and u sum|t| for the add into the
    old value, which is chosen with |old| <= sum|t| / 2.  No element is left out; the padding channels must stay what they were."""
    from madm_amd import ops, packing
    case = _case(name)
    _n, B, cins, H, W, Cout, KH, stride, pad_mode, ups, _s = case
    d = wu.case_dims(case, dtype)
    g = torch.Generator().manual_seed(123)
    xs = [torch.randn((B, c, H, W), generator=g).to(dtype).double() for c in cins]
    dy = torch.randn((B, Cout, d["OH"], d["OW"]), generator=g).to(dtype).double()
    x = torch.cat(xs, 1)
    ref, refb = wu.wgrad_f64(x, dy, KH, stride, pad_mode, ups)
    mag, magb = wu.wgrad_f64(x.abs(), dy.abs(), KH, stride, pad_mode, ups)
    n, _ = wu.wgrad_f64(torch.ones_like(x), torch.ones_like(dy), KH, stride, pad_mode, ups)      # products per element
    assert float(n.min()) >= 1 and float(n.max()) == d["M"]
    toks, dyt = _operands(case, dtype, xs, dy)
    for slabs in (None, 7):                                              # the rule (through the mode) and a remainder slice
        sign = (torch.rand(mag.shape, generator=g, dtype=torch.float64) < 0.5).double() * 2 - 1
        old, oldb = (0.5 * mag * sign).float(), (0.5 * magb).float()
        dw = packing.pack_conv_weight(old, F32, wu.k_tile(dtype), splits=cins).cuda().contiguous()
        assert tuple(dw.shape) == (d["N"], d["K"])
        pad0 = dw.clone()
        db = oldb.cuda()
        with ops.deterministic("slabs"):
            ops.conv2d_wgrad(toks[0], dyt, B, H, W, dw=dw, dbias=db, slabs=slabs, **_ops_kw(case, dtype, toks))
        torch.cuda.synchronize()
        got = _unpack(dw, case, dtype).double()
        err, bound = (got - (old.double() + ref)).abs(), (n + 1) * U * mag
        print(f"{name} slabs={slabs}: worst dw error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} dw elements outside the bound"
        errb, boundb = (db.cpu().double() - (oldb.double() + refb)).abs(), (d["M"] + 1) * U * magb
        print(f"{name} slabs={slabs}: worst dbias error / bound {float((errb / boundb).max()):.3f}")
        assert bool((errb <= boundb).all())
        # what is not a real channel kept its bits: subtracting the unpacked change leaves the packed old values
        changed = (dw != pad0)
        repacked = packing.pack_conv_weight(torch.ones_like(old), F32, wu.k_tile(dtype), splits=cins).cuda() != 0
        assert not bool((changed & ~repacked).any()), "a padding channel's gradient changed"


# ---- 4. the same bits every time ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name,slices", [("3x3_s1_sliced", 7), ("linear_lora", 0), ("3x3_s2_vae_asym", 2)])
def test_same_bits(cuda, dtype, name, slices):
    Lw = _lib()
    case = _case(name)
    _n, B, cins, H, W, Cout, KH, stride, pad_mode, ups, _s = case
    d = wu.case_dims(case, dtype)
    g = torch.Generator().manual_seed(31)
    xs = [torch.randn((B, c, H, W), generator=g) for c in cins]
    dy = torch.randn((B, Cout, d["OH"], d["OW"]), generator=g)
    toks, dyt = _operands(case, dtype, xs, dy)
    N, K = d["N"], d["K"]
    dw0, db0 = torch.randn((N, K), generator=g).cuda(), torch.randn((N,), generator=g).cuda()
    sl, _per, n = wu.query(Lw, wu.fill_args(Lw, dtype, d, slices))
    assert sl > 1 and n % 16 == 0

    def run(toks, dyt, ws, fill=None):
        dw, db = dw0.clone(), db0.clone()
        if fill is not None:
            ws.fill_(fill)
        _raw(d, dtype, toks, dyt, dw, db, ws, n, slices)
        torch.cuda.synchronize()
        return dw, db

    gw = guarded_flat(n // 4, torch.float32, pre=1024, post=16)         # 64 bytes of canary behind workspace_bytes (and more)
    ws = gw.flat
    assert ws.data_ptr() % 16 == 0
    first = run(toks, dyt, ws)
    assert not bool(torch.isnan(first[0]).any()) and not bool(torch.isnan(first[1]).any()), "an unwritten part of the workspace was read"
    assert not bool(torch.isnan(ws).any()), "part of the workspace was never written"
    gw.check("workspace")
    again = run(toks, dyt, ws)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), "two calls differ"
    # beside a side stream kept busy with queued matmuls
    side = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device="cuda")
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a) * 1e-3
    busy = run(toks, dyt, ws)
    torch.cuda.synchronize()
    assert torch.equal(busy[0], first[0]) and torch.equal(busy[1], first[1]), "the result changed beside a busy stream"
    # a workspace that holds NaN, then 1e30, before the call: nothing of it survives into the result
    for fill in (float("nan"), 1e30):
        r = run(toks, dyt, ws, fill)
        assert not bool(torch.isnan(r[0]).any()) and torch.equal(r[0], first[0]) and torch.equal(r[1], first[1]), f"workspace pre-filled with {fill}"
    gw.check("workspace")
    # operands and workspace at other addresses (offsets inside larger buffers, the alignment rules kept)
    toks2 = [torch.cat([torch.zeros((3, t.shape[1]), dtype=dtype, device="cuda"), t])[3:] for t in toks]
    dy2 = torch.cat([torch.zeros((5, Cout), dtype=dtype, device="cuda"), dyt])[5:]
    big_ws = torch.empty(n // 4 + 4096, dtype=torch.float32, device="cuda")
    ws2 = big_ws[1028:1028 + n // 4]
    assert ws2.data_ptr() % 16 == 0 and ws2.data_ptr() != ws.data_ptr() and all(t2.data_ptr() != t.data_ptr() for t, t2 in zip(toks, toks2))
    moved = run(toks2, dy2, ws2)
    assert torch.equal(moved[0], first[0]) and torch.equal(moved[1], first[1]), "the result changed with the buffers' addresses"


# ---- 5. windows --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("name,slices", [("3x3_s1_sliced", 7), ("linear_lora", 3)])
def test_windows(cuda, dtype, name, slices):
    """x1 / x2 / dout inside larger buffers (ld > columns) of NaN canaries with 256 guard rows in front and behind, dw, dbias and
    a workspace of exactly the queried size between canaries; N = 68: the last 16-byte chunk of a 16-bit dout row covers 4
    elements of the neighbour column, which must not reach the result."""
    Lw = _lib()
    case = _case(name)
    _n, B, cins, H, W, Cout, KH, stride, pad_mode, ups, _s = case
    d = wu.case_dims(case, dtype)
    g = torch.Generator().manual_seed(47)
    xs = [torch.randn((B, c, H, W), generator=g) for c in cins]
    dy = torch.randn((B, Cout, d["OH"], d["OW"]), generator=g)
    toks, dyt = _operands(case, dtype, xs, dy)
    N, K = d["N"], d["K"]
    old_w, old_b = torch.randn((N, K), generator=g), torch.randn((N,), generator=g)
    _sl, _per, n = wu.query(Lw, wu.fill_args(Lw, dtype, d, slices))
    e = wu.epc(dtype)

    dense_w, dense_b = old_w.cuda(), old_b.cuda()
    _raw(d, dtype, toks, dyt, dense_w, dense_b, torch.empty(n // 4, device="cuda"), n, slices)
    torch.cuda.synchronize()

    guards = []
    wins = []
    for i, t in enumerate(toks):
        gd = Guarded(t.shape[0], t.shape[1], dtype, ld=t.shape[1] + 2 * e, c0=e)
        wins.append(gd.load(t))
        guards.append((f"in{i + 1}", gd))
    gd = Guarded(dyt.shape[0], Cout, dtype, ld=Cout + 8, c0=4)           # ldd: a multiple of 4 elements, dout aligned to 4 elements
    dwin = gd.load(dyt)
    guards.append(("dout", gd))
    gw, gb, gs = guarded_flat(N * K, torch.float32), guarded_flat(N, torch.float32), guarded_flat(n // 4, torch.float32)
    gw.flat.copy_(old_w.reshape(-1))
    gb.flat.copy_(old_b)
    guards += [("dw", gw), ("dbias", gb), ("workspace", gs)]
    dw, db = gw.flat.view(N, K), gb.flat
    _raw(d, dtype, wins, dwin, dw, db, gs.flat, n, slices)
    torch.cuda.synchronize()
    for what, gd in guards:
        gd.check(what)
    assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any()), "a NaN reached the result: something outside the windows was read"
    assert not bool(torch.isnan(gs.flat).any()), "part of the workspace was never written"
    assert torch.equal(dw, dense_w) and torch.equal(db, dense_b), "the windowed run differs from the dense run"


# ---- 6. the path that ran --------------------------------------------------------------------------------------------------------

def test_the_mode_names_the_path(cuda, monkeypatch):
    from madm_amd import ops
    case = _case("3x3_s1")
    dtype = torch.float16
    d = wu.case_dims(case, dtype)
    ref = L.ref_wgrad_row(case, dtype)
    toks, dy = _operands(case, dtype, ref.xs, ref.dy)
    kw = _ops_kw(case, dtype, toks)
    Lw = _lib()
    calls, real = [], Lw.lib.mws_conv2d_wgrad
    monkeypatch.setattr(Lw.lib, "mws_conv2d_wgrad", lambda *a: (calls.append(1), real(*a))[1])
    want = ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], **kw)                       # default mode: the atomics
    assert not calls and ops.wgrad_path() == "atomic"
    _forbid(monkeypatch, "madm_conv2d_wgrad")
    with ops.deterministic("slabs"):
        assert ops.wgrad_path() == "slabs" and ops.is_deterministic() is True
        got = ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], **kw)
        assert len(calls) == 1
        with ops.deterministic(True):
            assert ops.wgrad_path() == "one_slice"
            with pytest.raises(AssertionError, match="madm_conv2d_wgrad was launched"):
                ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], **kw)
            with ops.deterministic(False):
                assert ops.wgrad_path() == "atomic" and ops.is_deterministic() is False
                ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], slabs=2, **kw)          # forced, whatever the mode
                assert len(calls) == 2
            assert ops.wgrad_path() == "one_slice"
        assert ops.wgrad_path() == "slabs" and len(calls) == 2
    assert ops.wgrad_path() == "atomic" and ops.is_deterministic() is False
    torch.cuda.synchronize()
    assert torch.equal(got, want)                                                             # (lattice data: one bit pattern)
    with pytest.raises(ValueError):
        ops.conv2d_wgrad(toks[0], dy, d["B"], d["H"], d["W"], slabs=0, **kw)
