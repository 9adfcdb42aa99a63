"""Exact and per-element tests of the flat optimizer kernels (madm_sumsq_f32, madm_adamw_step, madm_adamw_step_table,
madm_ema_update, madm_snapshot_f32) and of the Python layer that drives them (TableAdamW.step, EmaPairs); data, references, bounds
and mutants: tests/optim_util.py, proved on the host by test_optim_exact_host.py.

Layer 1 asserts torch.equal for p, m and v on data whose every float32 intermediate is representable -- at every size at which a
flat kernel takes another path (below and around one float4, a partial block and a tail, exactly one trip of the 2048-block
grid, a partial second trip, three trips) and for the table kernel at 65 536 + 3 chunks, the second trip of its chunk loop.
Layer 2 asserts a counted tolerance per element against float64, nothing excluded, and prints the worst ratio of each output."""
import numpy as np
import pytest
import torch

import optim_util as O

pytestmark = pytest.mark.gpu


def _lib():
    from madm_amd._lib import lib, check
    from madm_amd.ops import _stream
    return lib, check, _stream


def _adamw(p, g, m, v, h, step):
    lib, check, stream = _lib()
    check(lib.madm_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), h["lr"], h["b1"], h["b2"], h["eps"],
                              h["wd"], step, h["gs"], stream()), "madm_adamw_step")
    torch.cuda.synchronize()


def _adamw_table(p, g, m, v, ct, hy, h):
    lib, check, stream = _lib()
    check(lib.madm_adamw_step_table(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), ct.data_ptr(), hy.data_ptr(),
                                    h["b1"], h["b2"], h["eps"], h["gs"], stream()), "madm_adamw_step_table")
    torch.cuda.synchronize()


def _ema(e, q, alpha):
    from madm_amd import optim
    optim.ema_update(e, q, alpha)
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- layer 1: AdamW ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.FLAT_SIZES)
@pytest.mark.parametrize("row", ["a", "b"])
def test_adamw_flat_exact(cuda, row, n):
    """row a: step 1 from zero moments; row b: step 200, where 1 - 0.5^200 and 1 - 0.75^200 are 1 in double"""
    x = O.exact_elems(0, n, row)
    h = O.exact_hyper(row)
    want = O.adamw_ref(*x, h)
    p, g, m, v = (t.cuda() for t in x)
    _adamw(p, g, m, v, h, 1 if row == "a" else 200)
    for got, w, name in zip((p, m, v), want, "pmv"):
        assert torch.equal(got.cpu(), w.float()), f"{name} differs at n = {n}"
    assert torch.equal(g.cpu(), x[1]), "the gradient was written"


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan_in_skipped"])
@pytest.mark.parametrize("row", ["a", "b"])
def test_adamw_table_exact(cuda, row, nan):
    """tensors of 1, 2 and 5 chunks with their own lr / wd; a skipped tensor first, in the middle and last keeps its bits, also
    with NaN in its gradient; every padding tail stays exactly 0"""
    tc = O.TABLE_SMALL[row]
    x = tc.elems(0, tc.nchunks, nan_in_skipped=nan)
    want = tc.reference(0, tc.nchunks, nan_in_skipped=nan)
    p, g, m, v = (t.reshape(-1).cuda() for t in x)
    _adamw_table(p, g, m, v, tc.chunk_tensor().cuda(), torch.from_numpy(tc.hyper).cuda(), O.exact_hyper(row))
    _, skip = tc.hyper_rows(0, tc.nchunks)
    skip, live = skip.view(-1), tc.live(0, tc.nchunks)
    for got, w, old, name in zip((p, m, v), want, (x[0], x[2], x[3]), "pmv"):
        got = got.cpu().view(-1, O.CHUNK)
        assert torch.equal(got, w.float()), f"{name} differs"
        assert torch.equal(_bits(got[skip]), _bits(old[skip])), f"{name} of a skipped tensor changed its bits"
        assert int((_bits(got)[~live] != 0).sum()) == 0, f"{name}: a padding tail is no longer +0"


def test_adamw_table_exact_second_trip(cuda):
    """65 536 + 3 chunks (67.1 M elements): chunks 65 536 .. 65 538 are the second trip of the chunk loop; they are three tensors,
    the middle one skipped with NaN in its gradient, and chunk c - 65 536 belongs to a tensor with another hyper row.  Data and
    float64 reference are made on the device in pieces; one flag comes back."""
    tc = O.TABLE_BIG
    piece = 4096
    bufs = [torch.empty(tc.n, dtype=torch.float32, device="cuda") for _ in range(4)]
    for lo in range(0, tc.nchunks, piece):
        hi = min(tc.nchunks, lo + piece)
        for b, x in zip(bufs, tc.elems(lo, hi, "cuda", nan_in_skipped=True)):
            b[lo * O.CHUNK:hi * O.CHUNK] = x.reshape(-1)
    p, g, m, v = bufs
    _adamw_table(p, g, m, v, tc.chunk_tensor(device="cuda"), torch.from_numpy(tc.hyper).cuda(), O.exact_hyper("b"))
    bad = torch.zeros(3, dtype=torch.int64, device="cuda")
    moved = torch.zeros((), dtype=torch.int64, device="cuda")
    for lo in range(0, tc.nchunks, piece):
        hi = min(tc.nchunks, lo + piece)
        want = tc.reference(lo, hi, "cuda", nan_in_skipped=True)
        for k, (b, w) in enumerate(zip((p, m, v), want)):
            got = b[lo * O.CHUNK:hi * O.CHUNK].view(-1, O.CHUNK)
            bad[k] += (got.double() != w).sum()             # (a NaN anywhere counts: NaN != w)
        moved += (p[lo * O.CHUNK:hi * O.CHUNK].view(-1, O.CHUNK).double() != tc.elems(lo, hi, "cuda")[0].double()).sum()
    bad, moved = bad.tolist(), int(moved)
    assert bad == [0, 0, 0], f"elements that differ from the float64 reference rounded once (p, m, v): {bad}"
    assert moved > tc.n // 2, "the comparison compared nothing"


# ---- layer 2: AdamW ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", O.L2_ROWS, ids=[O.l2_id(r) for r in O.L2_ROWS])
def test_adamw_flat_bounds(cuda, row):
    x, h = O.l2_case(row)
    want, tol = O.adamw_bounds(*x, h)
    p, g, m, v = (t.clone().cuda() for t in x)
    _adamw(p, g, m, v, h, row[1])
    ratios = [O.worst_ratio(got.cpu(), w, t) for got, w, t in zip((p, m, v), want, tol)]
    print(f"L2 adamw_step {O.l2_id(row)}: worst |err| / bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}")
    assert max(ratios) <= 1.0, ratios


def test_adamw_table_bounds(cuda):
    """three tensors of two chunks at steps 2, 1000 and 10^6 with the two lr / wd pairs, the data of a layer-2 row"""
    (p, g, m, v), h = O.l2_case((6 * O.CHUNK, 10, 65536.0, 0))
    steps, which = (2, 1000, 10 ** 6), (0, 1, 0)
    rows = [(O.f32(O.L2_LRWD[w][0]), O.f32(O.L2_LRWD[w][1])) + O.bias_corrections(0.9, 0.999, s) for s, w in zip(steps, which)]
    hy = torch.tensor(rows, dtype=torch.float32)
    ct = torch.tensor([0, 0, 1, 1, 2, 2], dtype=torch.int32)
    col = hy.double()[ct.long()]
    hh = dict(h, lr=col[:, 0:1], wd=col[:, 1:2], bc1=col[:, 2:3], bc2s=col[:, 3:4])
    want, tol = O.adamw_bounds(*(t.view(6, O.CHUNK) for t in (p, g, m, v)), hh)
    d = [t.clone().cuda() for t in (p, g, m, v)]
    _adamw_table(*d, ct.cuda(), hy.cuda(), h)
    ratios = [O.worst_ratio(got.cpu().view(6, O.CHUNK), w, t) for got, w, t in zip((d[0], d[2], d[3]), want, tol)]
    print(f"L2 adamw_step_table: worst |err| / bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}")
    assert max(ratios) <= 1.0, ratios


# ---- EMA -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.FLAT_SIZES)
@pytest.mark.parametrize("alpha", O.EMA_EXACT_ALPHAS)
def test_ema_exact(cuda, alpha, n):
    e, q = O.ema_exact_data(n)
    want = O.ema_ref(e, q, alpha)
    de, dq = e.cuda(), q.cuda()
    _ema(de, dq, alpha)
    assert torch.equal(de.cpu(), want.float()) and torch.equal(dq.cpu(), q)


@pytest.mark.parametrize("n", [1027, O.TRIP + 3075])
def test_ema_alpha_zero_copies_the_bits_and_equal_stays_equal(cuda, n):
    e, q = O.ema_random_data(n)
    de, dq = e.cuda(), q.cuda()
    _ema(de, dq, 0.0)
    assert torch.equal(_bits(de.cpu()), _bits(q)), "alpha = 0 is not the student's bit pattern"
    for alpha in (0.999, 0.99, 2.0 / 3.0):          # teacher == student now: a + b == 1 and the product a e is not rounded
        _ema(de, dq, alpha)
        assert torch.equal(_bits(de.cpu()), _bits(q)), f"a teacher equal to its student moved at alpha = {alpha}"


@pytest.mark.parametrize("n", [1027, O.TRIP + 3075])
@pytest.mark.parametrize("alpha", O.EMA_L2_ALPHAS, ids=lambda a: f"{a:.4f}")
def test_ema_bounds(cuda, alpha, n):
    e, q = O.ema_random_data(n)
    want, tol = O.ema_bounds(e, q, alpha)
    de = e.cuda()
    _ema(de, q.cuda(), alpha)
    r = O.worst_ratio(de.cpu(), want, tol)
    print(f"L2 ema_update alpha={alpha:.4f} n={n}: worst |err| / bound {r:.3f}")
    assert r <= 1.0


# ---- sum of squares ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.FLAT_SIZES)
def test_sumsq_integers_exact(cuda, n):
    """the integer sum, also added into an ``out`` that already holds an integer"""
    lib, check, stream = _lib()
    x = O.sumsq_int_data(n)
    want = int((x.long() ** 2).sum())
    dx = x.cuda()
    out = torch.tensor([0.0, 12345678.0], dtype=torch.float64, device="cuda")
    for k in range(2):
        check(lib.madm_sumsq_f32(dx.data_ptr(), n, out[k:].data_ptr(), stream()), "madm_sumsq_f32")
    assert out.tolist() == [float(want), float(want + 12345678)]


def test_sumsq_flush_row(cuda):
    """n = 65 * 2^21 + 5 (537 MB): exact only if a thread's float32 partial, 1920 * 2^20 after 64 trips, goes to float64 before
    trip 65 adds its 4.  This row names the kernel's present geometry (2048 blocks of 256, a flush every 64 trips)."""
    from madm_amd import optim
    n = O.flush_row_n()
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    ref = torch.zeros((), dtype=torch.int64, device="cuda")
    for lo in range(0, n, 1 << 23):
        hi = min(n, lo + (1 << 23))
        x[lo:hi] = O.flush_row_elems(lo, hi, "cuda")
        ref += (x[lo:hi].double() ** 2).sum().to(torch.int64)       # integers below 2^53: exact in float64
    got = optim.grad_sumsq(x).item()
    ref = int(ref)
    assert ref == O.flush_row_sum()
    assert got == float(ref), f"off by {got - ref} (without the flush: {-4 * (2 ** 19 + 1)})"


def test_sumsq_bounds(cuda):
    from madm_amd import optim
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(O.TRIP + 3075, generator=gen)
    want, tol = O.sumsq_bounds(x)
    got = optim.grad_sumsq(x.cuda()).item()
    print(f"L2 sumsq random n={x.numel()}: |err| / bound {abs(got - want) / tol:.5f}")
    assert abs(got - want) <= tol
    xa = O.adversarial_sumsq(8 * O.TRIP + 3075)
    want, tol = O.sumsq_bounds(xa)
    got = optim.grad_sumsq(xa.cuda()).item()
    print(f"L2 sumsq adversarial: want {want} got {got} |err| / bound {abs(got - want) / tol:.5f}")
    assert abs(got - want) <= tol


# ---- snapshot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.FLAT_SIZES)
def test_snapshot_bits_and_fingerprint(cuda, n):
    from madm_amd import optim
    x = O.special_values(n)
    dx = x.cuda()
    for base in (0, 7, 2 ** 32 - n):                        # the last: index_base + n == 2^32
        want = O.fingerprint_ref(x, base)
        assert want == optim.fingerprint_host(x, base)
        dst = torch.zeros_like(dx)
        fp = torch.zeros(3, dtype=torch.int64, device="cuda")
        optim.snapshot(dx, dst, fp[0:1], base)              # copy and fingerprint
        assert torch.equal(_bits(dst.cpu()), _bits(x)), "the copy changed a bit pattern"
        dst2 = torch.zeros_like(dx)
        optim.snapshot(dx, dst2, None, base)                # copy only
        assert torch.equal(_bits(dst2.cpu()), _bits(x))
        optim.snapshot(dx, None, fp[1:2], base)             # fingerprint only
        k = n // 2 + 1 if n > 1 else 1                      # two parts (an odd split: the second part starts unaligned in index)
        k = k // 4 * 4                                      # (but 16-byte aligned in memory, as the launcher requires)
        if 0 < k < n:
            optim.snapshot(dx[:k], None, fp[2:3], base)
            optim.snapshot(dx[k:], None, fp[2:3], base + k)
        else:
            optim.snapshot(dx, None, fp[2:3], base)
        got = [f & (2 ** 64 - 1) for f in fp.tolist()]
        assert got == [want] * 3, (n, base)
        assert torch.equal(_bits(dx.cpu()), _bits(x)), "the source was written"


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
B1, B2, EPS = O.f32(0.9), O.f32(0.999), O.f32(1e-8)
SIZES = (1500, 24, 1024, 3000)
LRWD = [(O.f32(1e-3), O.f32(0.05)), (O.f32(1e-4), 0.0), (O.f32(1e-3), O.f32(0.01)), (O.f32(1e-4), O.f32(0.05))]


def _make_opt(seed):
    """a TableAdamW over four raw parameters and a float64 torch.optim.AdamW with the same (float32-representable) settings"""
    from madm_amd import optim
    gen = torch.Generator().manual_seed(seed)
    init = [0.1 * torch.randn(n, generator=gen) for n in SIZES]
    params = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = optim.TableAdamW([(p, lr, wd) for p, (lr, wd) in zip(params, LRWD)], betas=(B1, B2), eps=EPS)
    rp = [torch.nn.Parameter(t.double()) for t in init]
    ropt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(rp, LRWD)], betas=(B1, B2), eps=EPS)
    return opt, params, ropt, rp, gen


def _state(opt):
    """per tensor (p, m, v) float32 CPU copies"""
    out = []
    for p, o in zip(opt.flat.params, opt.flat.offsets):
        n = p.numel()
        out.append(tuple(b[o:o + n].detach().cpu().clone() for b in (opt.flat.flat, opt.m, opt.v)))
    return out


def _check_step(before, after, grads, counts, gs, rp, ropt, what):
    """every touched tensor: p, m, v within the counted bound of the float64 formula (bias corrections from the tensor's OWN step
    count, rounded as the table rounds them) and within that plus two roundings of the update of torch's own result, whose bias
    corrections stay in double; every untouched tensor: bit-identical"""
    worst = 0.0
    for k, (b, a, g) in enumerate(zip(before, after, grads)):
        if g is None:
            for x, y in zip(b, a):
                assert torch.equal(_bits(x), _bits(y)), f"{what}: skipped tensor {k} changed"
            continue
        bc1, bc2s = O.bias_corrections(B1, B2, int(counts[k]))
        h = dict(lr=LRWD[k][0], wd=LRWD[k][1], b1=B1, b2=B2, eps=EPS, bc1=bc1, bc2s=bc2s, gs=gs)
        want, tol = O.adamw_bounds(b[0], g, b[1], b[2], h)
        tr = {}
        O.adamw_ref(b[0], g, b[1], b[2], h, trace=tr)
        r = [O.worst_ratio(x, w, t) for x, w, t in zip(a, want, tol)]
        worst = max(worst, *r)
        assert max(r) <= 1.0, f"{what}: tensor {k} ratios {r}"
        st = ropt.state[rp[k]]
        assert int(st["step"]) == int(counts[k]), f"{what}: tensor {k} step count {counts[k]} vs torch {int(st['step'])}"
        extra = O.SECOND * 2 * O.U32 * tr["U"].abs()
        for x, w, t in zip(a, (rp[k].detach(), st["exp_avg"], st["exp_avg_sq"]), (tol[0] + extra, tol[1], tol[2])):
            assert O.worst_ratio(x, w, t) <= 1.0, f"{what}: tensor {k} against torch.optim.AdamW"
    return worst


def _torch_step(ropt, rp, state, grads, gs):
    """torch's step from the device's state: parameters and moments are overwritten, torch's own step counters are kept"""
    for k, (p, m, v) in enumerate(state):
        rp[k].data.copy_(p.double())
        st = ropt.state.get(rp[k], {})
        if "exp_avg" in st:
            st["exp_avg"].copy_(m.double())
            st["exp_avg_sq"].copy_(v.double())
        rp[k].grad = None if grads[k] is None else grads[k].double() * gs
    ropt.step()


@pytest.mark.parametrize("kind", ["inf", "nan", "square_overflows"])
def test_table_adamw_skips_a_non_finite_step(cuda, kind):
    from madm_amd import optim
    opt, params, ropt, rp, gen = _make_opt(21)
    scale, clip = 128.0, 0.7
    grads = [torch.randn(n, generator=gen) * scale for n in SIZES]
    for p, g in zip(params, grads):
        p.grad.copy_(g.cuda())
    bad = {"inf": float("inf"), "nan": float("nan"), "square_overflows": 3e19}[kind]
    with np.errstate(all="ignore"):
        assert np.isfinite(np.float32(bad)) == (kind == "square_overflows") and not np.isfinite(np.float32(bad) * np.float32(bad))
    params[2].grad.view(-1)[517] = bad
    bufs = [opt.flat.flat, opt.m, opt.v]
    fp0, steps0 = optim.fingerprints(bufs), opt.steps.copy()
    norm, stepped = opt.step(clip_grad=clip, loss_scale=scale)
    torch.cuda.synchronize()
    assert stepped is False and not np.isfinite(norm)
    assert optim.fingerprints(bufs) == fp0 and opt.steps.tolist() == steps0.tolist() == [0] * 4
    # the next, finite step is step 1 of an optimizer that never saw the skipped one
    params[2].grad.copy_(grads[2].cuda())
    before = _state(opt)
    norm, stepped = opt.step(clip_grad=clip, loss_scale=scale)
    torch.cuda.synchronize()
    assert stepped is True and np.isfinite(norm)
    gs = O.f32((1.0 / scale) * min(1.0, clip / (norm + 1e-6)))
    _torch_step(ropt, rp, before, grads, gs)
    assert opt.steps.tolist() == [1] * 4
    _check_step(before, _state(opt), grads, opt.steps, gs, rp, ropt, kind)


def test_table_adamw_touched_step_counts_diverge(cuda):
    """5 steps; tensor 1 gets no gradient in step 2, tensor 2 none in steps 3 and 4: the counts end at 5, 4, 3, 5 and every step
    uses each tensor's own bias corrections, as torch.optim.AdamW does for ``grad is None``"""
    opt, params, ropt, rp, gen = _make_opt(22)
    scale = 65536.0
    skipped = {2: {1}, 3: {2}, 4: {2}}
    worst = 0.0
    for step in range(1, 6):
        opt.zero_grad()
        grads = []
        for k, (p, n) in enumerate(zip(params, SIZES)):
            if k in skipped.get(step, ()):
                grads.append(None)
                continue
            g = (torch.randn(n, generator=gen) * 10.0 ** (k - 2) * scale).float()
            p.grad.copy_(g.cuda())
            grads.append(g)
        before = _state(opt)
        norm, stepped = opt.step(clip_grad=None, loss_scale=scale, touched={id(p) for p, g in zip(params, grads) if g is not None})
        torch.cuda.synchronize()
        assert stepped
        gs = O.f32(1.0 / scale)
        _torch_step(ropt, rp, before, grads, gs)
        worst = max(worst, _check_step(before, _state(opt), grads, opt.steps, gs, rp, ropt, f"step {step}"))
    assert opt.steps.tolist() == [5, 4, 3, 5]
    print(f"L2 TableAdamW.step over 5 steps: worst |err| / bound {worst:.3f}")


def test_ema_pairs_on_the_production_layout(cuda):
    """teacher in FlatParams(align=4), students in a TableAdamW flat with the late tensors first, one student outside: the
    launches counted from the layout, exact results at alpha = 1/2, and not one bit of either flat buffer moved outside the pairs"""
    tflat, opt, pairs, teachers, students = O.build_pairs("cuda")
    t0, s0 = tflat.flat.clone(), opt.flat.flat.clone()
    told = [t.detach().clone() for t in teachers]
    sold = [s.detach().clone() for s in students]
    pairs.update(0.5)
    torch.cuda.synchronize()
    assert len(pairs._spans) == O.expected_spans() == 8
    want = t0.clone()
    for t, a, b in zip(teachers, told, sold):
        o = (t.data_ptr() - tflat.flat.data_ptr()) // 4
        want[o:o + t.numel()] = (a.double() + b.double()).mul(0.5).float()      # multiples of 1/8: exact
        assert torch.equal(t.detach(), want[o:o + t.numel()])
    assert torch.equal(_bits(tflat.flat), _bits(want)), "the teacher flat moved outside the paired tensors (or inside them, wrongly)"
    assert torch.equal(_bits(opt.flat.flat), _bits(s0)), "the student flat was written"
    assert all(torch.equal(s.detach(), b) for s, b in zip(students, sold))


def test_ema_pairs_leave_an_unpaired_teacher_tensor_alone(cuda):
    """the layout of test_ema_pairs_never_span_a_foreign_tensor (host) through the kernel"""
    from madm_amd import optim
    tt = [torch.nn.Parameter(torch.full((n,), 3.0, device="cuda")) for n in (2024, 24, 1024)]
    ss = [torch.nn.Parameter(torch.full((n,), 1.0, device="cuda")) for n in (2024, 1024)]
    tflat = optim.FlatParams(tt, with_grad=False, align=4)
    opt = optim.TableAdamW([(s, 1e-3, 0.0) for s in ss])
    optim.EmaPairs([tt[0], tt[2]], ss).update(0.5)
    torch.cuda.synchronize()
    assert tflat.flat.tolist() == [2.0] * 2024 + [3.0] * 24 + [2.0] * 1024
    assert float(opt.flat.flat.sum()) == 2024 + 1024
