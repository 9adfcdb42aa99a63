"""Exact tests of the attention kernels on selector inputs (tests/attention_exact_util.py): every softmax row is 1 on one
key or 1/2 and 1/2 on two keys of different KV tiles, everything else below 2^-40, all operands exact in bf16 / f16 / f32.
The forward output then has ONE correct bit pattern in every type (the mean of the selected V rows), and so have the
gradients up to what the unselected keys add (below 1e-9, computed per case from the host-checked off-set weight W).
tests/test_attention_exact_host.py shows what these inputs cannot miss: a key admitted behind the tail, a dropped last
key, exchanged V rows, another head's V, a leaking causal mask."""
import pytest
import torch

import attention_exact_util as X
from attention_exact_util import F32, DT3, ID3

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


def _rows(t, dtype):
    """[B, L, H, D] float64 -> [B*L, H*D] of ``dtype`` (one rounding; the values here are exact in it or in f32)."""
    return t.reshape(t.shape[0] * t.shape[1], -1).float().to(dtype)


def _fused(d, dtype):
    """q, k, v as column windows of one fused buffer, as test_attention passes them."""
    C = d.H * d.D
    q, k, v = _rows(d.q, dtype), _rows(d.k, dtype), _rows(d.v, dtype)
    if d.Lq == d.Lk:
        fused = torch.cat([q, k, v], 1).cuda()
        return fused[:, :C], fused[:, C:2 * C], fused[:, 2 * C:]
    kv = torch.cat([k, v], 1).cuda()
    return q.cuda(), kv[:, :C], kv[:, C:]


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("form", X.FORMS)
@pytest.mark.parametrize("case", X.FWD_CASES, ids=[X.case_id(c) for c in X.FWD_CASES])
def test_attention_forward_exact(cuda, case, form, dtype):
    """madm_attention_fwd returns the mean of the selected V rows bit for bit: the selected score is 0, so its exponential is
    1; l is 1 or 2 and 1 / l is exact; what earlier tiles accumulated is rescaled by alpha <= 2^-57, below half an ulp of
    |v| >= 2; the 16-bit P operands 1 and 1/2 are exact; the ones-column configuration reads l = 1 or 2 back from
    accumulator column 40."""
    from madm_amd import ops
    B, H, Lq, Lk, D = case
    d, ex = X.build(*case, form), X.exact(*case, form)
    qd, kd, vd = _fused(d, dtype)
    out = torch.full((B * Lq, H * D), SENTINEL, dtype=dtype, device="cuda")
    ops.attention(qd, kd, vd, B, H, Lq, Lk, D, 1.0, out=out)
    got, want = out.cpu(), _rows(ex.o, dtype)
    bad = got != want
    print(f"fwd {X.case_id(case)} {form} {dtype}: {int(bad.sum())} of {bad.numel()} elements differ, "
          f"max |diff| {float((got.double() - want.double()).abs().max()):.3e}")
    assert torch.equal(got, want)


MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}


def _ulps(got, want, dtype):
    """|got - want| in units of the spacing of ``dtype`` at |want| (reporting only)."""
    w = want.double().abs().clamp_min(2.0 ** -14)
    return (got.double() - want.double()).abs() / torch.exp2(torch.floor(torch.log2(w)) - MANT[dtype])


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", X.BWD_CASES, ids=[X.case_id(c) for c in X.BWD_CASES])
def test_attention_backward_exact(cuda, case, dtype):
    """madm_attention_bwd on the pair form, given the exact O: dQ, dK, dV equal the exact gradients rounded once to the
    type (round to nearest even; |dk| reaches 1e4, so the 16-bit rounding is real), element by element, to within
    floor = W Lk max|dP - D| max(|q|, |k|) < 1e-9 -- what the unselected keys contribute (true zeros come back as
    about 1e-20).  No allowance is taken: the recomputed LSE is exactly 0 or 1 (log2 of 1 or 2) and P exactly 1 or 1/2 in all
    three types, and the kernel's 16-bit stores round to nearest even."""
    from madm_amd import ops
    B, H, Lq, Lk, D = case
    d, ex = X.build(*case, "pair"), X.exact(*case, "pair")
    W = X.off_set_weight(d, X.softmax_reference(d).p)
    floor = X.backward_floor(d, W)
    assert W < X.W_MAX and floor < 1e-9
    qd, kd, vd = _fused(d, dtype)
    od, dod = _rows(ex.o, dtype).cuda(), _rows(d.dout, dtype).cuda()
    dq, dk, dv = ops.attention_backward(qd, kd, vd, od, dod, B, H, Lq, Lk, D, 1.0)
    torch.cuda.synchronize()
    worst = {}
    for name, got, want in (("dq", dq, ex.dq), ("dk", dk, ex.dk), ("dv", dv, ex.dv)):
        want = _rows(want, dtype)
        got = got.cpu()
        diff = (got.double() - want.double()).abs()
        worst[name] = (float(diff.max()), int((diff > floor).sum()), float(_ulps(got, want, dtype).max()))
        print(f"bwd {X.case_id(case)} {dtype} {name}: max |diff| {worst[name][0]:.3e}, {worst[name][1]} of {diff.numel()} "
              f"above floor {floor:.2e}, max {worst[name][2]:.2f} ulp, max |want| {float(want.double().abs().max()):.0f}")
    for name, (mx, n, _) in worst.items():
        assert mx <= floor, f"{name}: {n} elements differ by up to {mx:.3e} (floor {floor:.2e})"


@pytest.mark.parametrize("form", X.FORMS)
@pytest.mark.parametrize("L", X.CAUSAL_L)
def test_causal_attention_exact(cuda, L, form):
    """madm_causal_attention_fwd (f32, D = 64, H = 12): selected keys a_i, b_i <= i, and for every query with a later key a
    bait j > i scoring exactly +40 (key i + 1 where the test can place it there) that takes the whole row if the mask
    leaks.  The output is the mean of the selected V rows bit for bit."""
    from madm_amd import ops
    d = X.build_causal(L, form)
    ex = X.closed_form(d)
    B, H, D = d.B, d.H, d.D
    C = H * D
    buf = torch.cat([torch.zeros((B * L, 4)), _rows(d.q, F32), _rows(d.k, F32), _rows(d.v, F32)], 1).cuda()
    out = torch.full((B * L, C), SENTINEL, dtype=F32, device="cuda")
    ops.causal_attention(buf[:, 4:4 + C], buf[:, 4 + C:4 + 2 * C], buf[:, 4 + 2 * C:4 + 3 * C], B, H, L, D, 1.0, out=out)
    got, want = out.cpu(), _rows(ex.o, F32)
    print(f"causal L{L} {form}: {int((got != want).sum())} of {want.numel()} elements differ")
    assert torch.equal(got, want)
