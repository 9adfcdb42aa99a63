"""The utilities of tests/optim_util.py, proved on the CPU: every exact row is exact in stepwise float32 (each
intermediate equals its float64 twin), every bound holds for the stepwise emulation and for the FMA-contracted one, every mutant
differs on the rows it applies to -- and the pure pieces of the Python layer: next_loss_scale and the span arithmetic of EmaPairs."""
import math

import pytest
import torch

import optim_util as O

# one full period of the index patterns of exact_elems (lcm(9, 257, 129) = 99 459) and a tail
N_PERIOD = 99459 + 544


def test_float32_on_the_cpu_keeps_subnormals():
    a = torch.tensor([2.0 ** -75], dtype=torch.float32) * torch.tensor([2.0 ** -70], dtype=torch.float32)
    assert float(a) == 2.0 ** -145


# ---- AdamW: the restatement is torch.optim.AdamW -----------------------------------------------------------------------------------
def test_formula_is_torch_adamw_in_float64():
    """6 steps, three groups with their own lr / weight decay, float64 parameters on the CPU.  Both sides round every operation
    to float64 and carries its own history: agreement to 64 * 2^-53 per step so far, of the magnitude of each output's terms, is
    what two orders of the same dozen operations can differ by."""
    gen = torch.Generator().manual_seed(0)
    groups = [(3e-3, 0.05), (7e-4, 0.0), (1e-4, 0.01)]
    params = [torch.randn(257, generator=gen, dtype=torch.float64) for _ in groups]
    mine = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    tp = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(tp, groups)], betas=(0.9, 0.999),
                            eps=1e-8)
    for step in range(1, 7):
        mags = []
        for k, (lr, wd) in enumerate(groups):
            g = torch.randn(257, generator=gen, dtype=torch.float64) * 10.0 ** (k - 2)
            tp[k].grad = g.clone()
            h = dict(lr=lr, wd=wd, b1=0.9, b2=0.999, eps=1e-8, bc1=1 - 0.9 ** step, bc2s=math.sqrt(1 - 0.999 ** step), gs=1.0)
            # the magnitudes of the terms of each output (|m / denom| <= 1 / (1 - b1) = 10 whatever the history)
            mags.append((mine[k][0].abs() + 10 * lr, mine[k][1].abs() + g.abs(), mine[k][2].abs() + g * g))
            mine[k] = O.adamw_formula(*((mine[k][0], g) + mine[k][1:]), O.hyper(h, torch.float64))
        opt.step()
        for k in range(len(groups)):
            st = opt.state[tp[k]]
            # both sides carry their own rounding history of the earlier steps: 64 roundings per step so far
            for a, b, mag, what in zip(mine[k], (tp[k].detach(), st["exp_avg"], st["exp_avg_sq"]), mags[k], "pmv"):
                assert bool(((a - b).abs() <= 64 * step * 2.0 ** -53 * mag).all()), f"step {step} group {k} {what}"


# ---- AdamW layer 1 -------------------------------------------------------------------------------------------------------------------
def _assert_exact(p, g, m, v, h, what):
    t32, t64 = {}, {}
    got = O.adamw_formula(p, g, m, v, O.hyper(h, torch.float32), trace=t32)
    want = O.adamw_ref(p, g, m, v, h, trace=t64)
    for k in t64:
        assert torch.equal(t32[k].double().expand_as(t64[k]), t64[k]), f"{what}: intermediate {k} is not exact in float32"
    for a, b in zip(got, want):
        assert torch.equal(a.double(), b)
    fused = O.adamw_emulate_fma(p, g, m, v, h) if all(not torch.is_tensor(x) or x.dim() == 0 for x in h.values()) else got
    for a, b in zip(fused, want):
        assert torch.equal(a.double(), b), f"{what}: the contracted form differs"
    return want


@pytest.mark.parametrize("row", ["a", "b"])
def test_exact_flat_rows_are_exact(row):
    p, g, m, v = O.exact_elems(0, N_PERIOD, row)
    assert float(p.abs().max()) == 8.0 and float((g * O.EX["gs"]).abs().max()) == 15.0 / 16
    P, M, V = _assert_exact(p, g, m, v, O.exact_hyper(row), f"row {row}")
    nz = g != 0
    gu = g.double() * O.EX["gs"]
    if row == "a":          # the closed form the issue states: m = g / 2, sqrt(v) = |g| / 2, m / denom = +-(2^k - 1) / 2^(k + 1)
        assert torch.equal(M, gu / 2) and torch.equal(V, gu * gu / 4)
        k = torch.log2(gu.abs() / O.EX["eps"] + 1)
        want_q = torch.where(nz, gu.sign() * (2.0 ** k - 1) / 2.0 ** (k + 1), torch.zeros_like(gu))
        assert torch.equal(P, p.double() * (1 - 2.0 ** -9) - 2.0 ** -5 * want_q)
    else:                   # v stays g^2
        assert torch.equal(V, gu * gu) and bool((m != 0).any())
    assert O.bias_corrections(0.5, 0.75, 1) == (0.5, 0.5) and O.bias_corrections(0.5, 0.75, 200) == (1.0, 1.0)
    assert O.bias_corrections(0.9, 0.999, 20000)[1] == 1.0 and O.bias_corrections(0.9, 0.999, 10 ** 6) == (1.0, 1.0)


APPLIES = {"eps_inside": ("a",), "bc2_plain": ("a",), "l2": ("a", "b"), "decay_after": ("a", "b"), "gscale_m_only": ("a", "b"),
           "gscale_once_in_v": ("a", "b")}


@pytest.mark.parametrize("mutant", O.ADAMW_MUTANTS)
def test_adamw_mutants_leave_the_exact_rows(mutant):
    killed = 0
    for row in ("a", "b"):
        x = O.exact_elems(0, 1027, row)
        h = O.exact_hyper(row)
        want = O.adamw_ref(*x, h)
        got = O.adamw_ref(*x, h, mutant=mutant)
        differs = any(not torch.equal(a.float(), b.float()) for a, b in zip(got, want))
        assert differs == (row in APPLIES[mutant]), f"{mutant} on row {row}"
        killed += differs
    assert killed == len(APPLIES[mutant]) >= 1


@pytest.mark.parametrize("row", ["a", "b"])
def test_exact_table_rows_are_exact(row):
    tc = O.TABLE_SMALL[row]
    assert tc.nchunks == 20 and sorted(set(tc.chunks)) == [1, 2, 5] and tc.skipped == {0, 4, tc.T - 1}
    ct = tc.chunk_tensor()
    assert ct.tolist() == [t for t, c in enumerate(tc.chunks) for _ in range(c)]
    p, g, m, v = tc.elems(0, tc.nchunks)
    h, skip = tc.hyper_rows(0, tc.nchunks)
    active = ~skip.view(-1)
    hs = dict(h, bc1=torch.where(skip, torch.ones_like(h["bc1"]), h["bc1"]))
    _assert_exact(p[active], g[active], m[active], v[active], {k: (x[active] if torch.is_tensor(x) else x) for k, x in hs.items()},
                  f"table row {row}")
    P, M, V = tc.reference(0, tc.nchunks)
    live = tc.live(0, tc.nchunks)
    assert int((~live).sum()) == tc.n - sum(tc.numel) > 0
    for x in (P, M, V):
        assert float(x[~live].abs().max()) == 0.0, "the padding tail moved"
    assert torch.equal(P[skip.view(-1)], p.double()[skip.view(-1)]) and torch.equal(M[skip.view(-1)], m.double()[skip.view(-1)])
    # NaN in a skipped tensor's gradient changes nothing
    P2, M2, V2 = tc.reference(0, tc.nchunks, nan_in_skipped=True)
    assert torch.equal(P, P2) and torch.equal(M, M2) and torch.equal(V, V2)
    assert bool(torch.isnan(tc.elems(0, tc.nchunks, nan_in_skipped=True)[1]).any())
    lrs = {(float(a), float(b)) for a, b in zip(h["lr"].view(-1)[active], h["wd"].view(-1)[active])}
    assert len(lrs) >= 4, "the tensors do not carry their own lr / wd"


@pytest.mark.parametrize("mutant", O.TABLE_MUTANTS + ("l2", "decay_after"))
def test_table_mutants_leave_the_exact_rows(mutant):
    for row in ("a", "b"):
        tc = O.TABLE_SMALL[row]
        want = tc.reference(0, tc.nchunks)
        got = tc.reference(0, tc.nchunks, mutant=mutant)
        if mutant == "skipped_moments" and row == "a":
            # row a's skipped tensors hold zero moments and their gradient is not read: nothing to see there; row b kills it
            continue
        assert any(not torch.equal(a.float(), b.float()) for a, b in zip(got, want)), f"{mutant} on row {row}"


def test_big_table_row_second_trip():
    """chunks 65 536 .. 65 538 of the 65 539-chunk row, built alone: exact, three tensors with the middle one skipped, rows that
    differ from those of chunks 0 .. 2; both coverage mutants differ there and nowhere before"""
    tc = O.TABLE_BIG
    assert tc.nchunks == O.TABLE_GRID + 3 and tc.n == 67111936
    lo, hi = O.TABLE_GRID, tc.nchunks
    assert tc.chunk_tensor(lo, hi).tolist() == [2, 3, 4] and tc.chunk_tensor(0, 3).tolist() == [0, 0, 0]
    assert tc.chunk_tensor(29999, 30001).tolist() == [0, 1]
    for t in (2, 4):
        assert tuple(tc.hyper[t][:2]) != tuple(tc.hyper[0][:2])
    assert tc.hyper[3][2] == 0.0
    for a, b in ((0, 4), (29998, 30002), (lo - 2, hi)):
        p, g, m, v = tc.elems(a, b)
        h, skip = tc.hyper_rows(a, b)
        act = ~skip.view(-1)
        _assert_exact(p[act], g[act], m[act], v[act], {k: (x[act] if torch.is_tensor(x) else x) for k, x in h.items()}, "big row")
    want = tc.reference(lo - 2, hi)
    for mutant in O.TABLE_BIG_MUTANTS:
        got = tc.reference(lo - 2, hi, mutant=mutant)
        assert all(torch.equal(a[:2], b[:2]) for a, b in zip(got, want))
        got = tc.reference(lo, hi, mutant=mutant)
        ref = tc.reference(lo, hi)
        for c in range(3):
            if c == 1 and mutant == "second_trip_untouched":
                continue        # the skipped tensor: untouched is what it should be
            assert any(not torch.equal(a[c].float(), b[c].float()) for a, b in zip(got, ref)), f"{mutant}: chunk {lo + c} unchanged"


@pytest.mark.parametrize("n", [5, 1027, O.TRIP + 3075])
def test_coverage_mutants_of_the_flat_rows(n):
    x = O.exact_elems(0, n, "b")
    want = O.adamw_ref(*x, O.exact_hyper("b"))
    starts = [n // 4 * 4] + ([O.TRIP] if n > O.TRIP else [])
    for start in starts:
        for out, orig in zip(want, (x[0], x[2], x[3])):
            if out is want[2]:
                continue        # v stays g^2 in row b by construction: p and m carry the coverage
            assert not torch.equal(O.untouched_from(out, orig, start), out), f"start {start}"


# ---- AdamW layer 2 -------------------------------------------------------------------------------------------------------------------
L2_HOST_ROWS = [r for r in O.L2_ROWS if r[0] == 1027] + [O.L2_ROWS[-2]]


@pytest.mark.parametrize("row", L2_HOST_ROWS, ids=[O.l2_id(r) for r in L2_HOST_ROWS])
def test_adamw_bounds_hold_for_the_emulations(row):
    x, h = O.l2_case(row)
    p, g, m, v = x
    if row[1] > 1:
        assert bool(((v > 0) & (v < 2.0 ** -126)).any()), "no subnormal v in the row"
    gu = g.double() * h["gs"]
    assert bool((gu == 0).any()) and bool(((gu != 0) & (gu.abs() < 1e-8)).any()) and float(gu.abs().max()) > 1.0
    want, tol = O.adamw_bounds(p, g, m, v, h)
    for name, got in (("stepwise", O.adamw_emulate(p, g, m, v, h)), ("fma", O.adamw_emulate_fma(p, g, m, v, h))):
        ratios = [O.worst_ratio(a, b, t) for a, b, t in zip(got, want, tol)]
        print(f"L2 host {O.l2_id(row)} {name}: worst |err| / bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}")
        assert max(ratios) <= 1.0, (name, ratios)


L2_APPLIES = {"eps_inside": lambda r: r[1] <= 1000, "bc2_plain": lambda r: r[1] <= 1000, "l2": lambda r: True,
              "gscale_m_only": lambda r: True, "gscale_once_in_v": lambda r: True}


@pytest.mark.parametrize("mutant", sorted(L2_APPLIES))
def test_adamw_mutants_exceed_the_bounds(mutant):
    """(decay_after moves p by lr wd |update|, 1e-6 .. 1.5e-4 of an update: at the small pair that is a float32 rounding of the
    update, so only layer 1 is claimed to see it)"""
    n = 0
    for row in L2_HOST_ROWS:
        x, h = O.l2_case(row)
        want, tol = O.adamw_bounds(*x, h)
        got = O.adamw_ref(*x, h, mutant=mutant)
        worst = max(O.worst_ratio(a.float(), b, t) for a, b, t in zip(got, want, tol))
        assert (worst > 1.0) == L2_APPLIES[mutant](row), f"{mutant} {O.l2_id(row)}: {worst}"
        n += worst > 1.0
    assert n >= 7


# ---- EMA -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", O.EMA_EXACT_ALPHAS)
def test_ema_exact_rows(alpha):
    e, q = O.ema_exact_data(5000)
    want = O.ema_ref(e, q, alpha)
    for fused in (False, True):
        assert torch.equal(O.ema_emulate(e, q, alpha, fused).double(), want)
    if alpha == 0.0:
        assert torch.equal(want.float().view(torch.int32), q.view(torch.int32))
    for mutant in O.EMA_MUTANTS:
        differs = not torch.equal(O.ema_ref(e, q, alpha, mutant), want)
        assert differs == (mutant == "zero_is_skip" and alpha == 0.0 or mutant == "swapped" and alpha not in (0.5,)), (mutant, alpha)


@pytest.mark.parametrize("n", [5, 1027, O.TRIP + 3075])
def test_coverage_mutants_of_the_ema_rows(n):
    e, q = O.ema_exact_data(n)
    for alpha in O.EMA_EXACT_ALPHAS:
        want = O.ema_ref(e, q, alpha)
        for start in [n // 4 * 4] + ([O.TRIP] if n > O.TRIP else []):
            assert not torch.equal(O.untouched_from(want, e, start), want), (alpha, start)


def test_ema_fixed_point_needs_the_fma():
    """teacher == student: fma(a, x, fl(b x)) rounds a x + b x + delta with |delta| <= ulp(b x) / 2, far inside x's own
    rounding interval, so x comes back bit for bit; the uncontracted sum rounds a x first and loses x in some elements"""
    x, _ = O.ema_random_data(200000)
    for alpha in (0.999, 0.99, 2.0 / 3.0):
        assert torch.equal(O.ema_emulate(x, x, alpha, fused=True).view(torch.int32), x.view(torch.int32))
    assert not torch.equal(O.ema_emulate(x, x, 0.999, fused=False), x)
    a = O.f32(0.999)
    rel = abs((1.0 - a) - (1 - 0.999)) / (1 - 0.999)
    print(f"EMA b: 1 - f32(0.999) = {1.0 - a!r}, double 1 - 0.999 = {1 - 0.999!r}, relative {rel:.3e}")
    assert 1.2e-5 < rel < 1.4e-5


@pytest.mark.parametrize("alpha", O.EMA_L2_ALPHAS)
def test_ema_bounds_and_mutants(alpha):
    e, q = O.ema_random_data(1027)
    want, tol = O.ema_bounds(e, q, alpha)
    a32 = torch.tensor(alpha, dtype=torch.float32)
    assert float(torch.ones((), dtype=torch.float32) - a32) == 1.0 - O.f32(alpha), "1 - alpha is not exact in float32"
    for fused in (False, True):
        r = O.worst_ratio(O.ema_emulate(e, q, alpha, fused), want, tol)
        print(f"EMA host alpha={alpha:.4f} fused={fused}: worst ratio {r:.3f}")
        assert r <= 1.0
    if alpha != 0.5:
        assert O.worst_ratio(O.ema_ref(e, q, alpha, "swapped").float(), want, tol) > 1.0


# ---- sum of squares ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, O.TRIP + 3075])
def test_sumsq_integer_rows(n):
    x = O.sumsq_int_data(n)
    assert float(x.abs().max()) <= 128.0
    want = int((x.long() ** 2).sum())
    assert want % 2 == 1
    assert O.sumsq_emulate(x, blocks=O.sumsq_grid(n)) == want
    if n % 4:
        assert O.sumsq_emulate(x, blocks=O.sumsq_grid(n), tail=False) != want
    if want > 2 ** 24:
        assert O.sumsq_emulate(x, blocks=O.sumsq_grid(n), final_f32=True) != want


def test_sumsq_flush_row():
    """the flush row on a launch of 2 x 64 threads with the kernel's flush interval and the row's own magnitudes: exact with the
    flush, 4 short per float4 of the late trips without it; the full-size row's closed-form sum is the same expression at 2048 x 256"""
    geo = dict(blocks=2, threads=64, flush=O.FLUSH)
    n = O.flush_row_n(**geo)
    x = O.flush_row_elems(0, n, **geo)
    want = int((x.double() ** 2).sum())
    assert want == O.flush_row_sum(**geo)
    assert O.sumsq_emulate(x, **geo) == want
    assert O.sumsq_emulate(x, blocks=2, threads=64, flush=None) == want - 4 * (2 * 64 + 1)     # (thread 0 makes a 66th trip)
    assert 30 * O.FLUSH * 2 ** 20 > 2 ** 25
    assert O.flush_row_n() == 65 * 2 ** 21 + 5 and O.flush_row_sum() < 2 ** 53
    # the first and last pieces of the full-size row follow the same pattern
    assert torch.equal(O.flush_row_elems(0, 8), torch.tensor([1024., -2048, 3072, -4096, -1024, 2048, -3072, 4096]))
    assert float(O.flush_row_elems(64 * O.TRIP - 1, 64 * O.TRIP + 1).abs().max()) == 4096.0
    assert O.flush_row_elems(64 * O.TRIP, O.flush_row_n()).abs().unique().tolist() == [1.0]


def test_sumsq_bounds():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(O.TRIP + 3075, generator=gen)
    want, tol = O.sumsq_bounds(x)
    got = O.sumsq_emulate(x)
    print(f"sumsq host random: |err| / bound {abs(got - want) / tol:.4f}")
    assert abs(got - want) <= tol
    geo = dict(blocks=2, threads=64)
    xa = O.adversarial_sumsq(64 * 2 * 64 * 4, lanes=(0, 1, 127), **geo)
    want, tol = O.sumsq_bounds(xa)
    got = O.sumsq_emulate(xa, **geo)
    assert want == 3 * (2 ** 24 + 63) and got == 3 * 2 ** 24, "the small terms were meant to be lost in the partial"
    print(f"sumsq host adversarial: |err| / bound {abs(got - want) / tol:.4f}")
    assert abs(got - want) <= tol
    assert abs(O.sumsq_emulate(xa, flush=None, **geo) - want) <= tol


# ---- fingerprint ---------------------------------------------------------------------------------------------------------------------
def test_fingerprint_restatement_and_mutants():
    from madm_amd.optim import fingerprint_host
    x = O.special_values(4099)
    assert int(torch.isnan(x).sum()) >= 3 and bool(torch.isinf(x).any())
    for base in (0, 5, 2 ** 32 - 4099):
        want = O.fingerprint_ref(x, base)
        assert want == fingerprint_host(x, base)
        k = 1027
        assert want == (O.fingerprint_ref(x[:k], base) + O.fingerprint_ref(x[k:], base + k)) % 2 ** 64
        for mutant in O.FP_MUTANTS:
            assert (O.fingerprint_ref(x, base, mutant) != want) == (mutant != "base_ignored" or base != 0), (mutant, base)
        assert O.fingerprint_ref(x, base, "index_low32") == want      # the same function on the domain the launcher admits


# ---- the loss scale ------------------------------------------------------------------------------------------------------------------
def test_next_loss_scale():
    from madm_amd.train import next_loss_scale
    kw = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    s, t = 65536.0, 0
    s, t = next_loss_scale(s, t, True, **kw)
    assert (s, t) == (65536.0, 1)
    s, t = next_loss_scale(s, t, True, **kw)
    assert (s, t) == (65536.0, 2)
    s, t = next_loss_scale(s, t, True, **kw)                # growth exactly at the interval, the tracker starts over
    assert (s, t) == (131072.0, 0)
    s, t = next_loss_scale(s, t, True, **kw)
    s, t = next_loss_scale(s, t, True, **kw)
    assert (s, t) == (131072.0, 2)
    s, t = next_loss_scale(s, t, False, **kw)               # a skip one step before growth: backoff and a reset
    assert (s, t) == (65536.0, 0)
    for k in range(1, 5):                                   # repeated backoff
        s, t = next_loss_scale(s, t, False, **kw)
        assert (s, t) == (65536.0 * 0.5 ** k, 0)
    s, t = next_loss_scale(s, t, True, **kw)
    s, t = next_loss_scale(s, t, True, **kw)
    assert (s, t) == (4096.0, 2)
    s, t = next_loss_scale(s, t, True, **kw)
    assert (s, t) == (8192.0, 0)
    # the arguments are not changed and amp = off is the caller's branch: the function has no such switch
    import inspect
    assert list(inspect.signature(next_loss_scale).parameters) == ["scale", "tracker", "stepped", "growth_factor", "backoff_factor",
                                                                   "growth_interval"]
    # torch's GradScaler makes the same moves
    assert next_loss_scale(1.0, 1999, True, 2.0, 0.5, 2000) == (2.0, 0) and next_loss_scale(1.0, 1998, True, 2.0, 0.5, 2000) == (1.0, 1999)


def test_run_step_calls_next_loss_scale():
    """_run_step holds no second copy of the arithmetic: it names the function and multiplies the scale nowhere itself"""
    import inspect
    from madm_amd import train
    src = inspect.getsource(train.MadmTrainer._run_step)
    assert "next_loss_scale(" in src and "self.scale *=" not in src and "_growth_tracker +=" not in src


# ---- EmaPairs: the span arithmetic on CPU tensors -------------------------------------------------------------------------------------
def test_ema_pairs_spans_on_the_production_layout():
    tflat, opt, pairs, teachers, students = O.build_pairs()
    spans = pairs._build()
    assert len(spans) == O.expected_spans() == 8
    assert sum(s[2] for s in spans) >= 4 * sum(O.PAIR_SIZES)
    # what a span covers beyond its pairs is padding of the flat buffers (zero on both sides, and zero stays zero)
    for side, flat, tensors in ((0, tflat.flat, teachers), (1, opt.flat.flat, students)):
        extra = O.covered(spans, side, flat, tensors) & ~O.owned(flat, tensors)
        assert float(flat[extra].abs().sum()) == 0.0 and int(extra.sum()) == 3 + 2     # behind 1021 and 1022


def test_ema_pairs_never_span_a_foreign_tensor():
    """A teacher tensor that is NOT in the pair list sits between two paired ones, and is exactly as long as the student side's
    padding there (24 elements behind 2024): a span across it would decay it towards the student's zero padding."""
    from madm_amd import optim
    tt = [torch.nn.Parameter(torch.ones(n)) for n in (2024, 24, 1024)]
    ss = [torch.nn.Parameter(torch.ones(n)) for n in (2024, 1024)]
    tflat = optim.FlatParams(tt, with_grad=False, align=4)
    opt = optim.TableAdamW([(s, 1e-3, 0.0) for s in ss])
    assert tt[2].data_ptr() - (tt[0].data_ptr() + 4 * 2024) == ss[1].data_ptr() - (ss[0].data_ptr() + 4 * 2024) == 96
    spans = optim.EmaPairs([tt[0], tt[2]], ss)._build()
    mask = O.covered(spans, 0, tflat.flat, tt)
    assert not bool(mask[2024:2048].any()), "a span runs over the unpaired teacher tensor"
    assert len(spans) == 2
