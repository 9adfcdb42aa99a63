"""Host checks of the selector inputs (tests/attention_exact_util.py): that they have the properties the exact GPU tests
(tests/test_attention_exact_gpu.py) rely on, and -- on the float64 reference alone -- that the faults those tests are
meant to catch change an output by a quarter of its value or by at least 1, not by 1e-3."""
import pytest
import torch

import attention_exact_util as X

ALL_CASES = sorted(set(X.FWD_CASES) | set(X.BWD_CASES))

@pytest.fixture(scope="module", params=[(c, f) for c in ALL_CASES for f in X.FORMS],
                ids=[f"{X.case_id(c)}-{f}" for c in ALL_CASES for f in X.FORMS])
def case(request):
    c, form = request.param
    d = X.build(*c, form)
    ref = X.softmax_reference(d, grad=True)
    return d, X.exact(*c, form), ref


def test_inputs_are_representable_in_both_16_bit_formats(case):
    d, ex, _ = case
    for name in ("q", "k", "v", "dout"):
        for dt in (X.BF16, X.F16):
            assert X.representable(getattr(d, name), dt), f"{name} in {dt}"
    v = d.v.transpose(1, 2).reshape(-1, d.D)
    assert v.abs().min() >= 2 and v.abs().max() <= 6 and torch.equal(v % 2, torch.zeros_like(v))
    assert torch.unique(v, dim=0).shape[0] == v.shape[0], "every (b, h, key) row of V is a different vector"
    nz = (d.dout != 0).sum(-1)
    assert nz.max() <= 4 and nz.min() >= 1 and d.dout.abs().max() == 1


def test_selected_scores_are_zero_and_all_others_below_the_gap(case):
    d, ex, ref = case
    s = X.scores(d)
    sel = ex.P > 0
    assert torch.equal(s[sel], torch.zeros_like(s[sel]))
    assert s[~sel].max() <= -X.GAP_ZERO <= -X.GAP_MIN
    assert X.off_set_weight(d, ref.p) < X.W_MAX
    if d.form == "pair":
        two = d.a != d.b
        assert two.float().mean() > 0.25, "the pair form selects two keys for a good share of the queries"
        for tz in X.key_tiles(d.Lk, d.D):
            assert bool(((d.a // tz) != (d.b // tz))[two].all()), "partners lie in different KV tiles"
    else:
        assert torch.equal(d.a, d.b)


def test_boundary_selections_are_present(case):
    d, _, _ = case
    for row, key in X.forced_selections(d.Lq, d.Lk, d.D):
        assert bool((d.a[:, :, row] == key).all())
    assert bool((d.a[:, :, d.Lq - 1] == d.Lk - 1).all())
    keys = {0, d.Lk - 1}
    for tz in X.key_tiles(d.Lk, d.D):
        keys |= {(d.Lk - 1) // tz * tz, min(tz, d.Lk) - 1}
    for b in range(d.B):
        for h in range(d.H):
            assert keys <= set(d.a[b, h].tolist())


def test_float64_autograd_equals_the_closed_forms(case):
    d, ex, ref = case
    W = X.off_set_weight(d, ref.p)
    vmax, qk = float(d.v.abs().max()), max(float(d.q.abs().max()), float(d.k.abs().max()))
    dpd = float(ex.dPmD.abs().max())
    assert dpd <= 48 and float((d.dout.transpose(1, 2) @ d.v.transpose(1, 2).transpose(2, 3)).abs().max()) <= 24
    eps = 1e-12     # float64 rounding of the reference's own sums (|dk| reaches 1e4)
    assert (ref.o - ex.o).abs().max() <= 2 * W * vmax + eps
    assert (ref.dv - ex.dv).abs().max() <= W * d.Lq + eps
    floor = X.backward_floor(d, W)
    assert floor < 1e-9
    assert (ref.dq - ex.dq).abs().max() <= 4 * floor + eps * qk
    assert (ref.dk - ex.dk).abs().max() <= 4 * floor * d.Lq / d.Lk + eps * qk * d.Lq


def test_outputs_and_ds_are_exact_in_bf16_and_f32(case):
    d, ex, _ = case
    assert X.representable(ex.o, X.BF16) and X.representable(ex.o, X.F16)
    assert X.representable(ex.dS, X.BF16) and X.representable(ex.dS, X.F16)
    assert torch.equal(ex.dS * 2, (ex.dS * 2).round())
    for name in ("dq", "dk", "dv"):        # the accumulated gradients are exact in f32: ONE rounding to a 16-bit type
        assert X.representable(getattr(ex, name), X.F32)
    if d.form == "pair":
        assert float(ex.dq.abs().max()) > 0, "partners have different K rows: dQ is not trivially 0"


# ---- what the GPU test cannot miss, shown on the float64 reference ----

@pytest.fixture(scope="module", params=[(c, f) for c in X.FWD_CASES for f in X.FORMS],
                ids=[f"{X.case_id(c)}-{f}" for c in X.FWD_CASES for f in X.FORMS])
def fcase(request):
    c, form = request.param
    return X.build(*c, form), X.exact(*c, form)


def _pad_key(d, t):
    return torch.cat([t, torch.zeros((d.B, 1, d.H, d.D), dtype=torch.float64)], 1)


def test_forward_cases_hold_the_input_properties(fcase):
    """The long-query forward cases are not in ``case`` (no autograd for them): scores, gap and weight here."""
    d, ex = fcase
    s = X.scores(d)
    sel = ex.P > 0
    assert torch.equal(s[sel], torch.zeros_like(s[sel])) and s[~sel].max() <= -X.GAP_ZERO
    p = torch.softmax(s, -1)
    W = X.off_set_weight(d, p)
    assert W < X.W_MAX
    o = (p @ d.v.transpose(1, 2)).transpose(1, 2)
    assert (o - ex.o).abs().max() <= 2 * W * 6 + 1e-12
    assert X.representable(ex.o, X.BF16) and X.representable(ex.o, X.F16)
    for row, key in X.forced_selections(d.Lq, d.Lk, d.D):
        assert bool((d.a[:, :, row] == key).all())


def test_mutation_one_phantom_zero_key(fcase):
    """A tail mask off by one admits the zero row an out-of-bounds load returns (score 0): every element of every output
    row with one selected key moves by at least 25 % (it is cut to 1/2; a pair row is cut to 2/3)."""
    d, ex = fcase
    mut = X.softmax_reference(d, k=_pad_key(d, d.k), v=_pad_key(d, d.v)).o
    rel = ((mut - ex.o).abs() / ex.o.abs().clamp_min(1e-30)).transpose(1, 2)       # [B, H, Lq, D]
    single = (d.a == d.b)
    assert bool(single.any()) or d.form == "pair"      # a power-of-two Lk gives every key a partner
    if bool(single.any()):
        assert rel[single].min() >= 0.25
    nz = (ex.o != 0).transpose(1, 2)
    assert rel[nz].min() >= 0.25, "pair rows too, wherever the mean is not 0"


def test_mutation_last_key_dropped(fcase):
    d, ex = fcase
    mut = X.softmax_reference(d, k=d.k[:, :-1], v=d.v[:, :-1]).o
    assert (mut - ex.o).abs().max() >= 1


def test_mutation_adjacent_value_rows_exchanged(fcase):
    d, ex = fcase
    v = d.v.clone()
    v[:, [d.Lk - 2, d.Lk - 1]] = v[:, [d.Lk - 1, d.Lk - 2]]
    mut = X.softmax_reference(d, v=v).o
    assert (mut - ex.o).abs().max() >= 1


def test_mutation_value_rows_of_the_next_head(fcase):
    d, ex = fcase
    if d.B * d.H == 1:
        return      # the one case with a single (b, h): there is no other head to read
    # head h + 1 of the flattened (b, h) order: what a head offset that is one too large reads
    flat = d.v.transpose(1, 2).reshape(d.B * d.H, d.Lk, d.D)
    v = flat.roll(-1, 0).reshape(d.B, d.H, d.Lk, d.D).transpose(1, 2)
    mut = X.softmax_reference(d, v=v).o
    assert (mut - ex.o).abs().amax((1, 3)).min() >= 1, "in every (b, h)"


# ---- causal ----

@pytest.fixture(scope="module", params=[(L, f) for L in X.CAUSAL_L for f in X.FORMS],
                ids=[f"L{L}-{f}" for L in X.CAUSAL_L for f in X.FORMS])
def ccase(request):
    L, form = request.param
    d = X.build_causal(L, form)
    return d, X.closed_form(d)


def test_causal_inputs(ccase):
    d, ex = ccase
    L = d.Lq
    for name in ("q", "k", "v"):
        assert X.representable(getattr(d, name), X.F32)
    assert float(d.q.abs().max()) < 2 ** 20, "every partial sum of a score stays an exact f32 integer"
    assert torch.equal(d.q * 2, (d.q * 2).round()) and torch.equal(d.k, d.k.round())
    i = torch.arange(L).view(1, 1, L)
    assert bool((d.a <= i).all()) and bool((d.b <= i).all())
    s = X.scores(d)
    vis = X.causal_mask(L).expand(d.B, d.H, L, L)
    sel = ex.P > 0
    assert torch.equal(s[sel], torch.zeros_like(s[sel]))
    if bool((vis & ~sel).any()):
        assert s[vis & ~sel].max() <= -X.GAP_ZERO
    has_later = (i < L - 1).expand_as(d.bait)
    assert torch.equal(d.bait >= 0, has_later), "a bait for every query that has a later key"
    if L > 1:
        bs = torch.gather(s, 3, d.bait.clamp_min(0).unsqueeze(-1)).squeeze(-1)
        assert bool((d.bait > i)[has_later].all())
        assert torch.equal(bs[has_later], torch.full_like(bs[has_later], X.BAIT))
        assert bool((d.bait == i + 1)[has_later].float().mean() > 0.4), "key i + 1 is the bait for a good share"
    ref = X.softmax_reference(d, mask=vis)
    W = X.off_set_weight(d, ref.p)
    assert W < X.W_MAX
    assert (ref.o - ex.o).abs().max() <= 2 * W * 6 + 1e-12
    assert X.representable(ex.o, X.F32)
    if form_has_pairs(d):
        assert bool((d.a != d.b).any())


def form_has_pairs(d):
    return d.form == "pair" and d.Lq > 2


def test_causal_mutation_leaking_mask(ccase):
    """Without the mask the bait (or a later key scoring even higher) takes the row: every baited row changes by >= 1."""
    d, ex = ccase
    if d.Lq == 1:
        return
    mut = X.softmax_reference(d).o
    diff = (mut - ex.o).abs().amax(-1).transpose(1, 2)          # [B, H, L]
    assert diff[d.bait >= 0].min() >= 1
    # a mask off by one (j <= i + 1) where key i + 1 is the bait
    L = d.Lq
    off1 = torch.ones((L, L), dtype=torch.bool).tril(1).expand(d.B, d.H, L, L)
    mut1 = X.softmax_reference(d, mask=off1).o
    diff1 = (mut1 - ex.o).abs().amax(-1).transpose(1, 2)
    nxt = d.bait == torch.arange(L).view(1, 1, L) + 1
    assert diff1[nxt].min() >= 1
