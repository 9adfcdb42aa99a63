"""Host-side checks of the integer-lattice oracle (tests/lattice_util.py) that tests/test_lattice_gpu.py relies on:
every case row's reference meets the exactness conditions in every dtype, and assert_exact rejects a result that differs
from the reference by ONE product, by two swapped K indices or by one tap shifted at the border.  The perturbations are
applied to the reference computation on the CPU; no kernel is involved."""
import pytest
import torch
import torch.nn.functional as F

import lattice_util as L
from lattice_util import DT3, ID3

ROWS = L.all_reference_rows()


def test_lattice_generator():
    t = L.lattice((64, 1000), 1, 3, 0.25)
    assert t.dtype == torch.float64 and torch.equal(t, t.round())
    assert sorted(set(t.unique().tolist())) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    assert abs(float((t != 0).double().mean()) - 0.25) < 0.01
    nz = t[t != 0]
    for v in (-3, -2, -1, 1, 2, 3):       # uniform over the six values
        assert abs(float((nz == v).double().mean()) - 1 / 6) < 0.01
    assert torch.equal(t, L.lattice((64, 1000), 1, 3, 0.25)) and not torch.equal(t, L.lattice((64, 1000), 2, 3, 0.25))
    d = L.lattice((100, 100), 3, 1)
    assert float(d.abs().min()) == 1.0    # density 1: no zeros
    b = L.small_dense((100, 100), 4)
    assert sorted(b.unique().tolist()) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert L.exact_density(128) == 0.5 and abs(L.exact_density(17280) - (100 / 17280) ** 0.5) < 1e-12


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_reference_meets_the_exactness_conditions(row):
    """The builder asserts every condition of lattice_util (integers, |acc| < 2^24 in any summation order, exact mode:
    hw max^2 < 2^24 and representable outputs, rounding mode: finite and at least 1 % of the outputs rounded); here also that
    at least half of the outputs are nonzero -- of the value the ReLU is applied to for the one ReLU row, whose negative half
    the activation clears by definition."""
    name, dtype, build = row
    ref = build(dtype)
    value = getattr(ref, "pre", ref.out)
    assert L.nonzero_fraction(value) >= 0.5, L.nonzero_fraction(value)
    if hasattr(ref, "pre") and ref.pre is not ref.out:
        assert L.nonzero_fraction(ref.out) >= 0.4


def test_check_reference_rejects_what_breaks_exactness():
    ref = L.conv_reference(2, (64,), 8, 8, 64, 3, 1, "same", False)
    L.check_reference(ref, torch.bfloat16)
    import copy
    big = copy.copy(ref)
    big.out = ref.out * 8            # integers beyond bf16's 256
    with pytest.raises(AssertionError):
        L.check_reference(big, torch.bfloat16)
    L.check_reference(big, torch.float16)
    wide = copy.copy(ref)
    wide.hw = 1 << 20                # partial sums of squares would leave 2^24
    with pytest.raises(AssertionError):
        L.check_reference(wide, torch.float32)
    dull = copy.copy(ref)
    dull.exact = False               # "rounding mode" data that no rounding changes
    with pytest.raises(AssertionError):
        L.check_reference(dull, torch.float16)
    frac = copy.copy(ref)
    frac.acc = ref.acc + 0.5
    with pytest.raises(AssertionError):
        L._finish(frac, ref.kred, 1, 1)


SENS_CASES = {
    "3x3": (2, (64,), 8, 8, 64, 3, 1, "same", False),
    "1x1": (2, (128,), 8, 8, 64, 1, 1, "none", False),
}


def _epilogue(ref, acc):
    return acc + ref.bias[None, :, None, None] + ref.rowvec[:, :, None, None] + ref.res


def _tap_term(xpad, w, kh, kw, H, W):
    """The contribution of one tap: sum_c w[n, c, kh, kw] xpad[b, c, y + kh, x + kw]."""
    return F.conv2d(xpad[:, :, kh:kh + H, kw:kw + W], w[:, :, kh:kh + 1, kw:kw + 1])


def _perturbed(ref, KH, kind):
    x, w = ref.xs[0], ref.w
    B, C, H, W = x.shape
    p = ref.pad
    xpad = F.pad(x, (p, p, p, p))
    if kind == "drop_one_product":          # one (tap, channel) product of ONE output
        acc = ref.acc.clone()
        for n, c, kh, kw in w.nonzero().tolist():
            hit = xpad[:, c, kh:kh + H, kw:kw + W].nonzero()
            if hit.shape[0]:
                b, y, xx = hit[0].tolist()
                acc[b, n, y, xx] -= w[n, c, kh, kw] * xpad[b, c, y + kh, xx + kw]
                return _epilogue(ref, acc)
        raise AssertionError("no nonzero product")
    if kind == "swap_two_k_indices":        # two columns of the [N, K] weight matrix trade places
        w2 = w.clone()
        k0 = (0, 0, 0)
        k1 = (1, KH - 1, KH - 1)
        w2[:, k0[0], k0[1], k0[2]], w2[:, k1[0], k1[1], k1[2]] = w[:, k1[0], k1[1], k1[2]], w[:, k0[0], k0[1], k0[2]]
        assert not torch.equal(w2, w)
        return _epilogue(ref, F.conv2d(x, w2, None, padding=p))
    if kind == "shift_one_tap_at_the_border":
        # the outputs of the last column read one tap one pixel to the left of where it belongs (3x3: the tap that belongs on
        # the zero padding reads the map's last column instead)
        kh, kw = KH // 2, KH - 1
        good = _tap_term(xpad, w, kh, kw, H, W)
        shifted = _tap_term(F.pad(xpad, (1, 0, 0, 0)), w, kh, kw, H, W)    # every read one pixel to the left ...
        acc = ref.acc.clone()
        acc[:, :, :, W - 1] += shifted[:, :, :, W - 1] - good[:, :, :, W - 1]   # ... taken by the border column only
        return _epilogue(ref, acc)
    raise ValueError(kind)


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("kind", ["drop_one_product", "swap_two_k_indices", "shift_one_tap_at_the_border"])
@pytest.mark.parametrize("case", list(SENS_CASES), ids=list(SENS_CASES))
def test_assert_exact_rejects_a_perturbed_reference(case, kind, dtype):
    """A kernel result is emulated as the reference rounded to the dtype; the unperturbed one passes, each perturbed one
    (whose difference from the reference is checked to be real) is rejected."""
    geom = SENS_CASES[case]
    ref = L.check_reference(L.conv_reference(*geom, seed=9), dtype)
    emulate = lambda out: L.to_tokens_cpu(out.float() if dtype == torch.float32 else out.to(dtype)).contiguous()
    L.assert_exact(emulate(ref.out), ref.out, dtype, case)
    wrong = _perturbed(ref, geom[5], kind)
    assert wrong.shape == ref.out.shape and not torch.equal(wrong, ref.out)
    if kind == "drop_one_product":
        assert int((wrong != ref.out).sum()) == 1 and float((wrong - ref.out).abs().max()) == 1.0
    with pytest.raises(AssertionError, match="differ from the exact result"):
        L.assert_exact(emulate(wrong), ref.out, dtype, f"{case} {kind}")


def test_assert_exact_names_the_mismatch():
    ref = L.conv_reference(2, (64,), 8, 8, 64, 3, 1, "same", False, seed=9)
    got = L.to_tokens_cpu(ref.out.to(torch.bfloat16)).contiguous()
    got[(1 * 8 + 5) * 8 + 3, 37] += 1            # image 1, y 5, x 3, channel 37
    got[(1 * 8 + 6) * 8 + 3, 21] += 1
    with pytest.raises(AssertionError) as e:
        L.assert_exact(got, ref.out, torch.bfloat16, "named")
    msg = str(e.value)
    assert "named: 2 of 8192 outputs differ" in msg and "(image 1, y 5, x 3, channel 37)" in msg
    assert "channel % 16 in [5]" in msg and "x % 16 in [3]" in msg and "y % 16 in [5, 6]" in msg
    want = float(ref.out[1, 37, 5, 3])
    assert f"got {want + 1!r}, want {want!r}" in msg
    # one rounding, ties to even: 257 -> 256, 259 -> 260 in bf16; a result rounded any other way is rejected
    tie = torch.tensor([[257.0, 259.0, 1027.0, -257.0]], dtype=torch.float64)
    L.assert_exact(torch.tensor([[256.0, 260.0, 1024.0, -256.0]]).to(torch.bfloat16), tie, torch.bfloat16, "ties")
    with pytest.raises(AssertionError):
        L.assert_exact(torch.tensor([[258.0, 260.0, 1024.0, -256.0]]).to(torch.bfloat16), tie, torch.bfloat16, "ties")
    with pytest.raises(AssertionError):          # NaN never equals
        L.assert_exact(torch.tensor([[float("nan"), 260.0, 1024.0, -256.0]]).to(torch.bfloat16), tie, torch.bfloat16, "nan")
