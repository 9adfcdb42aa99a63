"""What the tests of the ordered-slab weight gradient share (include/madm_wslab.h, libmadm_wslab.so; DESIGN.md section 28;
host-only torch code): the tests' own restatement of the launch geometry, the argument struct of a case, float64 references
cut into the pixel slices the kernel uses (and the mutants a comparison must reject), and the library's exports."""
import ctypes
import functools
import os

import torch

import lattice_util as L
import sidelib_util as su

ROOT = su.ROOT
F32, BF16, F16 = L.F32, L.BF16, L.F16
DT3, ID3 = L.DT3, L.ID3
DTYPE_CODE = {F32: 0, BF16: 1, F16: 2}
WGRAD_CASES = L.WGRAD_CASES
FORCED = (0, 1, 2, 7)                 # slice counts the GPU tests ask for: 0 = the rule
RANDOM_ROWS = ("3x3_s1_sliced", "3x3_s2_vae_asym", "3x3_concat", "linear_lora")
TARGET_BLOCKS, MAX_SLICES = 640, 65535


def epc(dtype):
    return 4 if dtype == F32 else 8


def px(dtype):
    """pixels of one reduction step: the k extent of one MFMA"""
    return 4 * epc(dtype)


def k_tile(dtype):
    return 32 if dtype == F32 else 64


def round_up(n, m):
    return (n + m - 1) // m * m


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------

def rule_slices(total_steps, tiles):
    """The slice count for `slices = 0` (wslab.hip: rule_slices): one round of TARGET_BLOCKS blocks, at least two steps per
    slice; for reductions of at most 512 steps the minimum of rounds * steps per slice * 1 us + tiles * 16384 * slices * 2.7 ps."""
    sl = max(1, min((TARGET_BLOCKS + tiles // 2) // tiles, total_steps // 2))
    if total_steps <= 512:
        best, sl = 1e30, 1
        for sm in range(1, min(32, total_steps) + 1):
            per = (total_steps + sm - 1) // sm
            blocks = tiles * ((total_steps + per - 1) // per)
            rounds = (blocks + 511) // 512
            t = float(rounds * per) * 1.0 + float(tiles) * 16384.0 * sm * 2.7e-6
            if t < best:
                best, sl = t, sm
    return sl


def geometry(dtype, M, N, K, slices=0):
    """(slices, steps per slice, workspace bytes) of a launch reducing M pixels into an [N, K] gradient"""
    total = (M + px(dtype) - 1) // px(dtype)
    sl = slices if slices > 0 else rule_slices(total, ((N + 127) // 128) * ((K + 127) // 128))
    sl = min(sl, total)
    per = (total + sl - 1) // sl
    sl = (total + per - 1) // per
    return sl, per, sl * (N * K + N) * 4


def case_dims(case, dtype):
    """The sizes of a WGRAD_CASES row as the launch sees them: dict of B, H, W, OH, OW, pad, C (padded channels per
    source), N, K, M."""
    name, B, cins, H, W, Cout, KH, stride, pad_mode, ups, _splitm = case
    He, We = (2 * H, 2 * W) if ups else (H, W)
    if pad_mode == "same":
        pad, OH, OW = KH // 2, (He + 2 * (KH // 2) - KH) // stride + 1, (We + 2 * (KH // 2) - KH) // stride + 1
    elif pad_mode == "asym":
        pad, OH, OW = 0, (He + 1 - KH) // stride + 1, (We + 1 - KH) // stride + 1
    else:
        pad, OH, OW = 0, (He - KH) // stride + 1, (We - KH) // stride + 1
    C = [round_up(c, k_tile(dtype)) for c in cins]
    return dict(B=B, H=H, W=W, OH=OH, OW=OW, pad=pad, C=C, N=Cout, K=KH * KH * sum(C), M=B * OH * OW, KH=KH, stride=stride, ups=ups)


def case_geometry(case, dtype, slices=0):
    d = case_dims(case, dtype)
    return geometry(dtype, d["M"], d["N"], d["K"], slices)


def distinct_slices(case, dtype):
    """The requested slice counts of FORCED whose clamped counts differ, in order: [(requested, effective)]"""
    out, seen = [], set()
    for s in FORCED:
        eff = case_geometry(case, dtype, s)[0]
        if eff not in seen:
            seen.add(eff)
            out.append((s, eff))
    return out


def exact_params():
    """(id, case, dtype, requested slices, effective slices) of the exact GPU test"""
    return [(f"{c[0]}-{dn}-s{s}", c, dt, s, eff) for c in WGRAD_CASES for dt, dn in zip(DT3, ID3) for s, eff in distinct_slices(c, dt)]


def fill_args(Lw, dtype, d, slices=0, ptrs=None):
    """mws_conv2d_wgrad_args of case_dims' sizes; ``ptrs``: dict of in1, in2, dout, dw, dbias, workspace (addresses),
    workspace_bytes, ld1, ld2, ldd"""
    a = Lw.Conv2dWgradArgs()
    a.dtype = DTYPE_CODE[dtype]
    a.C1, a.C2 = d["C"][0], (d["C"][1] if len(d["C"]) > 1 else 0)
    a.B, a.IH, a.IW, a.OH, a.OW = d["B"], d["H"], d["W"], d["OH"], d["OW"]
    a.KH = a.KW = d["KH"]
    a.stride, a.pad_t, a.pad_l, a.upsample = d["stride"], d["pad"], d["pad"], 1 if d["ups"] else 0
    a.N, a.slices = d["N"], slices
    for k, v in (ptrs or {}).items():
        setattr(a, k, v)
    return a


def query(Lw, a):
    """(slices, steps per slice, workspace bytes) the library answers for these arguments"""
    r = ctypes.byref(a)
    return Lw.lib.mws_conv2d_wgrad_slices(r), Lw.lib.mws_conv2d_wgrad_steps_per_slice(r), Lw.lib.mws_conv2d_wgrad_workspace_bytes(r)


# ---- float64 references by pixel slice -------------------------------------------------------------------------------------------

def wgrad_f64(x, dy, KH, stride, pad_mode, ups):
    """(dw [Cout, Cin, KH, KH], dbias [Cout]) of the conv statement of tests/test_ops_gpu.py by autograd, float64 CPU"""
    w = torch.zeros((dy.shape[1], x.shape[1], KH, KH), dtype=torch.float64, requires_grad=True)
    y, _ = L._conv_statement(x.double(), w, KH, stride, pad_mode, ups)
    y.backward(dy.double())
    return w.grad.detach(), dy.double().sum((0, 2, 3))


def slice_mask(dy, first, last):
    """dy (NCHW) with every output pixel outside [first, last) of the (image, y, x) order set to zero"""
    B, C, OH, OW = dy.shape
    m = torch.arange(B * OH * OW).view(B, 1, OH, OW)
    return dy * ((m >= first) & (m < last))


@functools.lru_cache(maxsize=None)
def sliced_reference(name, dtype_is_f32, slices):
    """The lattice reference of a WGRAD_CASES row cut as the kernel cuts it: (ref, [(dw_z, dbias_z)], magnitude) with the
    partial gradients of the pixel slices of ``slices`` requested slices (16-pixel steps for f32, 32 otherwise) and the sum
    of the products' magnitudes per dw element."""
    case = next(c for c in WGRAD_CASES if c[0] == name)
    dtype = F32 if dtype_is_f32 else F16
    ref = L.ref_wgrad_row(case, dtype)
    _n, B, cins, H, W, Cout, KH, stride, pad_mode, ups, _s = case
    x = torch.cat(ref.xs, 1)
    sl, per, _ws = case_geometry(case, dtype, slices)
    parts = []
    for z in range(sl):
        parts.append(wgrad_f64(x, slice_mask(ref.dy, z * per * px(dtype), (z + 1) * per * px(dtype)), KH, stride, pad_mode, ups))
    mag, _ = wgrad_f64(x.abs(), ref.dy.abs(), KH, stride, pad_mode, ups)
    return ref, parts, mag


def mutants(ref, parts, z):
    """What a comparison must reject: {name: (dw, dbias)} with slice z dropped, counted twice, and its bias partial dropped"""
    dwz, dbz = parts[z]
    return {"slice dropped": (ref.out - dwz, ref.dbias - dbz), "slice counted twice": (ref.out + dwz, ref.dbias + dbz),
            "bias partial dropped": (ref.out, ref.dbias - dbz)}


def same(got, want):
    """The comparison of the exact tests: both gradients equal, as torch.equal sees it"""
    return bool(torch.equal(got[0], want[0])) and bool(torch.equal(got[1], want[1]))


def ints(shape, seed, amp):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()


# ---- the library file ------------------------------------------------------------------------------------------------------------

def lib_path():
    return os.environ.get("MADM_WSLAB_LIB") or os.path.join(ROOT, "madm_amd", "libmadm_wslab.so")


def assert_exports_exactly_the_header():
    """of the project's prefixes (sidelib_util.PREFIXES and this library's own) the file exports what include/madm_wslab.h
    declares, nothing more or less; returns all exports"""
    from madm_amd import _cabi
    exported = su.exports(lib_path())
    mine = {s for s in exported if s.startswith(su.PREFIXES + ("mws_",))}
    declared = {n for n, _r, _p in _cabi.parse(os.path.join(ROOT, "include", "madm_wslab.h")).prototypes}
    assert mine == declared, (sorted(mine - declared), sorted(declared - mine))
    return exported
