"""Host-side checks of the deterministic mode's library (include/madm_det.h, libmadm_det.so, madm_amd/_lib_det.py): the
header and the exports, lazy loading, argument checks without a GPU, the shapes-only launch geometry, the exactness conditions
and negative controls of the lattice inputs tests/test_det_gpu.py compares with torch.equal, and the two static scans
tests/test_host.py runs over the main library.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import det_util as du
import sidelib_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mdet_colsum", "mdet_groupnorm_stats", "mdet_groupnorm_bwd_sums", "mdet_groupnorm_bwd_params",
                "mdet_layernorm_bwd_params", "mdet_dwconv3x3_wgrad"]


def test_header_declares_only_its_own_names():
    from madm_amd import _cabi
    abi = _cabi.parse(os.path.join(ROOT, "include", "madm_det.h"))
    names = [n for n, _r, _p in abi.prototypes]
    assert names and all(n.startswith("mdet_") for n in names), names
    assert abi.constants and all(k.startswith("MDET_") for k in abi.constants), abi.constants
    assert not abi.structs
    assert set(ENTRY_POINTS) <= set(names) and {"mdet_abi_version", "mdet_last_error", "mdet_slices"} <= set(names)
    # the launching entry points end in a stream, the queries take sizes only
    for n, _r, params in abi.prototypes:
        assert bool(params and params[-1][0] == "stream") == (n in ENTRY_POINTS), n
    # the dtype codes are the main header's
    main = _cabi.parse(os.path.join(ROOT, "include", "madm_hip.h")).constants
    assert [abi.constants[k] for k in ("MDET_F32", "MDET_BF16", "MDET_F16")] == [main[k] for k in ("MADM_F32", "MADM_BF16", "MADM_F16")]
    assert (abi.constants["MDET_MIN_SLICE_ROWS"], abi.constants["MDET_MAX_SLICES"]) == (du.MIN_SLICE_ROWS, du.MAX_SLICES)


def test_library_exports_exactly_the_header():
    path = os.environ.get("MADM_DET_LIB") or os.path.join(ROOT, "madm_amd", "libmadm_det.so")
    exported = su.assert_exports_exactly(path, "madm_det.h")
    assert not any(s.startswith("madm_") for s in exported)


def test_import_does_not_load_the_library():
    code = ("import sys, madm_amd, madm_amd.ops as ops, madm_amd.train\n"
            "assert 'madm_amd._lib_det' not in sys.modules\n"
            "assert 'libmadm_det' not in open('/proc/self/maps').read()\n"
            "assert ops.is_deterministic() is False\n"
            "assert ops.set_deterministic(False) is False and 'madm_amd._lib_det' not in sys.modules\n"
            "with ops.deterministic():\n"
            "    assert ops.is_deterministic() and 'madm_amd._lib_det' in sys.modules\n"
            "    assert 'libmadm_det' in open('/proc/self/maps').read()\n"
            "assert ops.is_deterministic() is False\n"
            "try:\n"
            "    with ops.deterministic():\n"
            "        raise KeyError('x')\n"
            "except KeyError:\n"
            "    pass\n"
            "assert ops.is_deterministic() is False\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


# ---- argument checks: nothing below touches a GPU (every call must fail before its launch) --------------------------------------

def _calls(L, m, ws_bytes):
    """{entry point: (function, good argument list, {argument index: what it is})} for a small f32 shape"""
    B, HW, C = 2, 40, 8
    p = lambda i: m.at(4096 * i)      # noqa: E731
    q = L.lib
    return {
        "mdet_colsum": (q.mdet_colsum, [0, p(0), C, B, HW, C, p(1), p(2), ws_bytes("colsum", B, HW, C), None],
                        dict(ptr=[1, 6, 7], al16=[1, 7], C=5, ws=8, dtype=0)),
        "mdet_groupnorm_stats": (q.mdet_groupnorm_stats, [0, p(0), B, HW, C, p(1), p(2), ws_bytes("groupnorm_stats", B, HW, C), None],
                                 dict(ptr=[1, 5, 6], al16=[1, 6], C=4, ws=7, dtype=0)),
        "mdet_groupnorm_bwd_sums": (q.mdet_groupnorm_bwd_sums,
                                    [0, p(0), p(1), C, B, HW, C, 0, C, 2, p(2), C, None, p(3), p(4), 0.0, 0, p(5), p(6),
                                     ws_bytes("groupnorm_bwd_sums", B, HW, C), None],
                                    dict(ptr=[1, 2, 10, 13, 14, 17, 18], al16=[1, 2, 18], C=6, ws=19, dtype=0)),
        "mdet_groupnorm_bwd_params": (q.mdet_groupnorm_bwd_params, [p(0), B, C, p(1), p(2), None], dict(ptr=[0, 3, 4], al16=[], C=None, ws=None,
                                                                                                        dtype=None)),
        "mdet_layernorm_bwd_params": (q.mdet_layernorm_bwd_params,
                                      [0, p(0), p(1), HW, C, 1e-5, p(2), p(3), p(4), ws_bytes("layernorm_bwd_params", HW, C), None],
                                      dict(ptr=[1, 2, 6, 7, 8], al16=[1, 2, 8], C=4, ws=9, dtype=0)),
        "mdet_dwconv3x3_wgrad": (q.mdet_dwconv3x3_wgrad,
                                 [0, p(0), p(1), C, p(2), B, 5, 8, C, 6, p(3), ws_bytes("dwconv3x3_wgrad", B, 5, 8, C), None],
                                 dict(ptr=[1, 2, 4, 10], al16=[1, 2, 10], C=8, ws=11, dtype=0)),
    }


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_bad_arguments_are_refused_without_a_gpu(entry):
    from madm_amd import _lib_det as L
    m = su.Host()

    def ws_bytes(family, *shape):
        n = getattr(L.lib, f"mdet_{family}_workspace_bytes")(*shape)
        assert 0 < n < 4096 * 8
        return n

    fn, good, spec = _calls(L, m, ws_bytes)[entry]

    def refused(args, what):
        if entry == "mdet_colsum":                                        # another entry point's message first
            L.lib.mdet_groupnorm_bwd_params(None, 0, 0, None, None, None)
        else:
            L.lib.mdet_colsum(0, None, 0, 0, 0, 0, None, None, 0, None)
        assert entry[len("mdet_"):] not in L.last_error()
        rc = fn(*args)
        assert rc == L.MDET_ERR_INVALID_ARG, f"{entry}: {what} was not refused (status {rc})"
        msg = L.last_error()
        assert entry[len("mdet_"):] + ":" in msg, (what, msg)

    for i in spec["ptr"]:
        bad = list(good)
        bad[i] = None
        refused(bad, f"null argument {i}")
    for i in spec["al16"]:
        bad = list(good)
        bad[i] = ctypes.c_void_p(good[i].value + 4)
        refused(bad, f"argument {i} off a 16-byte boundary")
    if spec["C"] is not None:
        bad = list(good)
        bad[spec["C"]] = good[spec["C"]] + 2                            # 10: not a multiple of the f32 chunk of 4
        refused(bad, "C not a multiple of the chunk")
        bad = list(good)
        bad[0] = 1                                                        # bf16: a chunk is 8 elements
        bad[spec["C"]] = 12
        refused(bad, "C not a multiple of the 16-bit chunk")
        bad = list(good)
        bad[spec["dtype"]] = 3
        refused(bad, "unknown dtype")
    if spec["ws"] is not None:
        bad = list(good)
        bad[spec["ws"]] = good[spec["ws"]] - 1
        refused(bad, "workspace one byte short of its query")
    for i, v in enumerate(good):                                          # every size: zero and negative
        if isinstance(v, int) and not isinstance(v, bool) and i not in (spec["ws"], spec["dtype"]) and v > 0:
            for z in (0, -1):
                bad = list(good)
                bad[i] = z
                refused(bad, f"size argument {i} = {z}")


def test_launch_geometry_is_a_function_of_the_shapes():
    """The queries against their restatement, twice, and under both tuning profiles of the main library."""
    from madm_amd import _lib, _lib_det as L
    q = L.lib
    shapes = [(B, R) for B in (1, 2, 3, 7, 1024, 5000) for R in (1, 9, 16, 17, 33, 37, 600, 4096, 262144, 1 << 22)]

    def table():
        rows = [q.mdet_slices(B, R) for B, R in shapes]
        rows += [q.mdet_dwconv3x3_wgrad_slices(B, H, W) for B in (1, 2, 3) for H, W in ((13, 13), (20, 20), (512, 512))]
        rows += [q.mdet_colsum_workspace_bytes(2, 37, 64), q.mdet_groupnorm_stats_workspace_bytes(2, 37, 64),
                 q.mdet_groupnorm_bwd_sums_workspace_bytes(2, 262144, 1024), q.mdet_layernorm_bwd_params_workspace_bytes(37, 64),
                 q.mdet_dwconv3x3_wgrad_workspace_bytes(2, 512, 512, 1024)]
        return rows

    first = table()
    assert first[:len(shapes)] == [du.image_slices(B, R)[0] for B, R in shapes]
    assert first[len(shapes):len(shapes) + 9] == [du.slices_for(B * H * W, du.DW_MAX_SLICES)[0]
                                                  for B in (1, 2, 3) for H, W in ((13, 13), (20, 20), (512, 512))]
    assert first[-5:] == [2 * 3 * 64 * 4, 2 * 3 * 2 * 64 * 4, 2 * 512 * 2 * 1024 * 4, (3 * 2 * 64 + 2 * 37) * 4, 256 * 9 * 1024 * 4]
    assert table() == first
    prev = _lib.lib.madm_get_tuning_profile()
    try:
        for code in (0, 1):
            assert _lib.lib.madm_set_tuning_profile(code) == 0
            assert table() == first
    finally:
        _lib.lib.madm_set_tuning_profile(prev)
    assert q.mdet_slices(0, 5) == 0 and q.mdet_slices(2, 0) == 0 and q.mdet_dwconv3x3_wgrad_slices(1, 0, 4) == 0
    # the case tables of the GPU tests have the slice counts they are meant to have
    for name, B, R, chunks, slices in du.ROW_CASES:
        assert q.mdet_slices(B, R) == slices, name
    for name, B, H, W, dil, chunks, slices in du.DW_CASES:
        assert q.mdet_dwconv3x3_wgrad_slices(B, H, W) == slices, name
    assert {c[4] for c in du.ROW_CASES} >= {1, 3} and max(c[3] for c in du.ROW_CASES) > 256


def _all_cases():
    out = []
    for dt, dn in zip(du.DT3, du.ID3):
        for fam in du.FAMILIES[:4]:
            for name, B, R, chunks, slices in du.ROW_CASES:
                out.append((f"{fam}-{name}-{dn}", lambda fam=fam, name=name, C=chunks * du.epc(dt): du.row_case(fam, name, C)))
        for name, B, R, chunks, slices in du.ROW_CASES[1:3]:
            out.append((f"groupnorm_bwd_sums-two_source-{name}-{dn}",
                        lambda name=name, C=chunks * du.epc(dt): du.row_case("groupnorm_bwd_sums", name, C, True)))
        for name, B, H, W, dil, chunks, slices in du.DW_CASES:
            out.append((f"dwconv3x3_wgrad-{name}-{dn}", lambda name=name, C=chunks * du.epc(dt): du.dw_case(name, C)))
    return out


@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: c[0])
def test_lattice_inputs_are_exact_and_the_comparison_sees_a_lost_row(case):
    """Every term and every partial sum an integer below 2^24 (the sum of magnitudes bounds every order); the float64
    reference changes when one row is dropped, one row is counted twice or one slice's partial is left out."""
    ns = du.check_exact(case[1]())
    ref = du.reduce(ns)
    assert bool(torch.equal(ref, ref.round())) and float(ref.abs().max()) < du.ACC_MAX
    if ns.family == "layernorm_bwd_params":
        assert du.ln_width_is_exact(ns.C)
        assert bool((ns.x.sum(1) == 0).all()) and bool(((ns.x * ns.x).sum(1) == ns.C).all())     # mean 0, variance 1
    if ns.family == "groupnorm_bwd_sums":
        # the statistics handed to the kernel: group mean 0, variance count * (1 / count), which is 1.0f in f32
        import numpy as np
        cnt = float(ns.count)
        assert np.float32(cnt * (1.0 / cnt)) == np.float32(1.0)
    per = du.slices_for(ns.R, du.DW_MAX_SLICES)[1] if ns.family == "dwconv3x3_wgrad" else du.image_slices(ns.B, ns.R)[1]
    for what, w in du.mutants(ns, per).items():
        assert not torch.equal(du.reduce(ns, w), ref), f"{what}: the reference does not change"


def test_det_kernels_use_no_scratch_and_no_packed_fp32():
    from madm_amd._lib_det import LIB_PATH
    rows = su.scan_kernels(LIB_PATH)
    names = " ".join(rows)
    # five functors x three dtypes, the fold, the GroupNorm parameter kernel, the LayerNorm row statistics x three dtypes
    assert len(rows) == 20 and names.count("partials_kernel") == 15 and "fold_kernel" in names, sorted(rows)
