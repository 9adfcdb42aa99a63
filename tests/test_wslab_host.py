"""Host-side checks of the ordered-slab weight gradient's library (include/madm_wslab.h, libmadm_wslab.so,
madm_amd/_lib_wslab.py): the header and the exports, lazy loading, argument checks without a GPU, the
shapes-only launch geometry against the tests' own restatement (tests/wslab_util.py), the exactness conditions and negative
controls of the lattice inputs tests/test_wslab_gpu.py compares with torch.equal, and the two static scans tests/test_host.py
runs over the main library.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import sidelib_util as su
import wslab_util as wu

ROOT = wu.ROOT


def test_header_declares_only_its_own_names():
    from madm_amd import _cabi
    abi = _cabi.parse(os.path.join(ROOT, "include", "madm_wslab.h"))
    names = [n for n, _r, _p in abi.prototypes]
    assert names and all(n.startswith("mws_") for n in names), names
    assert abi.constants and all(k.startswith("MWS_") for k in abi.constants), abi.constants
    assert list(abi.structs) == ["mws_conv2d_wgrad_args"]
    assert set(names) == {"mws_abi_version", "mws_last_error", "mws_conv2d_wgrad", "mws_conv2d_wgrad_slices",
                          "mws_conv2d_wgrad_steps_per_slice", "mws_conv2d_wgrad_workspace_bytes"}
    for n, _r, params in abi.prototypes:      # the launching entry point ends in a stream, the queries take the sizes only
        assert bool(params and params[-1][0] == "stream") == (n == "mws_conv2d_wgrad"), n
    main = _cabi.parse(os.path.join(ROOT, "include", "madm_hip.h"))
    assert [abi.constants[k] for k in ("MWS_F32", "MWS_BF16", "MWS_F16")] == [main.constants[k] for k in ("MADM_F32", "MADM_BF16", "MADM_F16")]
    assert (abi.constants["MWS_TARGET_BLOCKS"], abi.constants["MWS_MAX_SLICES"]) == (wu.TARGET_BLOCKS, wu.MAX_SLICES)
    # the fields of madm_conv2d_wgrad_args restated (all but splitm), then slices, workspace, workspace_bytes
    mine = [f for f, _t in abi.struct("mws_conv2d_wgrad_args")._fields_]
    theirs = [f for f, _t in main.struct("madm_conv2d_wgrad_args")._fields_ if f != "splitm"]
    assert mine == theirs + ["slices", "workspace", "workspace_bytes"]


def test_library_exports_exactly_the_header():
    exported = wu.assert_exports_exactly_the_header()
    assert not any(s.startswith(su.PREFIXES) for s in exported)


def test_import_and_the_one_slice_mode_do_not_load_the_library():
    code = ("import sys, madm_amd, madm_amd.ops as ops, madm_amd.train\n"
            "from madm_amd.train import MadmTrainer\n"
            "def absent():\n"
            "    return 'madm_amd._lib_wslab' not in sys.modules and 'libmadm_wslab' not in open('/proc/self/maps').read()\n"
            "assert absent() and ops.wgrad_path() == 'atomic'\n"
            "assert ops.set_deterministic(True) is False and absent()\n"
            "assert ops.is_deterministic() is True and ops.wgrad_path() == 'one_slice'\n"
            "assert ops.set_deterministic('slabs') is True and absent()          # loaded by the first launch, not by the switch\n"
            "assert ops.is_deterministic() is True and ops.wgrad_path() == 'slabs'\n"
            "assert ops.set_deterministic(False) == 'slabs' and ops.is_deterministic() is False and ops.wgrad_path() == 'atomic'\n"
            "with ops.deterministic('slabs'):\n"
            "    with ops.deterministic(True):\n"
            "        assert ops.wgrad_path() == 'one_slice'\n"
            "        with ops.deterministic(False):\n"
            "            assert ops.wgrad_path() == 'atomic' and not ops.is_deterministic()\n"
            "        assert ops.wgrad_path() == 'one_slice'\n"
            "    assert ops.wgrad_path() == 'slabs' and ops.is_deterministic() is True\n"
            "assert ops.wgrad_path() == 'atomic'\n"
            "try:\n"
            "    ops.set_deterministic('slab')\n"
            "    raise SystemExit('an unknown mode name was accepted')\n"
            "except ValueError:\n"
            "    pass\n"
            "assert ops.wgrad_path() == 'atomic'\n"
            "import torch\n"
            "for value in (True, 'slabs'):     # a trainer's construction (a small CPU module) loads neither side library\n"
            "    t = MadmTrainer(torch.nn.Linear(4, 4), lr=1e-4, weight_decay=0.0, deterministic=value)\n"
            "    assert t.deterministic is value or t.deterministic == value\n"
            "    assert absent() and ops.wgrad_path() == 'atomic'\n"
            "assert MadmTrainer(torch.nn.Linear(4, 4), lr=1e-4, weight_decay=0.0).deterministic is False\n"
            "assert absent()\n"
            "from madm_amd import _lib_wslab\n"
            "assert 'libmadm_wslab' in open('/proc/self/maps').read() and _lib_wslab.lib.mws_abi_version() == _lib_wslab.ABI_VERSION == 1\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_trainer_keeps_the_mode_value():
    """MadmTrainer stores False / True / "slabs" and run_step passes the value to ops.deterministic: trainers built on a small
    CPU module, with the step itself (which needs the GPU) replaced by a probe of the mode; another string is refused"""
    import torch
    from madm_amd import ops
    from madm_amd.train import MadmTrainer
    with pytest.raises(ValueError, match="'slabs'"):
        MadmTrainer(torch.nn.Linear(4, 4), lr=1e-4, weight_decay=0.0, deterministic="slab")
    for value, want in ((False, ("atomic", False)), (True, ("one_slice", True)), ("slabs", ("slabs", True)), (1, ("one_slice", True))):
        t = MadmTrainer(torch.nn.Linear(4, 4), lr=1e-4, weight_decay=0.0, deterministic=value)
        assert t.deterministic == value and type(t.deterministic) in (bool, str)
        t._run_step = lambda data: (ops.wgrad_path(), ops.is_deterministic())
        assert t.run_step(None) == want
        assert ops.wgrad_path() == "atomic" and ops.is_deterministic() is False


# ---- argument checks: nothing below touches a GPU (every call must fail before its launch) --------------------------------------

def _good(Lw, m, dtype=wu.F32):
    d = dict(B=2, H=6, W=6, OH=6, OW=6, pad=1, C=[8], N=8, K=72, M=72, KH=3, stride=1, ups=False)
    a = wu.fill_args(Lw, dtype, d)
    need = Lw.lib.mws_conv2d_wgrad_workspace_bytes(ctypes.byref(a))
    assert 0 < need < 16384
    ptrs = dict(in1=m.at(0).value, dout=m.at(4096).value, dw=m.at(8192).value, dbias=m.at(12288).value, workspace=m.at(16384).value,
                workspace_bytes=need)
    return wu.fill_args(Lw, dtype, d, ptrs=ptrs), need


def test_bad_arguments_are_refused_without_a_gpu():
    from madm_amd import _lib_wslab as Lw
    m = su.Host()

    def refused(change, what, dtype=wu.F32, expect=None):
        a, _need = _good(Lw, m, dtype)
        for k, v in change.items():
            setattr(a, k, v)
        other, _need = _good(Lw, m)                                          # another message first
        other.dtype = 3 if expect == "null argument" else 0
        other.in1 = other.in1 if expect == "null argument" else None
        Lw.lib.mws_conv2d_wgrad(ctypes.byref(other), None)
        before = Lw.last_error()
        rc = Lw.lib.mws_conv2d_wgrad(ctypes.byref(a), None)
        assert rc == Lw.MWS_ERR_INVALID_ARG, f"{what} was not refused (status {rc})"
        msg = Lw.last_error()
        assert msg.startswith("conv2d_wgrad:") and msg != before and (expect or "") in msg, (what, msg)

    a, need = _good(Lw, m)
    for f in ("in1", "dout", "dw", "workspace"):
        refused({f: None}, f"null {f}", expect="null argument")
    refused({"C2": 8}, "a second source without its pointer", expect="channel split")
    for f in ("in1", "workspace"):
        refused({f: getattr(a, f) + 4}, f"{f} off a 16-byte boundary", expect="16-byte aligned")
    refused({"dout": a.dout + 4}, "dout off its 16-byte boundary (f32: 4 elements)", expect="dout must be aligned")
    refused({"dout": a.dout + 4}, "dout off its 8-byte boundary (f16: 4 elements)", dtype=wu.F16, expect="dout must be aligned")
    refused({"dw": a.dw + 2}, "dw off a 4-byte boundary", expect="4-byte aligned")
    refused({"dbias": a.dbias + 2}, "dbias off a 4-byte boundary", expect="4-byte aligned")
    refused({"N": 6}, "N % 4 != 0", expect="multiple of 4")
    refused({"C1": 6}, "C1 % epc != 0 (f32)", expect="multiples of 4")
    refused({"C1": 12}, "C1 % epc != 0 (f16)", dtype=wu.F16, expect="multiples of 8")
    refused({"ld1": 10}, "ld1 not a multiple of the chunk", expect="row strides")
    refused({"ldd": 10}, "ldd not a multiple of 4", expect="row strides")
    refused({"dtype": 3}, "unknown dtype", expect="unknown dtype")
    refused({"workspace_bytes": need - 1}, "a workspace one byte short", expect=f"{need} needed")
    refused({"slices": wu.MAX_SLICES + 1}, "a slice count above the grid limit", expect="grid too large")
    refused({"slices": -1}, "a negative slice count", expect="slices")
    for f in ("B", "IH", "IW", "OH", "OW", "KH", "KW", "stride", "N", "C1"):
        for z in (0, -1):
            refused({f: z}, f"{f} = {z}")
    # a forced slice count whose slabs would pass 2^31 bytes: the index width the kernels were checked for
    big = dict(B=1, IH=1 << 15, IW=1, OH=1 << 15, OW=1, KH=1, KW=1, pad_t=0, pad_l=0, N=1024, C1=1024, slices=1024, workspace_bytes=1 << 40)
    refused(big, "slabs of 4 GiB", expect="at most 2 GiB")
    # and the good call is good up to the launch: with no GPU in the process the status is the launch's, not the arguments'
    a, _ = _good(Lw, m)
    if not torch.cuda.is_available():
        assert Lw.lib.mws_conv2d_wgrad(ctypes.byref(a), None) == Lw.MWS_ERR_LAUNCH and "launch failed" in Lw.last_error()


def test_queries_answer_zero_for_bad_sizes():
    from madm_amd import _lib_wslab as Lw
    good, _ = _good(Lw, su.Host())
    assert wu.query(Lw, good)[0] > 0
    assert Lw.lib.mws_conv2d_wgrad_slices(None) == 0 and Lw.lib.mws_conv2d_wgrad_workspace_bytes(None) == 0
    for f in ("B", "OH", "OW", "KH", "KW", "N", "C1"):
        a, _ = _good(Lw, su.Host())
        setattr(a, f, 0)
        assert wu.query(Lw, a) == (0, 0, 0), f
    a, _ = _good(Lw, su.Host())
    a.dtype = 7
    assert wu.query(Lw, a) == (0, 0, 0)


# ---- the launch geometry -------------------------------------------------------------------------------------------------------

# (M, N, K) of weight gradients of the 512 x 512 training step and of short and ragged reductions
SHAPES = [(2 * 512 * 512, 128, 1152), (2 * 256 * 256, 256, 2304), (2 * 64 * 64, 320, 2880), (2 * 32 * 32, 640, 5760),
          (2 * 16 * 16, 1280, 11520), (2 * 8 * 8, 1280, 23040), (2 * 4096, 320, 320), (2 * 77, 320, 768), (154, 1280, 320),
          (1, 4, 4), (15, 4, 8), (16, 8, 8), (17, 8, 8), (33, 68, 576), (16385, 128, 128), (1 << 20, 4, 36)]


def _shape_args(Lw, dtype, M, N, K, slices):
    d = dict(B=1, H=M, W=1, OH=M, OW=1, pad=0, C=[K], N=N, K=K, M=M, KH=1, stride=1, ups=False)
    return wu.fill_args(Lw, dtype, d, slices)


def test_launch_geometry_is_a_function_of_the_shapes():
    from madm_amd import _lib, _lib_wslab as Lw

    def table():
        rows = [wu.query(Lw, _shape_args(Lw, dt, M, N, K, s)) for dt in wu.DT3 for M, N, K in SHAPES for s in wu.FORCED + (3, 33, 65535)]
        rows += [wu.query(Lw, wu.fill_args(Lw, dt, wu.case_dims(c, dt), s)) for c in wu.WGRAD_CASES for dt in wu.DT3 for s in wu.FORCED]
        return rows

    first = table()
    want = [wu.geometry(dt, M, N, K, s) for dt in wu.DT3 for M, N, K in SHAPES for s in wu.FORCED + (3, 33, 65535)]
    # for every row of WGRAD_CASES and every slice count the GPU tests force: the query against the restatement
    want += [wu.case_geometry(c, dt, s) for c in wu.WGRAD_CASES for dt in wu.DT3 for s in wu.FORCED]
    assert first == want
    assert table() == first
    prev = _lib.lib.madm_get_tuning_profile()
    try:
        for code in (0, 1):
            assert _lib.lib.madm_set_tuning_profile(code) == 0
            assert table() == first
    finally:
        _lib.lib.madm_set_tuning_profile(prev)
    # slices x steps per slice covers all steps, no slice is empty, the slabs stay below the entry point's bound
    i = 0
    for dt in wu.DT3:
        for M, N, K in SHAPES:
            for s in wu.FORCED + (3, 33, 65535):
                sl, per, ws = first[i]
                i += 1
                total = (M + wu.px(dt) - 1) // wu.px(dt)
                assert sl >= 1 and per >= 1 and sl * per >= total, (M, N, K, s)
                assert (sl - 1) * per < total, f"slice {sl - 1} of {(M, N, K, s)} is empty"
                assert sl <= (s or total) and ws == sl * (N * K + N) * 4
                if s == 0:      # the rule: (past the short-reduction model) at least two steps per slice
                    assert ws < 1 << 31 and (sl == 1 or per >= 2 or total <= 512), (M, N, K)
    # the rule splits where the tiles alone leave the chip idle and does not where they fill it
    assert wu.geometry(wu.F16, 2 * 512 * 512, 128, 1152)[0] > 32 and wu.geometry(wu.F16, 2 * 8 * 8, 1280, 23040)[0] == 1
    # the case table of the GPU tests reaches what it is meant to reach: a remainder slice, an odd step count, M % PX != 0
    geos = [(c[0], dt, wu.case_dims(c, dt), wu.case_geometry(c, dt, s)) for c in wu.WGRAD_CASES for dt in wu.DT3 for s in wu.FORCED]
    steps = lambda d, dt: (d["M"] + wu.px(dt) - 1) // wu.px(dt)      # noqa: E731
    assert any(sl > 1 and steps(d, dt) % per for _n, dt, d, (sl, per, _w) in geos), "no remainder slice"
    assert any(sl > 1 and per % 2 for _n, dt, d, (sl, per, _w) in geos), "no odd step count"
    assert any(sl > 1 and d["M"] % wu.px(dt) for _n, dt, d, (sl, per, _w) in geos), "no ragged last step"
    assert {eff for c in wu.WGRAD_CASES for dt in wu.DT3 for _s, eff in wu.distinct_slices(c, dt)} >= {1, 2, 7}


# ---- exactness conditions and negative controls ---------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", [True, False], ids=["px16", "px32"])
@pytest.mark.parametrize("case", wu.WGRAD_CASES, ids=[c[0] for c in wu.WGRAD_CASES])
def test_lattice_rows_are_exact_in_every_partition_and_the_comparison_sees_a_lost_slice(case, f32):
    dtype = wu.F32 if f32 else wu.F16
    slices = max(eff for _s, eff in wu.distinct_slices(case, dtype))
    ref, parts, mag = wu.sliced_reference(case[0], f32, slices)
    # the sum of the products' magnitudes bounds every partial sum of every partition into slices and every order inside one
    assert float(mag.max()) < wu.L.ACC_MAX and float(ref.dy.abs().sum((0, 2, 3)).max()) < wu.L.ACC_MAX
    assert len(parts) == wu.case_geometry(case, dtype, slices)[0]
    assert torch.equal(sum(p[0] for p in parts), ref.out) and torch.equal(sum(p[1] for p in parts), ref.dbias)
    if len(parts) == 1:
        return
    for z in (0, len(parts) - 1):
        for what, m in wu.mutants(ref, parts, z).items():
            assert not wu.same(m, (ref.out, ref.dbias)), f"{what} (slice {z}): the comparison does not see it"


def test_wslab_kernels_use_no_scratch_and_no_packed_fp32():
    from madm_amd._lib_wslab import LIB_PATH
    rows = su.scan_kernels(LIB_PATH)
    names = " ".join(rows)
    assert len(rows) == 4 and names.count("wslab_kernel") == 3 and "wslab_fold_kernel" in names, sorted(rows)
