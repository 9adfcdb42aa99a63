"""What the host tests of the three side libraries (libmadm_data.so, libmadm_det.so, libmadm_headfuse.so) share: the
project's scanners loaded by path, the list of a built library's exports, host memory standing in for device buffers, and
the two static scans tests/test_host.py runs over the main library.  No GPU."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIXES = ("madm_", "mdata_", "mdet_", "mhf_")     # every library's own names


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def exports(path):
    """every defined dynamic symbol of the library (text, data, bss); skips the test when there is no nm"""
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if nm is None:
        pytest.skip("no nm to list the library's exports")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TtDdBb"}


def assert_exports_exactly(path, header):
    """of the project's prefixes the library exports what its header declares, nothing more or less; returns all exports"""
    from madm_amd import _cabi
    exported = exports(path)
    mine = {s for s in exported if s.startswith(PREFIXES)}
    declared = {n for n, _r, _p in _cabi.parse(os.path.join(ROOT, "include", header)).prototypes}
    assert mine == declared, (sorted(mine - declared), sorted(declared - mine))
    return exported


class Host:
    """Host memory standing in for device buffers: a refused call never dereferences it."""

    def __init__(self, nbytes=1 << 16):
        self.buf = ctypes.create_string_buffer(nbytes + 64)
        self.p = (ctypes.addressof(self.buf) + 63) & ~63

    def at(self, off=0):
        return ctypes.c_void_p(self.p + off)


def scan_kernels(lib_path):
    """{kernel: metadata} of the built library after asserting that no kernel uses scratch or spills and that its gfx950 code
    holds no packed-FP32 op; skips the test without the ROCm toolchain's llvm-readelf / llvm-objdump"""
    scratch, pk = tool("scratch_scan"), tool("isa_pk_scan")
    if not (os.path.exists(scratch.READELF) or shutil.which(scratch.READELF)) or \
            not (os.path.exists(pk.OBJDUMP) or shutil.which(pk.OBJDUMP)):
        pytest.skip("llvm-readelf / llvm-objdump of the ROCm toolchain not found")
    rows = scratch.kernels(lib_path)
    bad = {k: v for k, v in rows.items() if v.get("private_segment_fixed_size", 0) > 0 or v.get("vgpr_spill_count", 0) > 0}
    assert not bad, f"kernels with scratch: {bad}"
    assert len(pk.code_objects(lib_path)) >= 1, "no gfx950 code object found in the library"
    total, low, per = pk.scan(lib_path)
    assert total == 0 and low == 0 and not per, f"packed-FP32 ops in {os.path.basename(lib_path)}: {per}"
    return rows
