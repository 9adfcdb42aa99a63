"""Host tests of the header reader (madm_amd/_cabi.py) and of what _lib.py / _lib_data.py bind from it: the parser on
literal snippets, one per construct and one per refusal; the struct layouts against the C compiler; a few signatures
written out in full, so that a parser bug cannot hide behind "the binding equals the parse"; the one loader (_cabi.load)
against the four built libraries."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint, c_ulonglong, c_void_p

import pytest

from madm_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(tmp_path, text):
    p = tmp_path / "snippet.h"
    p.write_text(text)
    return _cabi.parse(str(p))


# ---- 1. the parser, construct by construct ---------------------------------------------------------------------------------

def test_multi_line_prototype_with_a_comment_between_arguments(tmp_path):
    abi = _parse(tmp_path, "int f(int a,   /* first */\n"
                           "      float b,   // second, with a ; and a ( in it\n"
                           "      void* stream);\n")
    assert abi.prototypes == [("f", c_int, [("a", c_int), ("b", c_float), ("stream", c_void_p)])]
    assert abi.symbols() == [("f", c_int, [c_int, c_float, c_void_p])]


def test_const_pointers_and_several_declarators_after_one_type(tmp_path):
    abi = _parse(tmp_path, "typedef struct {\n    const void *in1, *in2;\n    int C1, C2;\n    const float* bias; float *p , q;\n} s_t;\n"
                           "int f(const s_t* a, const void* x, void *y);\n")
    assert abi.struct("s_t")._fields_ == [("in1", c_void_p), ("in2", c_void_p), ("C1", c_int), ("C2", c_int), ("bias", c_void_p),
                                          ("p", c_void_p), ("q", c_float)]
    assert abi.struct("s_t").__name__ == "s_t" and issubclass(abi.struct("s_t"), ctypes.Structure)
    assert abi.prototypes == [("f", c_int, [("a", POINTER(abi.struct("s_t"))), ("x", c_void_p), ("y", c_void_p)])]


def test_unsigned_and_unsigned_long_long(tmp_path):
    abi = _parse(tmp_path, "int f(unsigned pattern, unsigned long long base, unsigned long long* fp, unsigned* u, const unsigned char* pal);\n")
    assert abi.symbols() == [("f", c_int, [c_uint, c_ulonglong, c_void_p, c_void_p, c_void_p])]


def test_size_t_and_fixed_width_pointers(tmp_path):
    abi = _parse(tmp_path, "size_t f(size_t n, const int64_t* ids, int32_t* hist, const uint8_t* src, double count, double* out);\n")
    assert abi.symbols() == [("f", c_size_t, [c_size_t, c_void_p, c_void_p, c_void_p, c_double, c_void_p])]


def test_void_argument_list_and_the_two_special_returns(tmp_path):
    abi = _parse(tmp_path, "int version(void);\nconst char* last_error(void);\nvoid set_tile(int tile);\nint g( void );\n")
    assert abi.symbols() == [("version", c_int, []), ("last_error", c_char_p, []), ("set_tile", None, [c_int]), ("g", c_int, [])]


def test_a_char_pointer_argument_is_an_ordinary_pointer(tmp_path):
    assert _parse(tmp_path, "int f(const char* name);\n").symbols() == [("f", c_int, [c_void_p])]


def test_constants_from_defines_and_enums_with_negative_values(tmp_path):
    abi = _parse(tmp_path, "#ifndef GUARD_H\n#define GUARD_H\n#include <stddef.h>\n#pragma once\n"
                           "#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
                           "#define ABI_VERSION 6\n#define MAX_TAPS 17   /* widest */\n#define MASK 0x7f\n"
                           "typedef enum {\n    OK = 0,\n    ERR_ARG = -1,   /* why */\n    ERR_LAUNCH = -3\n} status;\n"
                           "typedef enum { A = 0, B = 1, } kind;\n"
                           "#ifdef __cplusplus\n}\n#endif\n#endif /* GUARD_H */\n")
    assert abi.constants == {"ABI_VERSION": 6, "MAX_TAPS": 17, "MASK": 127, "OK": 0, "ERR_ARG": -1, "ERR_LAUNCH": -3, "A": 0, "B": 1}
    assert abi.structs == {} and abi.prototypes == []


REFUSED = {
    "unknown type name": ("int f(int a);\nint g(int a,\n      madm_dtype b);\n", 3),
    "unknown pointee": ("int f(int a);\nint g(const half* x);\n", 2),
    "array declarator": ("typedef struct {\n    int a;\n    int taps[17];\n} s_t;\n", 3),
    "array parameter": ("int f(float w[9]);\n", 1),
    "function pointer": ("typedef struct {\n    int (*cb)(int);\n} s_t;\n", 2),
    "function pointer parameter": ("\n\nint f(void (*cb)(void*), void* stream);\n", 3),
    "bit-field": ("typedef struct {\n    int a;\n    unsigned flag : 1;\n} s_t;\n", 3),
    "variadic": ("int f(const char* fmt, ...);\n", 1),
    "struct pointer before its struct": ("int f(const s_t* a);\ntypedef struct { int x; } s_t;\n", 1),
    "struct by value": ("typedef struct { int x; } s_t;\nint f(s_t a);\n", 2),
    "pointer to pointer": ("int f(void** out);\n", 1),
    "unnamed parameter": ("int f(int, float);\n", 1),
    "empty argument list": ("int f();\n", 1),
    "enumerator without a value": ("typedef enum {\n    A = 0,\n    B\n} kind;\n", 3),
    "tagged struct": ("struct s { int x; };\n", 1),
    "nested struct": ("typedef struct {\n    struct { int x; } in;\n} s_t;\n", 2),
    "macro with a non-integer value": ("#define N 4\n#define M (N + 1)\n", 2),
    "conditional compilation": ("#if defined(FOO)\nint f(void);\n#endif\n", 1),
    "unterminated declaration": ("int f(void);\nint g(void)\n", 2),
    "int by another name": ("int f(long n);\n", 1),
}


@pytest.mark.parametrize("what", list(REFUSED), ids=[w.replace(" ", "_") for w in REFUSED])
def test_what_the_headers_do_not_use_is_refused_with_its_line(tmp_path, what):
    text, line = REFUSED[what]
    with pytest.raises(_cabi.HeaderError, match=rf"snippet\.h:{line}: "):
        _parse(tmp_path, text)


def test_a_missing_header_is_an_import_error_that_names_the_path():
    with pytest.raises(ImportError, match=r"include.no_such_header\.h not found"):
        _cabi.parse_packaged("no_such_header.h")


# ---- 2. the two real headers -----------------------------------------------------------------------------------------------

def test_the_headers_parse_to_the_counts_they_hold():
    a, d = _cabi.parse_packaged("madm_hip.h"), _cabi.parse_packaged("madm_data.h")
    assert len(a.prototypes) == 83 and len({n for n, _r, _p in a.prototypes}) == 83
    assert {n: len(s._fields_) for n, s in a.structs.items()} == {
        "madm_conv2d_args": 48, "madm_conv2d_plan": 6, "madm_attention_args": 15, "madm_attention_bwd_args": 25,
        "madm_conv2d_wgrad_args": 24, "madm_vis_tile": 7}
    assert [n for n, _r, _p in d.prototypes] == ["mdata_abi_version", "mdata_last_error", "mdata_prep_image_u8", "mdata_prep_label_u8",
                                                 "mdata_png_unfilter"]
    assert d.structs == {}
    assert d.constants == {"MDATA_OK": 0, "MDATA_ERR_INVALID_ARG": 1, "MDATA_ERR_LAUNCH": 2, "MDATA_ERR_FORMAT": 3, "MDATA_MAX_TAPS": 17}


def test_signatures_written_out_in_full():
    """Six entry points of different shape, expected types typed here by hand from the header's text; compared with the
    parse AND with what the loaded function objects carry."""
    from madm_amd import _lib, _lib_data
    vp, f, i = c_void_p, c_float, c_int
    want = {
        "madm_conv2d_fwd": (c_int, [POINTER(_lib.Conv2dArgs), vp]),
        "madm_attention_bwd_workspace_bytes": (c_size_t, [POINTER(_lib.AttentionBwdArgs)]),
        "madm_adamw_step": (c_int, [vp, vp, vp, vp, c_size_t, f, f, f, f, f, i, f, vp]),
        "madm_snapshot_f32": (c_int, [vp, vp, c_size_t, c_ulonglong, vp, vp]),
        "madm_bn_fold_stats": (c_int, [vp, i, i, c_double, f, vp, vp, vp, vp]),
    }
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, (restype, argtypes) in want.items():
        assert table[name] == (restype, argtypes), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert {n: (r, a) for n, r, a in _lib_data.SYMBOLS}["mdata_png_unfilter"] == (c_int, [vp, c_size_t, vp, c_size_t, i, c_size_t, i])
    fn = _lib_data.lib.mdata_png_unfilter
    assert fn.restype is c_int and list(fn.argtypes) == [vp, c_size_t, vp, c_size_t, i, c_size_t, i]
    assert table["madm_last_error"] == (c_char_p, []) and table["madm_debug_set_conv_tile"] == (None, [c_int])
    # and two structs, field by field
    assert _lib.VisTile._fields_ == [("kind", i), ("src", vp), ("C", i), ("h", i), ("w", i), ("p0", f), ("p1", f)]
    assert _lib.Conv2dPlan._fields_ == [("tile", i), ("splitk", i), ("splitk_eff", i), ("post_gn", i), ("tuned_row", i),
                                        ("workspace_bytes", c_size_t)]
    assert (_lib.MADM_F32, _lib.MADM_BF16, _lib.MADM_F16, _lib.EPI_GEGLU, _lib.EPI_RELU, _lib.ACT_SILU, _lib.ACT_RELU) == (0, 1, 2, 1, 2, 1, 2)
    assert (_lib.VIS_IMAGE, _lib.VIS_LABEL, _lib.VIS_LOGITS, _lib.VIS_HEAT, _lib.VIS_MAX_TILES) == (0, 1, 2, 3, 16)
    assert (_lib.EXPORT_IMAGE_F32, _lib.EXPORT_IMAGE_U8, _lib.EPI_NONE, _lib.ACT_NONE, _lib_data.MAX_TAPS) == (0, 1, 0, 0, 17)


def test_the_poison_harness_wraps_what_takes_a_stream():
    """_PoisonedLib puts madm_debug_poison_lds in front of every entry point whose last parameter is ``stream``: the 70 that
    launch.  The rule it replaced (last argtype is a void pointer) selects the same set."""
    from madm_amd import _lib
    launching = _lib._PoisonedLib(None)._launching
    assert len(launching) == 70
    assert {"madm_conv2d_fwd", "madm_vis_compose", "madm_pack_weight", "madm_calib_mfma_loop"} <= launching
    assert not launching & {"madm_debug_poison_lds", "madm_debug_set_conv_tile", "madm_conv2d_make_plan", "madm_abi_version",
                            "madm_attention_bwd_workspace_bytes", "madm_mic_minmax_parts"}
    assert launching == {n for n, _r, a in _lib.SYMBOLS if a and a[-1] is c_void_p and not n.startswith("madm_debug")}


def test_a_library_of_another_abi_version_is_refused_at_import():
    """what _lib.py hands the loader, but for a header that declares version 7"""
    with pytest.raises(ImportError, match=r"ABI version 6, include/madm_hip.h declares 7: rebuild"):
        _load("hip", version=7)


# the loader (_cabi.load) against the four built libraries, with what each _lib*.py module hands it
class _Refused(RuntimeError):
    pass


LOADS = {
    "hip": dict(header="madm_hip.h", libname="libmadm_hip.so", env="MADM_HIP_LIB", version_fn="madm_abi_version",
                version="MADM_ABI_VERSION", version_from="include/madm_hip.h declares", last_error_fn="madm_last_error",
                error=_Refused, no_fallback="madm_amd has no CPU fallback"),
    "data": dict(header="madm_data.h", libname="libmadm_data.so", env="MADM_DATA_LIB", version_fn="mdata_abi_version",
                 version=1, last_error_fn="mdata_last_error", error=_Refused, no_fallback="the dataset pipeline has no CPU fallback"),
    "det": dict(header="madm_det.h", libname="libmadm_det.so", env="MADM_DET_LIB", version_fn="mdet_abi_version",
                version=1, last_error_fn="mdet_last_error", error=_Refused, no_fallback="the deterministic mode has no fallback"),
    "headfuse": dict(header="madm_headfuse.h", libname="libmadm_headfuse.so", env="MADM_HEADFUSE_LIB", version_fn="mhf_abi_version",
                     version=1, last_error_fn="mhf_last_error", error=_Refused, no_fallback="the fused classifier has no fallback"),
}


def _load(which, **change):
    """as the binding module does: the override is what its environment variable holds"""
    kw = dict(LOADS[which], **change)
    return _cabi.load(override=os.environ.get(kw.pop("env")), **kw)


def _comparable(t):
    """a ctypes type as something two parses of one header agree on: each parse makes its own struct classes"""
    if isinstance(getattr(t, "_type_", None), type) and issubclass(t._type_, ctypes.Structure):
        return ("pointer to", t._type_.__name__, [(n, _comparable(f)) for n, f in t._type_._fields_])
    return t


@pytest.mark.parametrize("which", list(LOADS))
def test_loader_returns_the_headers_symbols_bound(which):
    kw = LOADS[which]
    b = _load(which)
    fresh = _cabi.parse(os.path.join(ROOT, "include", kw["header"])).symbols()
    norm = lambda syms: [(n, r, [_comparable(a) for a in args]) for n, r, args in syms]      # noqa: E731
    assert b.SYMBOLS == b.ABI.symbols() and norm(b.SYMBOLS) == norm(fresh) and len(fresh) >= 3
    assert b.LIB_PATH == (os.environ.get(kw["env"]) or os.path.join(ROOT, "madm_amd", kw["libname"]))
    for name, restype, argtypes in b.SYMBOLS:
        fn = getattr(b.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert b.check(0, "nothing") is None and isinstance(b.last_error(), str)
    with pytest.raises(_Refused, match=r"^some call failed \(status 3\): "):
        b.check(3, "some call")


@pytest.mark.parametrize("which", list(LOADS))
def test_loader_refuses_another_abi_version(which):
    kw = LOADS[which]
    have = getattr(_load(which).lib, kw["version_fn"])()
    with pytest.raises(ImportError, match=rf"{kw['libname']} has ABI version {have}, .* {have + 1}: rebuild$"):
        _load(which, version=have + 1)


@pytest.mark.parametrize("which", list(LOADS))
def test_loader_names_a_missing_file_and_the_make_line(which, tmp_path, monkeypatch):
    kw = LOADS[which]
    missing = str(tmp_path / "nowhere" / kw["libname"])
    monkeypatch.setenv(kw["env"], missing)
    with pytest.raises(ImportError) as e:
        _load(which)
    csrc = os.path.join(ROOT, "madm_amd", "csrc")
    assert str(e.value) == f"{missing} not found: build it with `make -C {csrc}` (or __graft_entry__.build()); {kw['no_fallback']}"


# ---- 3. struct layouts: the ctypes classes against the compiler that built the library ----------------------------------------

C_NAME = {c_int: "int", c_uint: "unsigned", c_ulonglong: "unsigned long long", c_float: "float", c_double: "double", c_size_t: "size_t"}


def _layout_asserts(name, cls):
    """C11 static assertions that ``name`` of the headers is laid out like the ctypes class: size of the struct; offset, size
    and -- for scalars -- the type itself of every field (an int is not a float of the same width)."""
    out = [f'_Static_assert(sizeof({name}) == {ctypes.sizeof(cls)}, "sizeof {name}");']
    for field, ctype in cls._fields_:
        d = getattr(cls, field)
        out.append(f'_Static_assert(offsetof({name}, {field}) == {d.offset}, "offsetof {name}.{field}");')
        out.append(f'_Static_assert(sizeof((({name}*)0)->{field}) == {d.size}, "sizeof {name}.{field}");')
        if ctype is not c_void_p:
            out.append(f'_Static_assert(_Generic((({name}*)0)->{field}, {C_NAME[ctype]}: 1, default: 0), "type of {name}.{field}");')
    return out


def _compiler_accepts(tmp_path, lines):
    makefile = open(os.path.join(ROOT, "madm_amd", "csrc", "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)$", makefile, flags=re.M).group(1)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "madm_hip.h"\n#include "madm_data.h"\n' + "\n".join(lines) + "\n")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode == 0, r.stdout


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = {**_cabi.parse_packaged("madm_hip.h").structs, **_cabi.parse_packaged("madm_data.h").structs}
    assert len(structs) == 6
    lines = [ln for name, cls in structs.items() for ln in _layout_asserts(name, cls)]
    assert len(lines) >= 6 + 2 * 125      # 125 fields in all: offset and size of each, the type of the scalars
    ok, log = _compiler_accepts(tmp_path, lines)
    assert ok, log
    assert ctypes.sizeof(structs["madm_vis_tile"]) == 40      # what madm_vis_compose's kernel-argument table is sized by

    # the check can fail: a size_t bound as an int, and two swapped fields of one width
    class Narrow(ctypes.Structure):
        _fields_ = [(n, c_int) for n in ("tile", "splitk", "splitk_eff", "post_gn", "tuned_row", "workspace_bytes")]

    class Swapped(ctypes.Structure):
        _fields_ = [("kind", c_int), ("src", c_void_p), ("C", c_int), ("w", c_int), ("h", c_int), ("p0", c_float), ("p1", c_float)]

    class IntForFloat(ctypes.Structure):
        _fields_ = [("kind", c_int), ("src", c_void_p), ("C", c_int), ("h", c_int), ("w", c_int), ("p0", c_int), ("p1", c_float)]

    ok, log = _compiler_accepts(tmp_path, _layout_asserts("madm_conv2d_plan", Narrow) + _layout_asserts("madm_vis_tile", Swapped)
                                + _layout_asserts("madm_vis_tile", IntForFloat))
    assert not ok
    for message in ("sizeof madm_conv2d_plan.workspace_bytes", "sizeof madm_conv2d_plan\"", "offsetof madm_vis_tile.w", "offsetof madm_vis_tile.h",
                    "type of madm_vis_tile.p0"):
        assert message in log, (message, log)
    assert "madm_vis_tile.kind" not in log and "madm_conv2d_plan.tile" not in log
