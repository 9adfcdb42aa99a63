"""Reader of the C ABI headers (include/madm_hip.h, madm_data.h, madm_det.h, madm_headfuse.h, madm_wslab.h): the ctypes structures,
signatures and constants that ``_lib.py`` / ``_lib_data.py`` / ``_lib_det.py`` / ``_lib_headfuse.py`` / ``_lib_wslab.py`` bind come from the text
every ``.hip`` file is compiled against, not from a table kept next to it.  Standard library only: no torch; ``parse``
loads no library (tools/conv_plan_fixture.py and the host tests use it on their own), ``load`` at the end is the one
loader the binding modules share.

It reads the C these headers are written in and refuses the rest with the header's line (``HeaderError``), never
guessing a type: ``#define NAME <integer>``; ``typedef enum { NAME = <integer>, ... } name;``; ``typedef struct { ... }
name;`` with scalar and pointer fields (several names after one type allowed); prototypes.  Scalars by value: int,
unsigned, unsigned long long, float, double, size_t.  A pointer to a struct declared above it is ``POINTER(struct)``, a
``const char*`` RETURN is ``c_char_p``, a ``void`` return is ``None``, every other pointer to a known scalar type is
``c_void_p`` (``void* stream`` included).  Arrays, function pointers, bit-fields, ``...``, pointers to pointers, unnamed
parameters, unknown type names and pointers to structs not seen yet are errors.
"""
import ctypes
import os
import re
import types

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "int32_t", "int64_t", "uint8_t"}
_INT = r"-?(?:0[xX][0-9a-fA-F]+|0|[1-9]\d*)"


class HeaderError(ValueError):
    pass


class Abi:
    """constants {name: int}, structs {name: ctypes.Structure subclass}, prototypes [(name, restype, [(param, ctype)])]"""

    def __init__(self, path):
        self.path, self.constants, self.structs, self.prototypes = path, {}, {}, []

    def struct(self, name):
        return self.structs[name]

    def symbols(self):
        """[(name, restype, argtypes)]: what a ctypes function object takes"""
        return [(name, restype, [t for _p, t in params]) for name, restype, params in self.prototypes]


def parse(path):
    with open(path) as f:
        text = f.read()
    abi = Abi(path)

    def fail(off, msg):
        raise HeaderError(f"{path}:{text.count(chr(10), 0, off) + 1}: {msg}")

    def blank(m):   # what is cut out leaves its newlines behind: an offset into the text still tells the header's line
        return "\n" * m.group().count("\n")

    def pieces(s, off, sep=None):
        """the non-blank parts of s between separators (None: s itself), stripped, each with the offset of its first character"""
        for part in (s.split(sep) if sep else [s]):
            if part.strip():
                yield part.strip(), off + len(part) - len(part.lstrip())
            off += len(part) + 1

    def directive(m):
        line = m.group().strip()
        d = line[1:].split()
        if d[:1] == ["define"] and len(d) == 3 and re.fullmatch(_INT, d[2]):
            abi.constants[d[1]] = int(d[2], 0)
        elif not (d[:1] in (["include"], ["pragma"], ["ifndef"], ["endif"]) or (d[:1] == ["define"] and len(d) == 2)) \
                or line.endswith("\\"):
            fail(m.start(), f"unsupported directive {line!r}")
        return ""

    def declare(s, off, ret=False):
        """'const T *a, *b' -> [(a, ctype), (b, ctype)]"""
        bad = re.search(r"[^\w\s*,]", s)
        if bad:
            fail(off, f"unsupported declarator ({bad.group()!r}) in {s!r}")
        out, base = [], None
        for i, d in enumerate(s.split(",")):
            tok = re.findall(r"\w+|\*", d)
            rest = [t for t in tok[:-1] if t not in ("*", "const")]
            if not tok or not re.fullmatch(r"[A-Za-z_]\w*", tok[-1]) or tok[-1] == "const" or (i and rest):
                fail(off, f"no declarator name in {s!r}")
            base, stars = (base if i else " ".join(rest)), tok.count("*")
            if stars > 1:
                fail(off, f"pointer to pointer in {s!r}")
            if stars and base in abi.structs:
                t = ctypes.POINTER(abi.structs[base])
            elif stars and base == "char" and ret:
                t = ctypes.c_char_p
            elif stars and base in _POINTEES:
                t = ctypes.c_void_p
            elif stars:
                fail(off, f"pointer to unknown type {base!r} in {s!r} (a struct is declared above its first use)")
            elif base == "void" and ret:
                t = None
            elif base in _SCALARS:
                t = _SCALARS[base]
            else:
                fail(off, f"unknown type {base!r} in {s!r}")
            out.append((tok[-1], t))
        return out

    def statement(s, off):
        m = re.fullmatch(r"typedef\s+(enum|struct)\s*\{(.*)\}\s*(\w+)", s, flags=re.S)
        if m and m[1] == "enum":
            for item, ioff in pieces(m[2], off + m.start(2), ","):
                e = re.fullmatch(rf"(\w+)\s*=\s*({_INT})", item)
                if not e:
                    fail(ioff, f"enumerator without an integer value: {item!r}")
                abi.constants[e[1]] = int(e[2], 0)
        elif m:
            fields = [f for decl, doff in pieces(m[2], off + m.start(2), ";") for f in declare(decl, doff)]
            abi.structs[m[3]] = type(m[3], (ctypes.Structure,), {"_fields_": fields})
        else:
            m = re.fullmatch(r"([^()]*)\((.*)\)", s, flags=re.S)
            if not m:
                fail(off, f"neither a typedef'd struct / enum nor a prototype: {s.split(chr(10))[0]!r}")
            if "," in m[1] or not m[2].strip():
                fail(off, f"unsupported prototype (several names, or () instead of (void)): {s.split(chr(10))[0]!r}")
            (name, restype), = declare(m[1], off, ret=True)
            params = "" if m[2].strip() == "void" else m[2]
            abi.prototypes.append((name, restype, [declare(p, poff)[0] for p, poff in pieces(params, off + m.start(2), ",")]))

    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b", blank, text, flags=re.S | re.M)   # extern "C"
    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    depth = start = 0
    for m in re.finditer(r"[{};]", text):
        depth += {"{": 1, "}": -1, ";": 0}[m.group()]
        if m.group() == ";" and depth == 0:
            for s, off in pieces(text[start:m.start()], start):
                statement(s, off)
            start = m.end()
    for s, off in pieces(text[start:], start):
        fail(off, "unterminated declaration")
    return abi


def parse_packaged(name):
    """include/<name> of the tree this package lies in, as the binding modules read it; ImportError when it is missing"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", name)
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: the ctypes binding of the library is read from this header")
    return parse(path)


def load(header, libname, override, version_fn, version, last_error_fn, error, no_fallback, version_from="this binding is for"):
    """The one loader behind ``_lib.py``, ``_lib_data.py``, ``_lib_det.py``, ``_lib_headfuse.py`` and ``_lib_wslab.py``: binds madm_amd/<libname>,
    or the file ``override`` names (what the module's MADM_*_LIB environment variable holds), from include/<header>.  Returns a
    namespace of ABI (the parsed header), SYMBOLS (``ABI.symbols()``), LIB_PATH, lib (every declared symbol typed),
    last_error() and check(rc, what), which raises ``error`` with the library's text on a non-zero status.  ``version`` is
    what ``version_fn`` must return: an integer, or the name of the header's constant that holds it.  ImportError when the
    file is missing (names the path and the make line, ends with ``no_fallback``) or of another ABI version ("rebuild");
    AttributeError when a declared symbol is not exported."""
    here = os.path.dirname(os.path.abspath(__file__))
    abi = parse_packaged(header)
    path = override or os.path.join(here, libname)
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `make -C {os.path.join(here, 'csrc')}` "
                          f"(or __graft_entry__.build()); {no_fallback}")
    lib = ctypes.CDLL(path)
    for name, restype, argtypes in abi.symbols():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    want, got = (version if isinstance(version, int) else abi.constants[version]), getattr(lib, version_fn)()
    if got != want:
        raise ImportError(f"{path} has ABI version {got}, {version_from} {want}: rebuild")

    def last_error():
        return getattr(lib, last_error_fn)().decode("utf-8", "replace")

    def check(rc, what):
        if rc != 0:
            raise error(f"{what} failed (status {rc}): {last_error()}")

    return types.SimpleNamespace(ABI=abi, SYMBOLS=abi.symbols(), LIB_PATH=path, lib=lib, last_error=last_error, check=check)
