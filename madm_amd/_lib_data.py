"""ctypes binding of libmadm_data.so (the C ABI declared in include/madm_data.h): the dataset pipeline's kernels and the
PNG reader's unfilter loop.  Loaded by ``madm_amd/data.py`` and ``madm_amd/png_read.py`` only -- importing the package does
not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` there is no fallback: a missing library or
symbol raises on import."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADM_DATA_LIB") or os.path.join(_HERE, "libmadm_data.so")

MDATA_OK, MDATA_ERR_INVALID_ARG, MDATA_ERR_LAUNCH, MDATA_ERR_FORMAT = 0, 1, 2, 3
MAX_TAPS = 17
ABI_VERSION = 1

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t

# every symbol include/madm_data.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("mdata_abi_version", c_int, []),
    ("mdata_last_error", ctypes.c_char_p, []),
    ("mdata_prep_image_u8", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    ("mdata_prep_label_u8", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    ("mdata_png_unfilter", c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_size_t, c_int]),
]


class MadmDataError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or __graft_entry__.build()); the dataset pipeline has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mdata_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.mdata_abi_version()}, this binding is for {ABI_VERSION}: rebuild")
    return lib


lib = _load()


def last_error():
    return lib.mdata_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise MadmDataError(f"{what} failed (status {rc}): {last_error()}")
