"""The key directory's C ABI (no GPU): include/fdx.h declares the fdx_keydir_* entry points,
libfdx.so exports them with the ctypes signatures, and the arguments the header rules out are
FDX_E_INVALID before any HIP call."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("fdx_keydir_create", "fdx_keydir_destroy", "fdx_keydir_reset", "fdx_keydir_memory", "fdx_keydir_map",
         "fdx_keydir_counts", "fdx_keydir_keys", "fdx_keydir_load")


def test_header_declares_and_library_exports_the_entry_points():
    from fdx import _lib

    src = open(os.path.join(ROOT, "include", "fdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert "typedef struct fdx_keydir_s *fdx_keydir;" in code
    assert re.search(r"#define\s+FDX_KEYDIR_INSERT\s+1\b", code) and _lib.FDX_KEYDIR_INSERT == 1
    # the documented contract: numbering rule, reserved key, refusals
    for word in ("pandas.factorize", "INT64_MIN", "first occurrence".upper(), "status bit 4"):
        assert word in src, word


def test_invalid_arguments_return_without_a_gpu():
    from fdx import _lib

    L = _lib.load()
    h = ctypes.c_void_p()
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced
    c4 = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64()
    sz = ctypes.c_size_t()
    cases = [
        lambda: L.fdx_keydir_create(16, 16, None, None),                    # null out
        lambda: L.fdx_keydir_create(0, 16, ctypes.byref(h), None),          # capacity < 1
        lambda: L.fdx_keydir_create(-5, 16, ctypes.byref(h), None),
        lambda: L.fdx_keydir_create((1 << 30) + 1, 16, ctypes.byref(h), None),  # capacity > 2^30
        lambda: L.fdx_keydir_create(16, 0, ctypes.byref(h), None),          # max_batch < 1
        lambda: L.fdx_keydir_reset(None, None),
        lambda: L.fdx_keydir_memory(None, ctypes.byref(sz)),
        lambda: L.fdx_keydir_map(None, dummy, 4, 1, dummy, None),
        lambda: L.fdx_keydir_map(None, dummy, -1, 1, dummy, None),
        lambda: L.fdx_keydir_counts(None, c4, None),
        lambda: L.fdx_keydir_keys(None, dummy, 4, ctypes.byref(n), None),
        lambda: L.fdx_keydir_load(None, dummy, 4, None),
    ]
    for i, call in enumerate(cases):
        L.fdx_time_flags(None, -1, 0, None, None, None)  # (another message: the one below is this call's)
        assert call() == -1, (i, L.fdx_last_error())
        assert h.value is None
    assert b"capacity" in (L.fdx_keydir_create(0, 16, ctypes.byref(h), None), L.fdx_last_error())[1]
    assert L.fdx_keydir_destroy(None) == 0
