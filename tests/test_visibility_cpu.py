"""neb_gi_set_visibility / neb_gi_get_visibility (submeshes hidden and shown in place, the tree kept) at the C-ABI boundary: what holds
without a GPU."""
import ctypes as C
import os
import re

from nebulae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("neb_gi_set_visibility", "neb_gi_get_visibility")


def test_the_header_declares_both_calls_and_documents_them():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    m = re.search(r"int\s+neb_gi_set_visibility\s*\(\s*neb_ctx\*\s*ctx,\s*const uint32_t\*\s*geometry_indices,\s*const uint8_t\*\s*visible[^)]*"
                  r"uint32_t n,\s*neb_stream stream\)\s*;", text)
    assert m, "declaration missing or changed"
    doc = text[:m.start()].rsplit("/*", 1)[1]  # the comment right above the declaration
    for word in ("InstanceMask", "PERFORM_UPDATE", "NEB_ERR_STATE", "NEB_ERR_INVALID_ARG", "NEB_ERR_OUT_OF_RANGE", "Sun table", "Streams"):
        assert word in doc, word
    assert re.search(r"int\s+neb_gi_get_visibility\s*\(\s*const neb_ctx\*\s*ctx,\s*uint8_t\*\s*out,\s*uint32_t capacity,\s*uint32_t\*\s*n_out\)\s*;", text)
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in mirror, name
        assert name in guide, name


def test_the_binding_exports_them():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)
    sigs = _lib._gi_sigs()
    assert sigs["neb_gi_set_visibility"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_uint32, C.c_void_p])
    assert sigs["neb_gi_get_visibility"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)])


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    idx, vis, n = (C.c_uint32 * 1)(0), (C.c_uint8 * 1)(0), C.c_uint32(7)
    assert lib.neb_gi_set_visibility(None, idx, vis, 1, None) == -1
    assert lib.neb_gi_set_visibility(None, None, None, 0, None) == -1
    assert lib.neb_gi_get_visibility(None, vis, 1, C.byref(n)) == -1
    assert lib.neb_gi_get_visibility(None, None, 0, None) == -1
    assert n.value == 7 and vis[0] == 0  # nothing was written
