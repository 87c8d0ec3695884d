"""neb_gi_update_transforms (moving submeshes, the tree refitted in place) at the C-ABI boundary: what holds without a GPU."""
import ctypes as C
import os
import re

from nebulae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "neb_gi_update_transforms"


def test_the_header_declares_the_call_and_documents_it():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    m = re.search(r"int\s+neb_gi_update_transforms\s*\(\s*neb_ctx\*\s*ctx,\s*const uint32_t\*\s*geometry_indices,\s*const float\*\s*surfaceToWorld[^)]*"
                  r"uint32_t n,\s*neb_stream stream\)\s*;", text)
    assert m, "declaration missing or changed"
    doc = text[:m.start()].rsplit("/*", 1)[1]  # the comment right above the declaration
    for word in ("CreateTlas", "NEB_ERR_STATE", "NEB_ERR_INVALID_ARG", "NEB_ERR_OUT_OF_RANGE", "Sun table", "Streams"):
        assert word in doc, word
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    assert NAME in mirror


def test_the_binding_exports_it():
    assert NAME in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, NAME)


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    idx = (C.c_uint32 * 1)(0)
    m = (C.c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    assert lib.neb_gi_update_transforms(None, idx, m, 1, None) == -1
    assert lib.neb_gi_update_transforms(None, None, None, 0, None) == -1
