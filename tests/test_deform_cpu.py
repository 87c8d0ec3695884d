"""neb_gi_update_vertices (deforming submeshes, the tree refitted in place) at the C-ABI boundary: what holds without a GPU."""
import ctypes as C
import os
import re
import subprocess

from nebulae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "neb_gi_update_vertices"
FIELDS = ("geometry", "firstVertex", "numVertices", "positions", "positionStride", "normals", "normalStride", "tangents", "tangentStride")


def test_the_header_declares_the_call_and_documents_it():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    m = re.search(r"int\s+neb_gi_update_vertices\s*\(\s*neb_ctx\*\s*ctx,\s*const neb_vertex_update\*\s*updates,\s*uint32_t n,\s*neb_stream stream\)\s*;", text)
    assert m, "declaration missing or changed"
    doc = text[:text.index("typedef struct neb_vertex_update {")].rsplit("/*", 1)[1]  # the comment above the entry struct and the call
    for word in ("NO reference counterpart", "ALLOW_UPDATE", "NEB_ERR_STATE", "NEB_ERR_INVALID_ARG", "NEB_ERR_OUT_OF_RANGE", "svgf_motion", "Streams"):
        assert word in doc, word
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    assert NAME in mirror


def test_the_binding_exports_it():
    assert NAME in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, NAME)


def test_the_ctypes_mirror_of_the_update_entry_has_the_layout_of_the_c_struct(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\n'
                   "int main(void) { printf(\"%zu\", sizeof(neb_vertex_update));\n"
                   + "".join(f' printf(" %zu", offsetof(neb_vertex_update, {f}));\n' for f in FIELDS) + " return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert [f for f, _ in _lib.VertexUpdate._fields_] == list(FIELDS)
    assert got == [C.sizeof(_lib.VertexUpdate)] + [getattr(_lib.VertexUpdate, f).offset for f in FIELDS]


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    p = (C.c_float * 3)(0.0, 0.0, 0.0)
    u = _lib.VertexUpdate(geometry=0, firstVertex=0, numVertices=1, positions=C.addressof(p), positionStride=12)
    assert lib.neb_gi_update_vertices(None, C.byref(u), 1, None) == -1
    assert lib.neb_gi_update_vertices(None, None, 0, None) == -1
