"""neb_gi_update_vertices_device, neb_gi_update_status, neb_gi_scene_box at the C-ABI boundary: what holds without a GPU."""
import ctypes as C
import os
import re
import subprocess

from nebulae_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("neb_gi_update_vertices_device", "neb_gi_update_status", "neb_gi_scene_box")


def test_the_header_declares_the_three_calls_and_documents_them():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    decls = (r"int\s+neb_gi_update_vertices_device\s*\(\s*neb_ctx\*\s*ctx,\s*const neb_vertex_update\*\s*updates,\s*uint32_t n,\s*neb_stream stream\)\s*;",
             r"int\s+neb_gi_update_status\s*\(\s*neb_ctx\*\s*ctx,\s*uint64_t out\[2\]\)\s*;",
             r"int\s+neb_gi_scene_box\s*\(\s*neb_ctx\*\s*ctx,\s*float lo\[3\],\s*float hi\[3\]\)\s*;")
    for name, pattern in zip(NAMES, decls):
        m = re.search(pattern, text)
        assert m, f"{name}: declaration missing or changed"
        doc = text[:m.start()].rsplit("/*", 1)[1]  # the comment right above the declaration
        assert "*/" in doc and doc.rstrip().endswith("*/") and len(doc) > 150, name
    doc = text[:re.search(decls[0], text).start()].rsplit("/*", 1)[1]
    for word in ("DEVICE pointers", "stream order", "alive", "multiple of 4", "hipPointerGetAttributes", "neb_gi_update_status", "NEB_ERR_INVALID_ARG",
                 "refuses the WHOLE call", "neb_gi_build_bvh"):
        assert word in doc, word
    # the entry struct is shared with neb_gi_update_vertices: one definition, before both calls
    assert text.count("typedef struct neb_vertex_update {") == 1
    assert text.index("typedef struct neb_vertex_update {") < text.index("int neb_gi_update_vertices(") < text.index("int neb_gi_update_vertices_device(")


def test_the_bindings_export_them_with_the_signatures_of_the_header():
    sigs = _lib._gi_sigs()
    update = sigs["neb_gi_update_vertices"]
    assert sigs["neb_gi_update_vertices_device"][0] is C.c_int and sigs["neb_gi_update_vertices_device"][1] == update[1]  # the same entries, the same stream
    assert sigs["neb_gi_update_status"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    assert sigs["neb_gi_scene_box"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)])
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.exported_symbols(), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(sigs[name][1]), name


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    u = _lib.VertexUpdate(geometry=0, firstVertex=0, numVertices=1, positions=16, positionStride=12)  # (never dereferenced)
    assert lib.neb_gi_update_vertices_device(None, C.byref(u), 1, None) == -1
    assert lib.neb_gi_update_vertices_device(None, None, 0, None) == -1
    out, lo, hi = (C.c_uint64 * 2)(), (C.c_float * 3)(), (C.c_float * 3)()
    assert lib.neb_gi_update_status(None, out) == -1
    assert lib.neb_gi_scene_box(None, lo, hi) == -1


def test_the_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    """as tests/test_abi.py compiles include/nebulae_hip.hpp: here a translation unit that CALLS the three new methods"""
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror, name
    src = tmp_path / "use.cpp"
    src.write_text('#include "nebulae_hip.hpp"\n'
                   'static void use(Neb::GIPathtracer& g, const neb_vertex_update* u, neb_stream s)\n'
                   '{ uint64_t st[2]; float lo[3], hi[3]; g.UpdateVerticesDevice(u, 1, s); g.UpdateStatus(st); g.SceneBox(lo, hi); }\n'
                   'int main(int argc, char**) { Neb::SVGFDenoiser d; Neb::GIPathtracer g(d);\n'
                   '  if (argc > 7) use(g, nullptr, nullptr);\n'
                   '  try { d.Init(0, 0); } catch (const Neb::NebException& e) { return e.Status == NEB_ERR_INVALID_ARG ? 0 : 2; }\n'
                   '  return 1; }\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(build.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lnebulae_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([str(exe)]) == 0
