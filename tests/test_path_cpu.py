"""neb_gi_trace_paths: what holds without a GPU -- the two records and the bindings' view of them, trace32's records
under the judge of tests/path_ref.py, the calibration its tolerances are derived from, the judge shown able to fail, and that the ray
sets reach every kind of vertex the GPU tests are meant to judge."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import path_ref as P
import ray_query_ref as Q
import ray_shade_ref as R
from nebulae_amd import _lib, build
from nebulae_amd import scene as S
from oracle import gi_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
K = 8


# ------------------------------------------------------------------------------------------------
# 1: ABI
# ------------------------------------------------------------------------------------------------
def test_the_records_have_the_sizes_and_offsets_the_bindings_assume(tmp_path):
    fields = {"neb_ray_path": ("r", "t", "geometry", "primitive", "flags", "segments"),
              "neb_path_vertex": ("origin", "tmin", "direction", "t", "throughput", "rng", "added", "flags", "geometry", "primitive", "u", "v", "tmax", "pdiff",
                                  "reserved")}
    lines = "".join(f'  printf("{s} %zu", sizeof({s}));' + "".join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                    for s, fs in fields.items())
    lines += '  printf("%u %u\\n", NEB_PATH_ESCAPED, NEB_PATH_DIVIDED);\n'
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\nint main(void) {\n' + lines + "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    path, vertex = ([int(w) for w in out[k].split()[1:]] for k in (0, 1))
    assert path == [32, 0, 12, 16, 20, 24, 28], path
    assert vertex == [96, 0, 12, 16, 28, 32, 44, 48, 60, 64, 68, 72, 76, 80, 84, 88], vertex
    assert [P.PATH.fields[k][1] for k in P.PATH.names] == path[1:] and [P.VERTEX.fields[k][1] for k in P.VERTEX.names] == vertex[1:]
    assert [P.PATH.fields[k][1] for k in P.PATH.names[:5]] == [R.RADIANCE.fields[k][1] for k in R.RADIANCE.names[:5]]  # the layout of neb_ray_radiance
    assert [int(w) for w in out[2].split()] == [_lib.PATH_ESCAPED, _lib.PATH_DIVIDED] == [64, 128]


def test_the_library_exports_the_call_and_refuses_a_null_context_without_a_device(tmp_path):
    build.build()
    assert hasattr(C.CDLL(build.LIB_PATH), "neb_gi_trace_paths") and "neb_gi_trace_paths" in _lib.exported_symbols()
    assert _lib._gi_sigs()["neb_gi_trace_paths"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants), C.c_void_p,
                                                               C.c_void_p, C.c_void_p])
    lib = _lib.load()
    c = P.constants(3)
    assert lib.neb_gi_trace_paths(None, None, 0, 0, C.byref(c), None, None, None) == -1  # NEB_ERR_INVALID_ARG: a null context, no GPU touched
    src = tmp_path / "use.cpp"
    src.write_text('#include "nebulae_hip.hpp"\n'
                   'static void use(Neb::GIPathtracer& g, const neb_ray* r, const neb_gi_constants* c, neb_ray_path* a, neb_path_vertex* b, neb_stream s)\n'
                   '{ g.TracePaths(r, 1, 0, c, a, nullptr, s); g.TracePaths(r, 1, NEB_RAYS_SORT, c, a, b, s); }\n'
                   'int main(int argc, char**) { Neb::SVGFDenoiser d; Neb::GIPathtracer g(d);\n'
                   '  if (argc > 7) use(g, nullptr, nullptr, nullptr, nullptr, nullptr);\n'
                   '  try { d.Init(0, 0); } catch (const Neb::NebException& e) { return e.Status == NEB_ERR_INVALID_ARG ? 0 : 2; }\n'
                   '  return 1; }\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(build.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lnebulae_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([str(exe)]) == 0


# ------------------------------------------------------------------------------------------------
# the states and sets of the GPU tests, traced in float32 and judged: once, for every test below
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced():
    """{(state, set): dict(scene, tris, rays, c, out, vert, cast, shade, verdict)} for K = 8: trace32's records and what the judge says of them"""
    got = {}
    for state, (sc, hidden) in R.states().items():
        tris = Q.triangles(sc, hidden)
        sets = Q.ray_sets(*Q.scene_box(sc), tris)
        flat = gi_np.FlatScene(sc)
        cast, shade = P.cpu_cast(tris), P.cpu_shade(sc, tris, flat)
        for name in P.JUDGED_SETS:
            c = P.constants(K)
            out, vert = P.trace32(sc, tris, sets[name], c, flat)
            verdict = P.judge_vertices(sc, tris, sets[name], c, out, vert, cast, shade, f"trace32 / {state} / {name}")
            got[state, name] = dict(scene=sc, tris=tris, rays=sets[name], c=c, out=out, vert=vert, cast=cast, shade=shade, verdict=verdict)
    return got


def test_trace32_records_pass_the_judge(traced):
    """(the fixture has judged them: an assertion there fails every test of this file)  With K = 2 the records are the float32 reading
    ray_shade_ref's radiance judge takes."""
    assert len(traced) == 4 * len(P.JUDGED_SETS)
    for (state, name), t in traced.items():
        assert all(d <= P.TIE_CAP for d in t["verdict"]["differ"]) and t["verdict"]["live"][0] == len(t["rays"]), (state, name)
    t = traced["room, extras", "scattered"]
    c = P.constants(2)
    out, vert = P.trace32(t["scene"], t["tris"], t["rays"], c)
    assert vert.shape == (len(t["rays"]), 1) and (out["segments"] == 1).all()
    rec = np.zeros(len(out), R.RADIANCE)
    for k in ("radiance", "t", "geometry", "primitive"):
        rec[k] = out[k]
    rec["flags"] = out["flags"] & P.HIT_BITS
    R.judge_radiance(t["scene"], t["tris"], t["rays"], rec, c, "trace32 with K = 2 as radiance records")


def test_calibration(traced):
    """The largest error of each class of trace32's records under the judge, over every state and set the GPU tests judge, K = 8, is
    what path_ref.MEASURED says (TOL = 4 x)."""
    worst = {k: max(t["verdict"][k] for t in traced.values()) for k in P.CLASSES}
    print("[calibration] measured maxima: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    print("[calibration] constants:       " + ", ".join(f"{k} {P.MEASURED[k]:.3e}" for k in worst))
    for k, v in worst.items():
        assert v <= P.MEASURED[k], (k, v)
        assert P.MEASURED[k] <= 1.25 * v, f"{k}: the constant {P.MEASURED[k]:.3e} is not the measurement {v:.3e} rounded up"
        assert P.TOL[k] == 4.0 * P.MEASURED[k]


# ------------------------------------------------------------------------------------------------
# the judge fails what it should
# ------------------------------------------------------------------------------------------------
def test_the_judge_fails_each_corruption(traced):
    t = traced["room, extras", "scattered"]
    sc, tris, rays, c, out, vert = (t[k] for k in ("scene", "tris", "rays", "c", "out", "vert"))
    seg = out["segments"].astype(np.int64)
    flags = vert["flags"]

    def fails(bad_out, bad_vert, word):
        with pytest.raises(AssertionError, match=word):
            P.judge_vertices(sc, tris, rays, c, bad_out, bad_vert, t["cast"], t["shade"], "a record that is wrong")

    def resummed(bad_vert):
        o = out.copy()
        o["radiance"] = P.running_sum(bad_vert, seg)
        return o

    # rng advanced by two draws instead of three
    bad = vert.copy()
    i = int(np.flatnonzero(seg >= 3)[0])
    bad["rng"][i, 2] = P.draws(vert["rng"][i:i + 1, 1], 2)[1][0]
    fails(out, bad, "chain: rng")
    # throughput not divided where the flag says it was
    bad = vert.copy()
    m = (seg >= 2) & ((flags[:, 0] & _lib.PATH_DIVIDED) != 0) & (vert["throughput"][:, 1].max(-1) > 0.2)
    i = int(np.flatnonzero(m)[0])
    bad["throughput"][i, 1] = (vert["throughput"][i, 1] * vert["pdiff"][i, 0]).astype(F)
    fails(out, bad, "throughput off")
    # the next origin offset along SN instead of GN
    surf = t["shade"](rays)
    with np.errstate(all="ignore"):
        apart = np.abs(surf["shading_normal"] - surf["geometric_normal"]).max(-1)
    m = (seg >= 2) & (apart > 0.05)
    assert m.sum() >= 10, "no normal-mapped first hit to offset along"
    i = int(np.flatnonzero(m)[0])
    bad = vert.copy()
    bad["origin"][i, 1] = (surf["position"][i] + surf["shading_normal"][i] * F(1e-2)).astype(F)
    fails(out, bad, "origin off")
    # sky added without throughput (the sum follows, so that nothing else is wrong)
    bad = vert.copy()
    k_last = np.maximum(seg - 1, 0)
    escaped_late = (seg >= 2) & ((flags[np.arange(len(seg)), k_last] & _lib.HIT_FOUND) == 0) & (vert["throughput"][np.arange(len(seg)), k_last].max(-1) < 0.9)
    i = int(np.flatnonzero(escaped_late)[0])
    bad["added"][i, k_last[i]] = np.array(list(c.skyColor), F)
    fails(resummed(bad), bad, "added: a miss")
    # one `added` dropped from the sum
    lit = (seg >= 2) & (vert["added"][:, 1].max(-1) > 0)
    i = int(np.flatnonzero(lit)[0])
    bad_out = out.copy()
    dropped = vert.copy()
    dropped["added"][i, 1] = 0.0
    bad_out["radiance"][i] = P.running_sum(dropped, seg)[i]
    fails(bad_out, vert, "sum:")
    # the next directions of level 2 turned by a milliradian
    bad = vert.copy()
    m = seg >= 2
    d = vert["direction"][m, 1].astype(np.float64)
    axis = np.cross(d, [0.3, 0.5, 0.8])
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    bad["direction"][m, 1] = (d * np.cos(1e-3) + np.cross(axis, d) * np.sin(1e-3)).astype(F)
    fails(out, bad, "direction off")


# ------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------
def test_the_ray_sets_reach_every_kind_of_vertex(traced):
    which = R.room_with_extras()[1]
    for name in ("scattered", "outside"):
        t = traced["room, extras", name]
        out, vert = t["out"], t["vert"]
        seg, flags = out["segments"].astype(np.int64), vert["flags"]
        live = seg[:, None] > np.arange(K - 1)[None, :]
        miss = live & ((flags & _lib.HIT_FOUND) == 0)
        escaping = miss.sum(0)
        sampled = np.zeros_like(live)
        sampled[:, :-1] = live[:, 1:]
        divided = (sampled & ((flags & _lib.PATH_DIVIDED) != 0)).sum()
        undivided = (sampled & ((flags & _lib.PATH_DIVIDED) == 0)).sum()
        bare = (live & (vert["geometry"] == which[R.NO_MATERIAL])).sum(0)
        print(f"[coverage / {name}] alive at vertex 7: {int(live[:, K - 2].sum())}; escaping per level {escaping.tolist()}; divided {int(divided)}, "
              f"undivided {int(undivided)}; ended on the material-less box per level {bare.tolist()}")
        assert live[:, K - 2].sum() >= 10, name
        assert (escaping[1:] >= 1).all(), name
        assert divided >= 10 and undivided >= 10, name
        assert bare.sum() >= 10 and bare[1:].sum() >= 1, name
        ended = live & (vert["geometry"] == which[R.NO_MATERIAL])
        assert (seg[ended.any(-1)] == np.argmax(ended, -1)[ended.any(-1)] + 1).all(), name  # the path ends there
