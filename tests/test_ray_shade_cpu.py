"""neb_gi_shade_rays: what holds without a GPU -- the two records and the bindings' view of them, the judges of
tests/ray_shade_ref.py shown able to pass and to fail, and the calibration their tolerances are derived from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ray_query_ref as Q
import ray_shade_ref as R
from nebulae_amd import _lib, build
from nebulae_amd import scene as S
from oracle import gi_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32


# ------------------------------------------------------------------------------------------------
# 1: ABI
# ------------------------------------------------------------------------------------------------
def test_the_records_have_the_sizes_and_offsets_the_bindings_assume(tmp_path):
    fields = {"neb_ray_surface": ("position", "t", "geometricNormal", "geometry", "shadingNormal", "primitive", "albedo", "roughness", "metalness",
                                  "texcoord", "material", "u", "v", "flags", "reserved"),
              "neb_ray_radiance": ("r", "t", "geometry", "primitive", "flags", "reserved")}
    lines = "".join(f'  printf("{s} %zu", sizeof({s}));' + "".join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                    for s, fs in fields.items())
    consts = ("NEB_SHADE_SURFACE", "NEB_SHADE_RADIANCE", "NEB_HIT_FOUND", "NEB_HIT_ATTRIBUTES", "NEB_HIT_MATERIAL", "NEB_HIT_BACKFACE", "NEB_HIT_NOT_WALKED",
              "NEB_HIT_SUN_VISIBLE")
    lines += '  printf("' + " %u" * len(consts) + '\\n", ' + ", ".join(consts) + ");\n"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\nint main(void) {\n' + lines + "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    surface = [int(w) for w in out[0].split()[1:]]
    radiance = [int(w) for w in out[1].split()[1:]]
    assert surface == [96, 0, 12, 16, 28, 32, 44, 48, 60, 64, 68, 76, 80, 84, 88, 92], surface
    assert radiance == [32, 0, 12, 16, 20, 24, 28], radiance
    # ... which is where the test mirrors and the renderer's views look
    assert [R.SURFACE.fields[k][1] for k in R.SURFACE.names] == surface[1:] and R.SURFACE.itemsize == 96
    assert [R.RADIANCE.fields[k][1] for k in R.RADIANCE.names] == radiance[1:] and R.RADIANCE.itemsize == 32
    assert [int(w) for w in out[2].split()] == [_lib.SHADE_SURFACE, _lib.SHADE_RADIANCE, _lib.HIT_FOUND, _lib.HIT_ATTRIBUTES, _lib.HIT_MATERIAL,
                                                _lib.HIT_BACKFACE, _lib.HIT_NOT_WALKED, _lib.HIT_SUN_VISIBLE] == [0, 1, 1, 2, 4, 8, 16, 32]


def test_the_library_exports_the_call_and_the_bindings_declare_it(tmp_path):
    build.build()
    assert hasattr(C.CDLL(build.LIB_PATH), "neb_gi_shade_rays") and "neb_gi_shade_rays" in _lib.exported_symbols()
    assert _lib._gi_sigs()["neb_gi_shade_rays"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants),
                                                              C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert lib.neb_gi_shade_rays(None, None, 0, 0, 0, None, None, None) == -1  # a null context
    src = tmp_path / "use.cpp"
    src.write_text('#include "nebulae_hip.hpp"\n'
                   'static void use(Neb::GIPathtracer& g, const neb_ray* r, const neb_gi_constants* c, neb_ray_surface* a, neb_ray_radiance* b, neb_stream s)\n'
                   '{ g.ShadeRays(r, 1, NEB_SHADE_SURFACE, 0, nullptr, a, s); g.ShadeRays(r, 1, NEB_SHADE_RADIANCE, NEB_RAYS_SORT, c, b, s); }\n'
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
# the states and sets of the GPU tests, with float64's own answers
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (sc, hidden) in R.states().items():
        tris = Q.triangles(sc, hidden)
        sets = Q.ray_sets(*Q.scene_box(sc), tris)
        out[name] = dict(scene=sc, tris=tris, sets=sets, flat=gi_np.FlatScene(sc))
    return out


def _float64_answers(case, name, c):
    rays = case["sets"][name]
    ref = Q.reference(case["tris"], rays)
    reading = R.reading64(case["scene"], case["tris"], rays, ref["geometry"], ref["primitive"], c)
    return rays, ref, R.as_answers(reading, rays, ref["geometry"], ref["primitive"])


# ------------------------------------------------------------------------------------------------
# 2: the judges can fail
# ------------------------------------------------------------------------------------------------
def test_the_judges_pass_float64_and_fail_what_they_should(cases):
    case = cases["room, extras"]
    sc, tris = case["scene"], case["tris"]
    c = R.constants()
    rays, ref, ans = _float64_answers(case, "scattered", c)
    rays = rays.copy()
    rays[7, 4:7] = 0.0  # one ray that cannot be walked
    g, p = ref["geometry"].copy(), ref["primitive"].copy()
    g[7] = p[7] = Q.NO_SUBMESH
    ans = R.as_answers(R.reading64(sc, tris, rays, g, p, c), rays, g, p)
    surf, rad = R.surface_records(ans), R.radiance_records(ans)
    R.judge_surface(sc, tris, rays, surf, "float64 fed back")
    assert R.judge_radiance(sc, tris, rays, rad, c, "float64 fed back")[0] == 0
    shaded, att = ans["shaded"], ans["attributes"]
    assert shaded.sum() > 1000 and (att & ~shaded).sum() > 10 and (ans["found"] & ~att).sum() > 10 and not ans["walkable"][7]
    normal_mapped = shaded & (np.abs(ans["SN"] - ans["GN"]).max(-1) > 1e-3)
    assert normal_mapped.sum() > 500

    def fails(judge, rec, *more):
        with pytest.raises(AssertionError):
            judge(sc, tris, rays, rec, *more, "a record that is wrong")

    bad = surf.copy()
    bad["albedo"] = bad["albedo"][:, [1, 0, 2]]  # a swapped albedo channel
    fails(R.judge_surface, bad)
    bad = surf.copy()
    bad["shading_normal"][normal_mapped] = bad["geometric_normal"][normal_mapped]  # SN = GN on normal-mapped hits
    fails(R.judge_surface, bad)
    bad = surf.copy()
    k = int(np.flatnonzero(att)[3])
    a = 1e-3  # one normal rotated by a milliradian about an axis across it
    n = bad["geometric_normal"][k].astype(np.float64)
    axis = np.cross(n, [0.3, 0.5, 0.8])
    axis /= np.linalg.norm(axis)
    bad["geometric_normal"][k] = n * np.cos(a) + np.cross(axis, n) * np.sin(a)
    fails(R.judge_surface, bad)
    bad = surf.copy()
    bad["texcoord"][np.flatnonzero(ans["found"] & ~att)[0]] = 0.5  # a field a clear flag leaves
    fails(R.judge_surface, bad)
    bad = rad.copy()
    nine = np.flatnonzero(shaded)[::37][:9]  # nine flipped sun flags, their light following the flag
    bad["flags"][nine] ^= _lib.HIT_SUN_VISIBLE
    bad["radiance"][nine] = np.where(((bad["flags"][nine] & _lib.HIT_SUN_VISIBLE) != 0)[:, None], ans["lit"][nine], 0.0)
    fails(R.judge_radiance, bad, c)
    eight = bad.copy()
    eight["flags"][nine[0]], eight["radiance"][nine[0]] = rad["flags"][nine[0]], rad["radiance"][nine[0]]
    assert R.judge_radiance(sc, tris, rays, eight, c, "eight flipped flags")[0] == 8  # (the cap itself)
    bad = rad.copy()
    bad["radiance"][7] = np.array(list(c.skyColor), F)  # sky on a ray that was not walked
    fails(R.judge_radiance, bad, c)
    bad = rad.copy()
    lit = int(np.argmax(ans["radiance"].max(-1) * ans["visible"]))  # (the brightest lit hit: above 1, where the error is relative)
    assert ans["radiance"][lit].max() > 1.0
    bad["radiance"][lit] *= F(1.0 + 2.0 * R.TOL["radiance"])
    fails(R.judge_radiance, bad, c)


# ------------------------------------------------------------------------------------------------
# 3: calibration
# ------------------------------------------------------------------------------------------------
def test_calibration(cases):
    """The float32 reading against the float64 restatement on float64's own triangles, every state and set of the GPU tests: the
    largest error of each field class is what ray_shade_ref.MEASURED says (TOL = 4 x), and the float32 chain's shadow outcomes differ
    from float64's at no more than TIE_CAP // 2 rays per set, at the disk's centre and with the default disk."""
    worst = {k: 0.0 for k in R.FIELDS}
    for state, case in cases.items():
        sc, tris = case["scene"], case["tris"]
        for name in Q.SETS:
            rays = case["sets"][name]
            ref = Q.reference(tris, rays)
            for tan_half in (0.0, None):
                c = R.constants(frame_index=3, tan_half=tan_half)
                r64 = R.reading64(sc, tris, rays, ref["geometry"], ref["primitive"], c)
                r32 = R.reading32(sc, tris, rays, ref["geometry"], ref["primitive"], c, flat=case["flat"])
                assert np.array_equal(r32["shaded"], r64["shaded"])
                err = R.errors(r64, r32, "lit")
                differ = int((r32["visible"] != r64["visible"]).sum())
                print(f"[{state} / {name} / tan {float(c.sunTanHalfAngle):.4f}] " + ", ".join(f"{k} {v:.3e}" for k, v in err.items())
                      + f"; shadow outcomes differ at {differ} of {int(r64['shaded'].sum())} ({int(r64['visible'].sum())} see the sun); "
                      f"largest radiance {float(r64['lit'].max(initial=0.0)):.3f}, smallest roughness {float(r64['roughness'][r64['shaded']].min(initial=1.0)):.3f}")
                assert differ <= R.TIE_CAP // 2, (state, name, differ)
                for k, v in err.items():
                    worst[k] = max(worst[k], v)
    print("[calibration] measured maxima: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    print("[calibration] constants:       " + ", ".join(f"{k} {R.MEASURED[k]:.3e}" for k in worst))
    for k, v in worst.items():
        assert v <= R.MEASURED[k], (k, v)
        assert R.MEASURED[k] <= 1.25 * v, f"{k}: the constant {R.MEASURED[k]:.3e} is not the measurement {v:.3e} rounded up"
        assert R.TOL[k] == 4.0 * R.MEASURED[k]
