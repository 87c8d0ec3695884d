"""neb_gi_probe_rays / neb_gi_bake_probes: what holds without a GPU -- the two records and the bindings' view of
them, the calibration the ray tolerance is derived from, tests/probe_ref.py's reducer against its own float64 projection on real path
records and on a constant radiance, and the reducer shown able to fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import path_ref as P
import probe_ref as B
import ray_query_ref as Q
import ray_shade_ref as R
from nebulae_amd import _lib, build
from nebulae_amd import scene as S
from oracle import gi_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
SAMPLES, K = 192, 3


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------
# 1: ABI
# ------------------------------------------------------------------------------------------------
def test_the_records_have_the_sizes_and_offsets_the_bindings_assume(tmp_path):
    fields = {"neb_probe": ("position", "tmin", "normal", "tmax"), "neb_probe_record": ("sh", "samples", "hits", "backfaces", "segments", "flags")}
    lines = "".join(f'  printf("{s} %zu", sizeof({s}));' + "".join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                    for s, fs in fields.items())
    lines += '  printf("%u %u %u\\n", NEB_BAKE_SH, NEB_BAKE_IRRADIANCE, NEB_PROBE_NOT_BAKED);\n'
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\nint main(void) {\n' + lines + "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    probe, record = ([int(w) for w in out[k].split()[1:]] for k in (0, 1))
    assert probe == [32, 0, 12, 16, 28], probe
    assert record == [128, 0, 108, 112, 116, 120, 124], record  # (samples at word 27)
    assert [B.PROBE.fields[k][1] for k in B.PROBE.names] == probe[1:] and [B.RECORD.fields[k][1] for k in B.RECORD.names] == record[1:]
    assert C.sizeof(_lib.Probe) == 32 and C.sizeof(_lib.ProbeRecord) == 128
    assert [getattr(_lib.Probe, k).offset for k in B.PROBE.names] == probe[1:]
    assert [getattr(_lib.ProbeRecord, k).offset for k in B.RECORD.names] == record[1:] and _lib.ProbeRecord.samples.offset == 4 * 27
    assert [int(w) for w in out[2].split()] == [_lib.BAKE_SH, _lib.BAKE_IRRADIANCE, _lib.PROBE_NOT_BAKED] == [0, 1, 1]


def test_the_library_exports_the_calls_and_refuses_a_null_context_without_a_device(tmp_path):
    build.build()
    lib = C.CDLL(build.LIB_PATH)
    assert hasattr(lib, "neb_gi_probe_rays") and hasattr(lib, "neb_gi_bake_probes")
    assert {"neb_gi_probe_rays", "neb_gi_bake_probes"} <= set(_lib.exported_symbols())
    sigs = _lib._gi_sigs()
    assert sigs["neb_gi_probe_rays"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    assert sigs["neb_gi_bake_probes"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants),
                                                    C.c_void_p, C.c_void_p])
    lib = _lib.load()
    c = P.constants(3)
    assert lib.neb_gi_probe_rays(None, None, 0, 64, 0, 1, None, None) == -1  # NEB_ERR_INVALID_ARG: a null context, no GPU touched
    assert lib.neb_gi_bake_probes(None, None, 0, 64, 0, 0, C.byref(c), None, None) == -1
    src = tmp_path / "use.cpp"
    src.write_text('#include "nebulae_hip.hpp"\n'
                   'static void use(Neb::GIPathtracer& g, const neb_probe* p, const neb_gi_constants* c, neb_ray* r, neb_probe_record* o, neb_stream s)\n'
                   '{ g.ProbeRays(p, 1, 64, NEB_BAKE_SH, 1, r, s); g.BakeProbes(p, 1, 64, NEB_BAKE_IRRADIANCE, 0, c, o, s); }\n'
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
# 2: the rays -- the float32 restatement under the judge, and what the tolerance is derived from
# ------------------------------------------------------------------------------------------------
def shapes_probes(n, seed=11):
    """n probes in the room's box with normals of every kind the frame's hemisphere sample distinguishes (|z| on both sides of 0.999)"""
    rng = np.random.default_rng(seed + n)
    pr = B.probes(rng.uniform(-0.8, 0.8, (n, 3)) + np.array([0.0, 0.0, -1.0]), tmin=1e-3)
    nrm = rng.standard_normal((n, 3))
    nrm[0::5] = (0.0, 0.0, 1.0)
    nrm[1::5] = (0.0, 1.0, 0.0)
    nrm[2::5] = (0.1, 0.2, -1.0)
    pr[:, 4:7] = nrm * rng.uniform(0.5, 3.0, (n, 1))
    return pr


def test_calibration():
    """The largest direction error of rays32 under judge_rays over the shapes the GPU test judges is what probe_ref.MEASURED says
    (TOL = 4 x); the float32 draws are the same bits in both, so everything before the directions is exact."""
    worst = 0.0
    for what in B.WHAT:
        for n in (1, 3, 65):
            for samples in (64, 192):
                pr = shapes_probes(n)
                up = np.abs(gi_np.normalize(pr[:, 4:7])[:, 2])
                assert (np.abs(up - 0.999) > 5e-4).all()  # (no normal near the frame's switch of tangent frames)
                worst = max(worst, B.judge_rays(pr, samples, what, 3, B.rays32(pr, samples, what, 3), f"rays32 / {what} / {n} x {samples}", tol=np.inf))
    print(f"[calibration] measured direction error {worst:.3e}; constant {B.MEASURED['direction']:.3e}")
    assert worst <= B.MEASURED["direction"] <= 1.25 * worst, f"the constant is not the measurement {worst:.3e} rounded up"
    assert B.TOL["direction"] == 4.0 * B.MEASURED["direction"]


def test_the_ray_judge_fails_what_it_should():
    pr = shapes_probes(3)
    for what in B.WHAT:
        good = B.rays32(pr, 64, what, 3)
        for word, spoil in (("direction", lambda r: r.__setitem__((slice(None), 4), r[:, 4] + F(2e-5))),
                            ("origin or interval", lambda r: r.__setitem__((5, 3), F(0.5))),
                            ("direction|stratum|below", lambda r: r.__setitem__((slice(None), slice(4, 7)), r[::-1, 4:7].copy()))):
            bad = good.copy()
            spoil(bad)
            with pytest.raises(AssertionError, match=word):
                B.judge_rays(pr, 64, what, 3, bad, "spoiled")
        assert not same_bits(good, B.rays32(pr, 64, what, 4))  # another frame index, other directions
    dead = pr.copy()
    dead[1, 0] = np.nan
    rays = B.rays32(dead, 64, "sh", 3)
    assert not rays[64:128].view(U32).any() and rays[:64].view(U32).any() and rays[128:].view(U32).any()


# ------------------------------------------------------------------------------------------------
# 3: the reducer on real path records
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced():
    """{what: (paths, rays)}: trace32's records along the reference's own rays, three probes in the room with extras"""
    sc, hidden = R.states()["room, extras"]
    tris = Q.triangles(sc, hidden)
    flat = gi_np.FlatScene(sc)
    lo, hi = Q.scene_box(sc)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    got = {}
    for what in B.WHAT:
        pr = B.probes([c + h * (0.1, -0.2, 0.3), c + h * (-0.5, 0.4, -0.3), c + h * (0.3, -0.9, 0.1)], normal=(0.05, 1.0, 0.1), tmin=1e-3)
        rays = B.rays32(pr, SAMPLES, what, 3)
        paths, _ = P.trace32(sc, tris, rays, P.constants(K), flat)
        assert (paths["segments"] > 0).all() and (paths["radiance"].max(-1) > 0).sum() > SAMPLES
        got[what] = (paths, rays)
    return got


@pytest.mark.parametrize("what", list(B.WHAT))
def test_bake_ref_is_inside_the_bound_of_the_float64_projection(traced, what):
    paths, rays = traced[what]
    rec = B.bake_ref(paths, rays, SAMPLES, what)
    value, bound = B.project64(paths, rays, SAMPLES, what)
    ratio = B.inside_bound(rec, value, bound)
    print(f"[bake_ref / {what}] largest error {ratio:.3f} of the bound; sh[0] {rec['sh'][:, 0].tolist()}")
    assert ratio <= 1.0
    assert (rec["samples"] == SAMPLES).all() and not rec["flags"].any() and (rec["hits"] > 0).all() and (rec["hits"] <= SAMPLES).all()
    assert np.array_equal(rec["segments"], paths["segments"].reshape(3, SAMPLES).sum(-1)) and (rec["segments"] <= SAMPLES * (K - 1)).all()
    if what == "irradiance":
        assert not rec["sh"][:, 1:].view(U32).any()


@pytest.mark.parametrize("what", list(B.WHAT))
def test_a_constant_radiance_gives_the_closed_form(traced, what):
    paths, rays = traced[what]
    flat_paths = paths.copy()
    L = np.array([0.75, 2.5, 8.0], F)
    flat_paths["radiance"] = L
    rec = B.bake_ref(flat_paths, rays, SAMPLES, what)
    _, bound = B.project64(flat_paths, rays, SAMPLES, what)
    want = (4.0 * np.pi * float(B.K00) if what == "sh" else np.pi) * L.astype(np.float64)
    # (the bound is around the float scale: the scale's own rounding, 2^-24 relative, is added)
    err = np.abs(rec["sh"][:, 0].astype(np.float64) - want)
    assert (err <= bound[:, 0:3] + 2.0 ** -24 * want).all(), (err, bound[:, 0:3])
    if what == "sh":  # the higher bands of a constant vanish with 1 / sqrt(S) at best: only that they are small against band 0
        assert np.abs(rec["sh"][:, 1:]).max() < 0.25 * rec["sh"][:, 0].max()


def test_bake_ref_fails_each_corruption(traced):
    lanes = np.arange(64)

    def dropped(words, S, scale):  # one round dropped
        return B.reduce32(words.reshape(-1, S, words.shape[-1])[:, :S - 64].reshape(-1, words.shape[-1]), S - 64, scale)

    def sequential(words, S, scale):  # the lanes of a round added one after the other
        w = words.reshape(-1, S // 64, 64, words.shape[-1])
        total = np.zeros((w.shape[0], w.shape[-1]), F)
        for r in range(S // 64):
            acc = w[:, r, 0].copy()
            for lane in lanes[1:]:
                acc = (acc + w[:, r, lane]).astype(F)
            total = (total + acc).astype(F)
        return (total * F(scale)).astype(F)

    def scale_per_round(words, S, scale):
        w = words.reshape(-1, S // 64, 64, words.shape[-1])
        total = np.zeros((w.shape[0], w.shape[-1]), F)
        for r in range(S // 64):
            total = (total + (B.butterfly(w[:, r]) * F(scale)).astype(F)).astype(F)
        return total

    def swapped(radiance, directions, what):  # Y(1,-1) and Y(1,1)
        w = B.words32(radiance, directions, what).reshape(-1, 9, 3)
        return w[:, [0, 3, 2, 1, 4, 5, 6, 7, 8]].reshape(-1, 27)

    for what in B.WHAT:
        paths, rays = traced[what]
        good = B.bake_ref(paths, rays, SAMPLES, what)
        value, bound = B.project64(paths, rays, SAMPLES, what)
        assert same_bits(good, B.bake_ref(paths, rays, SAMPLES, what))
        for name, reducer, outside in (("one round dropped", dropped, True), ("sequential lanes", sequential, False), ("scale per round", scale_per_round, False)):
            bad = B.bake_ref(paths, rays, SAMPLES, what, reducer=reducer)
            # (the inputs are chosen so that the bits do differ: real path radiances, three rounds -- checked here.  A change of rounding
            # can leave the three words of one irradiance record alone by chance; it does not leave three records alone.)
            differs = (bad["sh"].view(U32) != good["sh"].view(U32)).reshape(len(good), -1).any(-1)
            assert differs.all() if outside or what == "sh" else differs.any(), (what, name, differs)
            assert all(np.array_equal(bad[k], good[k]) for k in ("samples", "hits", "backfaces", "segments", "flags"))
            ratio = B.inside_bound(bad, value, bound)
            assert (ratio > 1.0) == outside, (what, name, ratio)  # a change of rounding stays inside the bound, a lost round does not
    paths, rays = traced["sh"]
    good, bad = B.bake_ref(paths, rays, SAMPLES, "sh"), B.bake_ref(paths, rays, SAMPLES, "sh", words=swapped)
    assert same_bits(bad["sh"][:, 1], good["sh"][:, 3]) and not same_bits(bad["sh"][:, 1], good["sh"][:, 1])
    assert B.inside_bound(bad, *B.project64(paths, rays, SAMPLES, "sh")) > 1.0
