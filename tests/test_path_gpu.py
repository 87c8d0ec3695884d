"""neb_gi_trace_paths: multi-bounce path radiance along the caller's rays -- with two path vertices against
neb_gi_shade_rays' radiance records bit for bit, with more against the per-vertex judge of tests/path_ref.py (whose tolerances
tests/test_path_cpu.py establishes on the CPU) with the device's own cast_rays / shade_rays as the judge's queries, sorted against
unsorted and with against without vertex records bit for bit, across updates and streams, beside a frame it must not disturb, and at
its refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import path_ref as P
import ray_query_ref as Q
import ray_shade_ref as R
import views_ref as V
from motion_ref import NO_SUBMESH
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from nebulae_amd.svgf import PLANE_RADIANCE, NebError
from test_ray_query_gpu import H, W, on_device, same_bits
from test_ray_query_gpu import cast as cast_rays
from test_ray_shade_gpu import _own_scene, renderer, state_renderer
from test_ray_shade_gpu import shade as shade_rays
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
FILL = float("nan")


# ------------------------------------------------------------------------------------------------
def enqueue(r, d_rays, c, sort=False, vertices=True, stream=None):
    """one call into buffers filled with a pattern no record has -> (out, vertices or None) tensors (nothing waits)"""
    n, K = d_rays.shape[0], int(c.maxPathVertices)
    out = torch.full((n, 8), FILL, dtype=torch.float32, device="cuda")
    vert = torch.full((n, K - 1, 24), FILL, dtype=torch.float32, device="cuda") if vertices else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = r.trace_paths(d_rays, constants=c, sort=sort, vertices=vert if vertices else False, out=out, stream=None if stream is None else stream.cuda_stream)
    assert res["records"] is out and (not vertices or res["vertex_records"] is vert)
    return out, vert


def to_host(pair):
    out, vert = pair
    paths = np.ascontiguousarray(out.cpu().numpy()).view(P.PATH).reshape(-1)
    if vert is None:
        return paths, None
    return paths, np.ascontiguousarray(vert.cpu().numpy()).view(P.VERTEX).reshape(vert.shape[0], vert.shape[1])


def trace(r, rays, c, sort=False, vertices=True):
    d = on_device(rays)
    torch.cuda.synchronize()
    pair = enqueue(r, d, c, sort, vertices)
    torch.cuda.synchronize()
    return to_host(pair)


@pytest.fixture(scope="module")
def cases():
    """the scene states of tests/ray_shade_ref.py with their ray sets, computed once and left unchanged"""
    out = {}
    for name, (sc, hidden) in R.states().items():
        tris = Q.triangles(sc, hidden)
        out[name] = dict(scene=sc, hidden=hidden, tris=tris, sets=Q.ray_sets(*Q.scene_box(sc), tris))
    return out


# ------------------------------------------------------------------------------------------------
# 1: two path vertices are NEB_SHADE_RADIANCE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("state", list(R.states()))
def test_two_vertices_are_the_radiance_records_bit_for_bit(cases, state, exact):
    case = cases[state]
    r = state_renderer(case, bool(exact))
    no_sun = P.constants(2)
    no_sun.sunLightDirection[:] = (0.0, 0.0, 0.0)  # (a NaN sun frame, a shadow ray the walk refuses: the same bits all the same)
    for name in Q.SETS:
        rays = case["sets"][name]
        for what, c in (("centre", P.constants(2, tan_half=0.0)), ("disk", P.constants(2)), ("zero sun", no_sun)):
            paths, vert = trace(r, rays, c)
            rad = shade_rays(r, rays, "radiance", c)
            for k in ("radiance", "t", "geometry", "primitive"):
                assert same_bits(paths[k].view(U32), rad[k].view(U32)), (state, name, what, k)
            assert same_bits(paths["flags"] & P.HIT_BITS, rad["flags"]), (state, name, what)
            assert same_bits(paths["radiance"].view(U32), vert["added"][:, 0].view(U32)) and (paths["segments"] <= 1).all(), (state, name, what)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: the judge, vertex by vertex, with the device's own queries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("name", P.JUDGED_SETS)
@pytest.mark.parametrize("state", list(R.states()))
def test_every_vertex_against_float64_and_the_library_s_own_queries(cases, state, name, K, exact):
    case = cases[state]
    r = state_renderer(case, bool(exact))
    rays, c = case["sets"][name], P.constants(K)
    paths, vert = trace(r, rays, c)
    verdict = P.judge_vertices(case["scene"], case["tris"], rays, c, paths, vert, lambda x, any_hit=False: cast_rays(r, x, any_hit=any_hit),
                               lambda x: shade_rays(r, x, "surface"), f"{state} / {name} / K {K} / exact {exact}")
    assert verdict["live"][0] == len(rays)
    if case["hidden"]:
        assert not np.isin(vert["geometry"], list(case["hidden"])).any()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3, 4, 5: the same bits with and without vertex records, sorted and unsorted, twice
# ------------------------------------------------------------------------------------------------
def test_out_is_the_same_bits_with_and_without_vertices_and_on_a_second_call(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    for K in (2, 5, 8):
        c = P.constants(K)
        for name in ("scattered", "outside"):
            rays = case["sets"][name]
            with_v, vert = trace(r, rays, c)
            without, none = trace(r, rays, c, vertices=False)
            again, vert2 = trace(r, rays, c)
            assert none is None and same_bits(with_v, without) and same_bits(with_v, again) and same_bits(vert, vert2), (K, name)
            assert not np.isnan(with_v["t"]).any() and not np.isnan(vert["tmax"]).any()  # (every record replaced the buffer's fill)
    r.destroy()


def test_sorted_equals_unsorted_bit_for_bit(cases):
    """wave boundaries and one ray past raysort's 4096-pair tile; the whole of both buffers"""
    case = cases["room"]
    r = state_renderer(case, exact=False)
    pool = np.concatenate([case["sets"][k] for k in ("scattered", "outside", "axis")])
    c = P.constants(8)
    for n in (1, 63, 64, 65, 4097):
        a, av = trace(r, pool[:n], c)
        b, bv = trace(r, pool[:n], c, sort=True)
        assert same_bits(a, b) and same_bits(av, bv), n
        assert same_bits(a, trace(r, pool[:n], c, sort=True, vertices=False)[0]), n
    assert (a["segments"] == 7).sum() > 100
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 6: rays that cannot be walked
# ------------------------------------------------------------------------------------------------
def test_rays_that_cannot_be_walked_say_so_and_a_real_miss_carries_the_sky(cases):
    case = cases["room"]
    r = state_renderer(case)
    c = P.constants(8)
    good = case["sets"]["scattered"].copy()  # (the room is open at the front: some leave it and miss for real)
    n = len(good)
    bad = good.copy()
    kinds = ["zero direction", "nan origin", "infinite direction", "tmin -1", "tmin nan", "tmax == tmin"]
    where = {}
    for base in (0, n - 64):  # one of each kind in the first wave and one in the last
        for k, kind in enumerate(kinds):
            i = base + 5 + 9 * k
            where[i] = kind
            if kind == "zero direction":
                bad[i, 4:7] = 0.0
            elif kind == "nan origin":
                bad[i, 1] = np.nan
            elif kind == "infinite direction":
                bad[i, 5] = np.inf
            elif kind == "tmin -1":
                bad[i, 3] = -1.0
            elif kind == "tmin nan":
                bad[i, 3] = np.nan
            else:
                bad[i, 3] = bad[i, 7] = 0.25
    rows = np.array(sorted(where))
    others = np.setdiff1d(np.arange(n), rows)
    blank = np.zeros(1, P.PATH)
    blank["t"], blank["geometry"], blank["primitive"], blank["flags"] = np.inf, NO_SUBMESH, NO_SUBMESH, _lib.HIT_NOT_WALKED
    sky = np.zeros(1, P.PATH)
    sky["radiance"], sky["t"], sky["geometry"], sky["primitive"], sky["flags"], sky["segments"] = list(c.skyColor), np.inf, NO_SUBMESH, NO_SUBMESH, _lib.PATH_ESCAPED, 1
    for sort in (False, True):
        (a, av), (b, bv) = trace(r, good, c, sort), trace(r, bad, c, sort)
        assert same_bits(a[others], b[others]) and same_bits(av[others], bv[others]), sort
        for i in rows:
            assert same_bits(b[i:i + 1], blank), (sort, where[i], b[i])
        assert not bv[rows].view(U32).any(), sort
        missed = a["geometry"] == NO_SUBMESH
        assert missed.sum() >= 10 and same_bits(a[missed], np.repeat(sky, int(missed.sum()))), sort  # a real first-segment miss: the sky's exact bits
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 7: linearity in the two lights (no formula of the path is restated here)
# ------------------------------------------------------------------------------------------------
def test_sky_and_sun_add_up(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    both, sky_only, sun_only = P.constants(8), P.constants(8), P.constants(8)
    sky_only.sunLightRadiance[:] = (0.0, 0.0, 0.0)
    sun_only.skyColor[:] = (0.0, 0.0, 0.0)
    assert max(both.skyColor) > 0 and max(both.sunLightRadiance) > 0
    for name in ("scattered", "outside"):
        rays = case["sets"][name]
        (a, _), (b, _), (ab, _) = (trace(r, rays, c, vertices=False) for c in (sky_only, sun_only, both))
        agree = (a["segments"] == ab["segments"]) & (b["segments"] == ab["segments"]) & (a["flags"] == ab["flags"]) & (b["flags"] == ab["flags"])
        assert agree.sum() >= 0.99 * len(rays), name
        want = a["radiance"].astype(np.float64) + b["radiance"].astype(np.float64)
        e = (np.abs(ab["radiance"].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max(-1)
        tol = P.TOL["added"] * np.maximum(ab["segments"], 1)
        print(f"[linearity / {name}] {int(agree.sum())} rays agree in segments and flags; largest error {float(e[agree].max()):.2e}, "
              f"largest sum {float(want[agree].max()):.3f}")
        assert (e[agree] <= tol[agree]).all(), name
        assert (a["radiance"][agree].max(-1) > 0).sum() > 100 and (b["radiance"][agree].max(-1) > 0).sum() > 100, name
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 8: updates are seen
# ------------------------------------------------------------------------------------------------
def test_updates_reach_the_query_without_rebuild_or_host_synchronisation(cases):
    sc0, updates = V.room_updates()
    sc = _own_scene(sc0)
    r = renderer(sc)
    c = P.constants(5)
    rays = cases["room"]["sets"]["scattered"]
    d = on_device(rays)
    before = to_host(enqueue(r, d, c))
    torch.cuda.synchronize()
    RED = sc.geometries[3]["material"]
    ALBEDO_MAP = sc.materials[sc.geometries[0]["material"]]["textures"][0]
    # the four updates and the query, enqueued back to back
    r.update_materials([RED], albedo=[(0.11, 0.22, 0.83)])
    r.update_texture(ALBEDO_MAP, np.full((64, 96, 4), (250, 3, 120, 255), np.uint8), x=40, y=100)
    _, _, (indices, moved), s1 = updates[0]  # the boxes rotated
    r.update_transforms(indices, moved)
    r.set_visible([V.POST], False)
    pair = enqueue(r, d, c)
    torch.cuda.synchronize()
    behind = to_host(pair)
    settled = to_host(enqueue(r, d, c))
    torch.cuda.synchronize()
    assert same_bits(behind[0], settled[0]) and same_bits(behind[1], settled[1])
    assert not same_bits(behind[0]["radiance"], before[0]["radiance"])
    assert (before[1]["geometry"] == V.POST).any() and not (behind[1]["geometry"] == V.POST).any()
    now = r._scene
    P.judge_vertices(now, Q.triangles(now, (V.POST,)), rays, c, behind[0], behind[1], lambda x, any_hit=False: cast_rays(r, x, any_hit=any_hit),
                     lambda x: shade_rays(r, x, "surface"), "after four updates")
    r.destroy()


def test_a_query_runs_behind_an_update_on_another_stream_and_a_later_update_waits_for_it():
    sc0, updates = V.room_updates()
    _, _, (indices, moved), s1 = updates[0]  # the boxes rotated
    orig = np.stack([sc0.geometries[i]["M"] for i in indices])
    one = Q.ray_sets(*Q.scene_box(s1), Q.triangles(s1))["scattered"]
    rays = np.tile(one, (4, 1))  # (a query long enough for an update to overtake, if it could)
    c = P.constants(8)
    r = renderer(clone(sc0))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    d = on_device(rays)
    still = to_host(enqueue(r, d, c))  # the scene before the move
    torch.cuda.synchronize()
    r.update_transforms(indices, moved, stream=a.cuda_stream)
    out1 = enqueue(r, d, c, stream=b)  # no host synchronisation in between
    torch.cuda.synchronize()
    h1 = to_host(out1)
    settled = to_host(enqueue(r, d, c))
    torch.cuda.synchronize()
    # the opposite order: the query on b, then an update on a that moves the boxes back
    out2 = enqueue(r, d, c, sort=True, stream=b)
    r.update_transforms(indices, orig, stream=a.cuda_stream)
    torch.cuda.synchronize()
    h2 = to_host(out2)
    back = to_host(enqueue(r, d, c))
    torch.cuda.synchronize()
    for k in (0, 1):
        assert same_bits(h1[k], settled[k]) and same_bits(h1[k], h2[k]) and same_bits(back[k], still[k]) and not same_bits(still[k], h1[k]), k
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 9: the frame is untouched
# ------------------------------------------------------------------------------------------------
def test_the_frame_its_counters_and_the_sun_table_are_untouched(cases):
    case = cases["room"]
    sc, cam = clone(case["scene"]), cornell_camera()
    r = _renderer(sc, cam, W, H, sun_table=1, hits=True)
    for f in (2, 3):
        frame(r, sc, cam, f)

    def snapshot():
        torch.cuda.synchronize()
        return r.ray_count(), r.traversal_stats(), r.sun_table_stats(), r.svgf.download(PLANE_RADIANCE).copy()
    count, trav, table, plane = snapshot()
    assert count > 0 and table["builds"] == 1 and plane[..., :3].max() > 0.05
    other_sun = P.constants(8, frame_index=9)
    other_sun.sunLightDirection[:] = (-0.3, -1.0, 0.4)  # (a sun the table was not built for: the call must not make it chase)
    rays = case["sets"]["scattered"]
    for sort in (False, True):
        for c in (P.constants(8), other_sun, P.constants(2)):
            paths, _ = trace(r, rays, c, sort)
            assert (paths["flags"] & _lib.HIT_FOUND).any()
    count2, trav2, table2, plane2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(plane2, plane)
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05  # the table still serves its own sun
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 10: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_name_the_cause(cases):
    case = cases["room"]
    rays = case["sets"]["scattered"]
    n = len(rays)
    d = on_device(rays)
    r = DeferredRenderer()
    r.init(W, H)
    lib, ctx = r._lib, r._ctx
    out = torch.full((n + 1, 8), FILL, dtype=torch.float32, device="cuda")
    vert = torch.full((n + 1, 2, 24), FILL, dtype=torch.float32, device="cuda")
    k3, k1, k9 = P.constants(3), P.constants(3), P.constants(3)
    k1.maxPathVertices, k9.maxPathVertices = 1, 9
    cp = C.byref(k3)
    SORT = _lib.RAYS_SORT

    def call(p_rays, count, flags, c, p_out, p_vert):
        return lib.neb_gi_trace_paths(ctx, C.c_void_p(p_rays), count, flags, c, C.c_void_p(p_out), C.c_void_p(p_vert), None)

    def error():
        return lib.neb_last_error(ctx)

    assert call(d.data_ptr(), n, 0, cp, out.data_ptr(), 0) == -4 and b"neb_gi_trace_paths" in error()  # no scene
    sc = clone(case["scene"])
    G, ng, M, nm, T, nt = sc.descs()
    assert lib.neb_gi_set_scene(ctx, G, ng, M, nm, T, nt) == 0
    assert call(d.data_ptr(), n, 0, cp, out.data_ptr(), vert.data_ptr()) == -4 and b"not ready" in error()  # a scene, no tree
    assert lib.neb_gi_build_bvh(ctx, None) == 0
    host_mem = torch.empty((n + 2, 48), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    D, O, VX = d.data_ptr(), out.data_ptr(), vert.data_ptr()
    refused = [("null constants", (D, n, 0, None, O, VX), -1, b"constants"),
               ("one path vertex", (D, n, 0, C.byref(k1), O, VX), -1, b"maxPathVertices"),
               ("nine path vertices", (D, n, SORT, C.byref(k9), O, 0), -1, b"maxPathVertices"),
               ("unknown flag", (D, n, 4, cp, O, VX), -1, b"flag"),
               ("any hit", (D, n, _lib.RAYS_ANY_HIT, cp, O, VX), -1, b"NEB_RAYS_ANY_HIT"),
               ("any hit, sorted", (D, n, _lib.RAYS_ANY_HIT | SORT, cp, O, 0), -1, b"NEB_RAYS_ANY_HIT"),
               ("null rays", (0, n, 0, cp, O, VX), -1, b"null"),
               ("null out", (D, n, SORT, cp, 0, VX), -1, b"null"),
               ("misaligned rays", (D + 8, n - 1, 0, cp, O, VX), -1, b"misaligned"),
               ("misaligned out", (D, n, 0, cp, O + 16, VX), -1, b"misaligned"),
               ("misaligned vertices", (D, n, 0, cp, O, VX + 16), -1, b"misaligned"),
               ("host-memory rays", (host_ptr, n, 0, cp, O, VX), -1, b"rays is not memory"),
               ("host-memory out", (D, n, 0, cp, host_ptr, VX), -1, b"out is not memory"),
               ("host-memory vertices", (D, n, 0, cp, O, host_ptr), -1, b"vertices is not memory"),
               ("out overlapping rays", (D, n, 0, cp, D + 32 * (n - 1), VX), -1, b"overlaps"),
               ("out is rays", (D, n, SORT, cp, D, 0), -1, b"overlaps"),
               ("vertices overlapping rays", (D, n, 0, cp, O, D + 32 * (n - 1)), -1, b"overlaps"),
               ("vertices overlapping out", (D, n, 0, cp, O, O + 32 * (n - 1)), -1, b"overlaps"),
               ("vertices is out", (D, n, SORT, cp, O, O), -1, b"overlaps"),
               ("too many rays", (D, (1 << 28) + 1, 0, cp, O, VX), -5, b"2^28"),
               ("out too small for its allocation", (D, n, SORT, cp, end - 32 * (n - 1), VX), -1, b"out is not memory"),
               ("vertices too small for their allocation", (D, n, 0, cp, O, end - 192 * n + 96), -1, b"vertices is not memory"),
               ("rays too short for their allocation", (end - 32 * (n - 1), n, 0, cp, O, VX), -1, b"rays is not memory")]
    torch.cuda.synchronize()
    for what, args, want, word in refused:
        assert call(*args) == want, (what, error())
        assert b"neb_gi_trace_paths" in error() and word in error(), (what, error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(vert).all()), "a refused call wrote something"
    assert call(0, 0, 0, cp, 0, 0) == 0 and call(0, 0, SORT, None, 0, 0) == 0  # n == 0: a no-op that succeeds and looks at no pointer
    # ... and the same context answers: the ranges that just fit their allocation are accepted
    assert call(D, n, 0, cp, O, end - 192 * n) == 0
    assert call(D, n, 0, cp, O, VX) == 0
    torch.cuda.synchronize()
    paths, vs = to_host((out[:n], vert[:n]))
    P.judge_vertices(case["scene"], case["tris"], rays, k3, paths, vs, lambda x, any_hit=False: cast_rays(r, x, any_hit=any_hit),
                     lambda x: shade_rays(r, x, "surface"), "after the refusals")
    assert bool(torch.isnan(out[n]).all()) and bool(torch.isnan(vert[n]).all())
    r.destroy()


def test_the_python_mirror_checks_its_arguments_and_returns_the_views(cases):
    r = state_renderer(cases["room"])
    d = on_device(cases["room"]["sets"]["scattered"][:100])
    for bad in (d.cpu(), d[:, :7], d.double(), d[::2]):
        with pytest.raises(NebError):
            r.trace_paths(bad)
    with pytest.raises(NebError):
        r.trace_paths(d, out=torch.empty((100, 8), dtype=torch.float32))
    with pytest.raises(NebError):
        r.trace_paths(d, max_path_vertices=4, vertices=torch.empty((100, 4, 24), dtype=torch.float32, device="cuda"))
    for K in (1, 9):
        with pytest.raises(NebError):
            r.trace_paths(d, max_path_vertices=K)
    c = P.constants(3)
    res = r.trace_paths(d, constants=c, max_path_vertices=6, vertices=True)
    assert c.maxPathVertices == 3  # the caller's constants are left alone
    views = ("radiance", "t", "geometry", "primitive", "flags", "segments")
    assert res["records"].shape == (100, 8) and res["vertex_records"].shape == (100, 5, 24)
    assert [res[k].data_ptr() - res["records"].data_ptr() for k in views] == [P.PATH.fields[k][1] for k in views]
    vviews = {"origin": "origin", "tmin": "tmin", "direction": "direction", "vertex_t": "t", "throughput": "throughput", "rng": "rng", "added": "added",
              "vertex_flags": "flags", "vertex_geometry": "geometry", "vertex_primitive": "primitive", "u": "u", "v": "v", "tmax": "tmax", "pdiff": "pdiff"}
    assert set(res) == set(views) | set(vviews) | {"records", "vertex_records"}
    assert [res[k].data_ptr() - res["vertex_records"].data_ptr() for k in vviews] == [P.VERTEX.fields[f][1] for f in vviews.values()]
    assert all(res[k].dtype == torch.int32 for k in ("geometry", "primitive", "flags", "segments", "rng", "vertex_flags")) and res["added"].shape == (100, 5, 3)
    res = r.trace_paths(d)  # (the frame's own constants)
    assert set(res) == set(views) | {"records"}
    empty = r.trace_paths(d[:0], max_path_vertices=8, sort=True, vertices=True)
    assert empty["records"].shape == (0, 8) and empty["vertex_records"].shape == (0, 7, 24)
    torch.cuda.synchronize()
    r.destroy()
