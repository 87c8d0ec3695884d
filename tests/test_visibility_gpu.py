"""neb_gi_set_visibility: submeshes hidden and shown in place, the tree kept.

The reference of a hidden submesh is the scene "without" it: the submesh keeps its slot in the geometry table and gets an empty index
list, so geometry ids agree and hit records compare directly.  The bar is test_refit_gpu's for refit == rebuild: G-buffer planes,
radiance, hit records and ray counts bit for bit, except at most TIE_CAP pixels per frame with coincident hits (assert_same_frames).
Frames are 64 x 48 unless stated."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import morph_ref
import reproject_ref as R
import views_ref as V
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import (NebError, PLANE_ALBEDO, PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE, PLANE_ROUGH_METAL, PLANE_SUBMESH_ID,
                              PLANE_WORLDPOS, SLOT_CURRENT)
from test_deform_gpu import ATRIUM_COLUMNS, twist_and_shear, with_arrays
from test_gi_gpu import scenes
from test_motion_gpu import motion_renderer, outputs, reference, seed_planes
from test_refit_gpu import TIE_CAP, _bits, _renderer, assert_same_frames, clone, cornell_camera, cornell_parts, frame, moved_matrices, \
    with_matrices, world_transform
from reproject_ref import surface
from test_reproject_gpu import seeded_history
from test_skin_gpu import cornell_case as skin_cornell_case, on_device
from test_update_views_gpu import _assert_split, _assert_view, _look, _motion_on, longthin

pytestmark = pytest.mark.gpu

F = np.float32
VW, VH = 64, 48
KEYS = ("positions", "normals", "tangents")
SINGLES = [(k,) for k in range(5)]
PAIRS = [(a, b) for a in range(5) for b in range(a + 1, 5)]
HIDE_FRAMES = ((3, 1), (4, 4), (5, 1))  # (frame index, spp); with the table on, the hold of two dispatches ends inside the sequence
SHOW_FRAMES = ((6, 1), (7, 4), (8, 1))


@functools.lru_cache(maxsize=None)
def parts():
    """cornell_parts(), made once and never written to (every context gets a clone that shares its arrays)"""
    return cornell_parts()


def without(sc, hidden):
    """the scene with the named geometries' index lists emptied: they keep their slots"""
    out = clone(sc)
    for gi in hidden:
        out.geometries[gi]["indices"] = sc.geometries[gi]["indices"][:0].copy()
    return out


def rend(sc, cam, sun_table=1, w=VW, h=VH, **init):
    return _renderer(sc, cam, w, h, sun_table=sun_table, **init)


@functools.lru_cache(maxsize=None)
def full_frames(sun_table):
    """the untouched Cornell parts at every (frame, spp) the tests render after a show: computed once per table setting"""
    sc, cam = clone(parts()), cornell_camera()
    r = rend(sc, cam, sun_table)
    out = {(f, spp): frame(r, sc, cam, f, spp) for f, spp in SHOW_FRAMES}
    r.destroy()
    return out


def same_box(ra, rb, what):
    (alo, ahi), (blo, bhi) = ra.scene_box(), rb.scene_box()
    assert np.array_equal(alo.view(np.uint32), blo.view(np.uint32)) and np.array_equal(ahi.view(np.uint32), bhi.view(np.uint32)), (what, alo, ahi, blo, bhi)


# ------------------------------------------------------------------------------------------------
# 1: every single submesh and every pair of the smallest scene, hidden and shown
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("subset", SINGLES + PAIRS, ids=lambda s: "hide" + "".join(str(k) for k in s))
def test_hidden_equals_the_scene_without_and_shown_equals_the_full_scene(subset, sun_table):
    sc0, cam = parts(), cornell_camera()
    sa, sb = clone(sc0), without(sc0, subset)
    ra, rb = rend(sa, cam, sun_table), rend(sb, cam, sun_table)
    depth, info = ra.bvh_depth(), ra.scene_info()
    frame(ra, sa, cam, 2)  # (a dispatch before the call: with the table on, it exists and is then dropped)
    ra.set_visible(list(subset), False)
    assert ra.bvh_depth() == depth and ra.scene_info() == info  # the tree is kept
    assert ra.visibility().tolist() == [k not in subset for k in range(5)]
    same_box(ra, rb, f"hidden {subset}")
    for f, spp in HIDE_FRAMES:
        a, b = frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp)
        assert not np.isin(a["hits"]["geometry"][a["hits"]["t"] >= 0], subset).any()
        assert_same_frames(a, b, f"hidden {subset} table={sun_table} f={f} spp={spp}")
    if sun_table:
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 1
    ra.set_visible(list(subset), [True] * len(subset))
    assert ra.visibility().all()
    for f, spp in SHOW_FRAMES:
        assert_same_frames(frame(ra, sa, cam, f, spp), full_frames(sun_table)[(f, spp)], f"shown again {subset} table={sun_table} f={f} spp={spp}")
    ra.destroy(), rb.destroy()


@pytest.mark.parametrize("subset", [(1,), (0, 2), (3, 4)], ids=lambda s: "hide" + "".join(str(k) for k in s))
def test_the_table_on_equals_the_table_off_with_hidden_submeshes(subset):
    """no exception: what the table answers is what the walk would have answered, hidden triangles or not"""
    sc0, cam = parts(), cornell_camera()
    s0, s1 = clone(sc0), clone(sc0)
    r0, r1 = rend(s0, cam, 0), rend(s1, cam, 1)
    for r in (r0, r1):
        r.set_visible(list(subset), False)
    for f, spp in ((2, 1), (3, 1), (4, 4), (5, 1)):
        a, b = frame(r0, s0, cam, f, spp), frame(r1, s1, cam, f, spp)
        assert_same_frames(a, b, f"table off / on, hidden {subset} f={f}", ties_allowed=False)
    st = r1.sun_table_stats()
    assert st["builds"] == 1 and (st["rays_answered"] > 0 or subset != (1,)), st
    r0.destroy(), r1.destroy()


# ------------------------------------------------------------------------------------------------
# 2: show restores the tree
# ------------------------------------------------------------------------------------------------
def test_hide_then_show_restores_every_node_bit_for_bit():
    """against a context that received update_transforms(geometry, its current matrix) instead: frames AND traversal counts -- which
    depend on every box -- are equal, so no slot stayed empty; whichever geometry owns leaf-order slot 0 is among the five"""
    sc0, cam = parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = rend(sa, cam, 0), rend(sn, cam, 0)
    f = 2
    for subset in SINGLES + [(1, 2), (0, 1, 2, 3, 4)]:
        idx = list(subset)
        ra.set_visible(idx, False)
        hidden = frame(ra, sa, cam, f)
        ra.set_visible(idx, True)
        rn.update_transforms(idx, np.stack([sn.geometries[i]["M"] for i in idx]))
        a, n = frame(ra, sa, cam, f + 1), frame(rn, sn, cam, f + 1)
        assert not np.isin(hidden["hits"]["geometry"][hidden["hits"]["t"] >= 0], idx).any(), subset
        assert_same_frames(a, n, f"hidden and shown {subset}", ties_allowed=False)
        assert a["stats"] == n["stats"] and a["stats"]["bounce_nodes"] > 0, (subset, a["stats"], n["stats"])
        f += 2
    ra.destroy(), rn.destroy()


# ------------------------------------------------------------------------------------------------
# 3: everything hidden
# ------------------------------------------------------------------------------------------------
def _frame_on_planes(r, sc, cam, f, planes):
    """one GI frame on a G-buffer that is uploaded, not cast: rays start on surfaces the scene no longer shows"""
    r.gi_ui.gi_samples_per_pixel, r.gi_ui.max_path_vertices = 1, 2
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
    r.svgf.upload(PLANE_ALBEDO, 0, planes["albedo"])
    r.svgf.upload(PLANE_ROUGH_METAL, 0, planes["rough_metal"])
    r.svgf.upload(PLANE_WORLDPOS, 0, planes["world_pos"])
    r.svgf.upload(PLANE_NORMAL, SLOT_CURRENT, planes["normal"])
    r.svgf.upload(PLANE_DEPTH, SLOT_CURRENT, planes["depth"])
    r.svgf.upload(PLANE_RADIANCE, -1, np.zeros((r.svgf.row_end - r.svgf.row_begin, r.width, 4), F))
    r.ray_count(reset=True)
    r.submit_commands_gi_pathtrace()
    out = dict(radiance=r.svgf.download(PLANE_RADIANCE), hits=r.download_hits(), rays=r.ray_count(), stats=r.traversal_stats())
    r.end_frame()
    return out


@pytest.mark.parametrize("sun_table", [0, 1])
def test_everything_hidden(sun_table):
    sc0, cam = parts(), cornell_camera()
    everything = list(range(5))
    sa, se, sn = clone(sc0), without(sc0, everything), clone(sc0)
    ra, re_, rn = rend(sa, cam, sun_table), rend(se, cam, sun_table), rend(sn, cam, sun_table)
    first = frame(ra, sa, cam, 2)
    planes = {k: first[k] for k in ("albedo", "world_pos", "normal", "depth")}
    planes["rough_metal"] = ra.svgf.download(PLANE_ROUGH_METAL, 0)
    builds = ra.sun_table_stats()["builds"]
    ra.set_visible(everything, False)
    lo, hi = ra.scene_box()
    assert not lo.any() and not hi.any(), (lo, hi)
    for f in (3, 4, 5):
        a, e = frame(ra, sa, cam, f), frame(re_, se, cam, f)
        assert_same_frames(a, e, f"everything hidden f={f}", ties_allowed=False)
        assert np.array_equal(_bits(a["depth"]), _bits(e["depth"])) and not np.array_equal(a["depth"], first["depth"])
        assert a["stats"]["bounce_tris"] == 0 and a["stats"]["shadow_tris"] == 0, a["stats"]
    assert ra.sun_table_stats()["builds"] == builds  # nothing visible: no table is built
    # rays that do start (a G-buffer of the full scene, uploaded): each visits the root, enters nothing and tests no triangle
    a, e = _frame_on_planes(ra, sa, cam, 6, planes), _frame_on_planes(re_, se, cam, 6, planes)
    assert a["rays"] > 0 and a["rays"] == e["rays"], (a["rays"], e["rays"])
    assert (a["hits"]["t"] < 0).all()
    assert a["stats"]["bounce_tris"] == 0 and a["stats"]["shadow_tris"] == 0, a["stats"]
    assert a["stats"]["bounce_nodes"] <= a["stats"]["rays"], a["stats"]
    assert np.array_equal(_bits(a["radiance"]), _bits(e["radiance"]))
    # showing everything again: the tree of a context that was given its own matrices
    ra.set_visible(everything, True)
    rn.update_transforms(everything, np.stack([g["M"] for g in sn.geometries]))
    same_box(ra, rn, "everything shown")
    for f, spp in SHOW_FRAMES:
        a, n = frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp)
        assert_same_frames(a, n, f"everything shown f={f}", ties_allowed=False)
        assert a["stats"]["bounce_nodes"] == n["stats"]["bounce_nodes"] and a["stats"]["bounce_tris"] == n["stats"]["bounce_tris"] > 0
    for r in (ra, re_, rn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 4: updates while hidden
# ------------------------------------------------------------------------------------------------
def _update_case(kind):
    """-> (scene, geometries the update names, apply(renderer), the updated scene, {geometry: arrays the pools hold afterwards})"""
    if kind == "transform":
        sc0 = parts()
        mats = moved_matrices(sc0, [1], world_transform("rotate"))
        return sc0, [1], lambda r: r.update_transforms([1], mats), with_matrices(sc0, [1], mats), {1: sc0.geometries[1]}
    if kind in ("vertices", "vertices_device"):
        sc0 = parts()
        d = twist_and_shear(sc0, 1)
        if kind == "vertices":
            return sc0, [1], lambda r: r.update_vertices(1, **d), with_arrays(sc0, {1: d}), {1: d}
        return sc0, [1], lambda r: r.update_vertices_device(1, **on_device(d)), with_arrays(sc0, {1: d}), {1: d}
    if kind == "skin":
        c = skin_cornell_case()
        arrays = c.skinned(0)

        def apply(r):
            c.bind(r)
            c.call(r, 0)
        return c.sc0, c.indices, apply, with_arrays(c.sc0, arrays), arrays
    if kind == "morph":
        c = morph_ref.CASES["cornell"]()
        arrays = c.morphed(0)

        def apply(r):
            c.bind(r)
            c.call(r, 0)
        return c.sc0, c.indices, apply, with_arrays(c.sc0, arrays), arrays
    raise ValueError(kind)


@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("kind", ["transform", "vertices", "vertices_device", "skin", "morph"])
def test_an_update_of_a_hidden_submesh_keeps_it_hidden_and_shows_later(kind, sun_table):
    sc0, named, apply, updated, arrays = _update_case(kind)
    cam = cornell_camera()
    sa, sb, su = clone(sc0), without(sc0, named), clone(updated)
    ra, rb, ru = rend(sa, cam, sun_table), rend(sb, cam, sun_table), rend(su, cam, sun_table)
    frame(ra, sa, cam, 2)
    ra.set_visible(named, False)
    apply(ra)
    assert not ra.visibility()[named].any()
    same_box(ra, rb, f"{kind} while hidden")
    for f, spp in HIDE_FRAMES:
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp), f"{kind} while hidden table={sun_table} f={f}")
    ra.set_visible(named, True)
    same_box(ra, ru, f"{kind} shown")
    for f, spp in SHOW_FRAMES:
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(ru, su, cam, f, spp), f"{kind} then shown table={sun_table} f={f}")
    for gi, want in arrays.items():
        for key, got in zip(KEYS, ra.download_vertices(gi)):
            assert np.array_equal(np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want[key], F).view(np.uint32)), (kind, gi, key)
    for r in (ra, rb, ru):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 5: neb_gi_build_bvh with a hidden submesh
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("subset", [(2,), (0, 3)], ids=["hide2", "hide03"])
def test_a_build_keeps_the_flags(subset, sun_table):
    sc0, cam = parts(), cornell_camera()
    sa, sb, sn = clone(sc0), without(sc0, subset), clone(sc0)
    ra, rb, rn = rend(sa, cam, sun_table), rend(sb, cam, sun_table), rend(sn, cam, sun_table)
    info, depth = ra.scene_info(), ra.bvh_depth()
    ra.set_visible(list(subset), False)
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    assert ra.scene_info() == info and ra.bvh_depth() == depth  # built over ALL triangles: the topology does not depend on the flags
    assert ra.visibility().tolist() == [k not in subset for k in range(5)]
    same_box(ra, rb, "built while hidden")
    for f, spp in HIDE_FRAMES:
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp), f"built with {subset} hidden table={sun_table} f={f}")
    ra.set_visible(list(subset), True)
    for f, spp in SHOW_FRAMES:
        a, n = frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp)
        assert_same_frames(a, n, f"built hidden, then shown {subset} table={sun_table} f={f}", ties_allowed=False)  # the same tree: no mask
        assert a["stats"]["bounce_nodes"] == n["stats"]["bounce_nodes"] and a["stats"]["bounce_tris"] == n["stats"]["bounce_tris"]
    for r in (ra, rb, rn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 6: trees that hold split references
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", ["hidden", "shown again"])
def test_a_beam_hidden_and_shown_seen_from_eight_cameras(phase):
    """the beamed room of views_ref (its beams are referenced by clipped pieces in several leaves): against a rebuild and against the
    float64 caster, test_update_views_gpu's bars, from the eight cameras of views_ref.swept_views"""
    sc0 = V.beamed_room()
    views = V.swept_views(cornell_camera())
    sa, sb = clone(sc0), (without(sc0, [V.BEAMS]) if phase == "hidden" else clone(sc0))
    ra, rb = (_motion_on(_renderer(s, views["room"], V.VW, V.VH, sun_table=0)) for s in (sa, sb))
    _assert_split(ra, sc0, "beamed room")
    ra.set_visible([V.BEAMS], False)
    if phase != "hidden":
        frame(ra, sa, views["room"], 2)
        ra.set_visible([V.BEAMS], True)
    f, tris = 4, V.triangles(sb)
    for vname, cam in views.items():
        _assert_view(_look(ra, sa, cam, f), _look(rb, sb, cam, f), sb, cam, V.VW, V.VH, f"beams {phase} / {vname}", tris)
        f += 2
    ra.destroy(), rb.destroy()


def _primary_lattice(tris, cam, w, h, step, dtype=np.float64):
    """views_ref.primary on the pixels (step // 2 + i step, step // 2 + j step) only: the float64 caster over 125 k triangles takes
    seconds for a few dozen rays -> (ys, xs, dict(geometry, covered))"""
    c = R.Camera(cam, w, h)
    ys, xs = np.meshgrid(np.arange(step // 2, h, step), np.arange(step // 2, w, step), indexing="ij")
    ndc_x = ((xs + 0.5) / w * 2.0 - 1.0).astype(dtype)
    ndc_y = (1.0 - (ys + 0.5) / h * 2.0).astype(dtype)
    xa, ya, za = [np.asarray(v, dtype) for v in (c.x, c.y, c.z)]
    d = xa * (ndc_x * dtype(c.sx))[..., None] + ya * (ndc_y * dtype(c.sy))[..., None] - za
    d = (d / np.sqrt(np.sum(d * d, -1, keepdims=True))).astype(dtype)
    out = V.cast(tris, np.asarray(c.eye, dtype), d.reshape(-1, 3), dtype=dtype)
    with np.errstate(all="ignore"):
        zv = out["t"].reshape(ys.shape) * -(d @ za)
    geometry = out["geometry"].reshape(ys.shape)
    return ys, xs, dict(geometry=geometry, covered=(geometry != V.NO_SUBMESH) & (zv >= dtype(cam.znear)) & (zv <= dtype(cam.zfar)))


@functools.lru_cache(maxsize=None)
def _longthin_reference(hidden):
    """the float64 answer on the lattice for atrium_longthin without `hidden`: computed once, shared by both table settings"""
    make, cam, w, h, _, _ = longthin()
    return _primary_lattice(V.triangles(without(make(), hidden)), cam, w, h, 32)


@pytest.mark.parametrize("sun_table", [0, 1])
def test_strips_and_beams_of_the_long_thin_atrium_hidden_and_shown(sun_table):
    """atrium_longthin: the last three submeshes with oversized triangles (two outer walls' strips and the beams); against a rebuild
    through test_refit_gpu's frames at the scene's own camera and size, and -- coverage and submesh ids on a lattice of every 32nd
    pixel -- against views_ref.cast in float64 over the triangles that are left"""
    make, cam, w, h, with_big, _ = longthin()
    sc0 = make()
    hidden = with_big[-3:]
    sa, sb, sn = clone(sc0), without(sc0, hidden), clone(sc0)
    ra, rb, rn = (_motion_on(_renderer(s, cam, w, h, sun_table=sun_table)) for s in (sa, sb, sn))
    _assert_split(ra, sc0, "atrium_longthin")
    frame(ra, sa, cam, 2)
    ra.set_visible(hidden, False)
    same_box(ra, rb, "long thin hidden")
    for f, spp in HIDE_FRAMES:
        a = frame(ra, sa, cam, f, spp)
        ids = ra.svgf.download(PLANE_SUBMESH_ID)  # (the slots turn at begin_frame: this is still the frame's)
        assert_same_frames(a, frame(rb, sb, cam, f, spp), f"long thin hidden table={sun_table} f={f}")
    ys, xs, ref = _longthin_reference(tuple(hidden))
    got = dict(covered=surface(a["depth"])[ys, xs], geometry=ids[ys, xs])
    n_wrong = int(V.differing(got, ref).sum())
    print(f"[long thin hidden table={sun_table}] against float64 on {ys.size} pixels: coverage / ids differ at {n_wrong}")
    assert not np.isin(ids, hidden).any() and int(ref["covered"].sum()) > ys.size // 2
    assert n_wrong <= TIE_CAP
    ra.set_visible(hidden, True)
    for f, spp in SHOW_FRAMES:
        # (ties allowed, node counts not compared: a leaf that held a clipped piece of a shown triangle has taken the whole triangle's bounds)
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp), f"long thin shown table={sun_table} f={f}")
    for r in (ra, rb, rn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 7: ordering
# ------------------------------------------------------------------------------------------------
def test_calls_with_two_dispatches_in_flight_on_two_streams():
    """test_refit_gpu.test_updates_with_two_dispatches_in_flight_on_two_streams with columns that come and go: the call is enqueued on a
    stream of its own while the previous frame's dispatch is in flight on a side stream, the next dispatch goes to the other side
    stream, and nothing but the library orders the three; the denoised sequence equals the serial one"""
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    flicker = [3, 11, 12, 27, 41, 58]
    outs = []
    for mode in ("plain", "two_streams"):
        sc = clone(sc0)
        r = DeferredRenderer()
        r.init(w, h, atrous_levels=4)
        main = torch.cuda.current_stream()
        sides = [torch.cuda.Stream() for _ in range(2)]
        mover = torch.cuda.Stream()
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1, stream=main.cuda_stream))
        r.submit_commands_gbuffer()
        torch.cuda.synchronize()
        for pl in (PLANE_NORMAL, PLANE_DEPTH):
            r.svgf.plane_tensor(pl, 0).copy_(r.svgf.plane_tensor(pl, 1))
        rad = [r.svgf.plane_tensor(PLANE_RADIANCE, 0), r.svgf.plane_tensor(PLANE_RADIANCE, 1)]
        direct = torch.full_like(rad[0], 0.125)
        r.svgf.set_option("gi_sun_hold", 2)
        if mode == "two_streams":
            r.set_defer_resolve(2)
        resolved = [None, None]
        for f in range(2, 16):
            if f in (4, 5, 6, 9, 13):  # (4-6: every frame; then rests, so that tables come and go as well)
                r.set_visible(flicker[:3] if f % 2 else flicker, f in (5, 13), stream=(mover if mode == "two_streams" else main).cuda_stream)
            side, slot = sides[f % 2], f % 2
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f, stream=main.cuda_stream))
            cur = r.svgf.get_current_resource_index()
            if mode == "two_streams":
                if resolved[slot] is not None:
                    side.wait_event(resolved[slot])
                r.submit_commands_gi_pathtrace(stream=side.cuda_stream)
                rad[cur].copy_(direct, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
                main.wait_event(done)
                r.submit_commands_gi_resolve()
                resolved[slot] = torch.cuda.Event()
                resolved[slot].record(main)
            else:
                rad[cur].copy_(direct, non_blocking=True)
                r.submit_commands_gi_pathtrace()
            r.submit_commands_svgf_denoising()
            r.end_frame()
        torch.cuda.synchronize()
        assert r.visibility().tolist() == [k not in flicker[3:] for k in range(len(sc0.geometries))]
        outs.append(r.svgf.download(PLANE_RADIANCE))
        r.destroy()
    assert float(np.abs(outs[0][..., :3]).max()) > 0.2
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------
# 8: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    sc0, cam = parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = rend(sa, cam), rend(sn, cam)
    for r in (ra, rn):
        r.set_visible([2], False)  # (a state that is not the initial one)
    lib, ctx = ra._lib, ra._ctx
    P32, P8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)

    def call(idx, vis, n=None):
        idx, vis = np.asarray(idx, np.uint32), np.asarray(vis, np.uint8)
        return lib.neb_gi_set_visibility(ctx, idx.ctypes.data_as(P32) if idx.size else None, vis.ctypes.data_as(P8) if vis.size else None,
                                         len(idx) if n is None else n, None)

    one32, one8 = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    cases = [("null indices", lambda: lib.neb_gi_set_visibility(ctx, None, one8.ctypes.data_as(P8), 1, None), -1),
             ("null flags", lambda: lib.neb_gi_set_visibility(ctx, one32.ctypes.data_as(P32), None, 1, None), -1),
             ("index out of range", lambda: call([1, 5], [0, 0]), -5),
             ("index far out of range", lambda: call([0xFFFFFFFF], [0]), -5),
             ("index twice", lambda: call([1, 3, 1], [0, 0, 1]), -1),
             ("more entries than geometries", lambda: call([0, 1, 2, 3, 4, 0], [0] * 6), -1),
             ("n == 0", lambda: call([], []), 0),
             ("n == 0 with pointers", lambda: call([1], [0], n=0), 0),
             ("already in that state", lambda: call([2, 1, 0], [0, 1, 7]), 0)]
    f = 2
    for what, fn, want in cases:
        assert fn() == want, what
        if want != 0:
            assert b"neb_gi_set_visibility" in lib.neb_last_error(ctx), what
        assert ra.visibility().tolist() == [True, True, False, True, True], what
        a, n = frame(ra, sa, cam, f), frame(rn, sn, cam, f)
        assert_same_frames(a, n, f"after refusal: {what}", ties_allowed=False)
        assert a["stats"] == n["stats"], what
        assert ra.sun_table_stats() == rn.sun_table_stats(), what  # (a call that changes nothing keeps the table)
        f += 1
    with pytest.raises(NebError):
        ra.set_visible([1, 1], False)
    with pytest.raises(NebError):
        ra.set_visible([1, 2], [True])
    # neb_gi_get_visibility: either output alone, a short buffer
    n_out, buf = C.c_uint32(0), np.full(8, 9, np.uint8)
    assert lib.neb_gi_get_visibility(ctx, None, 0, C.byref(n_out)) == 0 and n_out.value == 5
    assert lib.neb_gi_get_visibility(ctx, buf.ctypes.data_as(P8), 3, None) == 0 and buf.tolist() == [1, 1, 0, 9, 9, 9, 9, 9]
    assert lib.neb_gi_get_visibility(ctx, None, 3, None) == -1
    ra.destroy(), rn.destroy()
    # before a successful build: no scene at all, and a scene that has not been built; a new scene shows everything
    r = DeferredRenderer()
    r.init(VW, VH)
    args = (one32.ctypes.data_as(P32), one8.ctypes.data_as(P8), 1, None)
    assert r._lib.neb_gi_set_visibility(r._ctx, *args) == -4
    assert r._lib.neb_gi_get_visibility(r._ctx, None, 0, C.byref(n_out)) == -4
    G, ng, M, nm, T, nt = sc0.descs()
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_set_visibility(r._ctx, *args) == -4
    assert r._lib.neb_gi_build_bvh(r._ctx, None) == 0
    assert r._lib.neb_gi_set_visibility(r._ctx, *args) == 0
    assert r._lib.neb_gi_get_visibility(r._ctx, buf.ctypes.data_as(P8), 8, None) == 0 and buf.tolist() == [0, 1, 1, 1, 1, 9, 9, 9]
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_get_visibility(r._ctx, buf.ctypes.data_as(P8), 8, None) == 0 and buf.tolist() == [1, 1, 1, 1, 1, 9, 9, 9]
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 9: strips
# ------------------------------------------------------------------------------------------------
def test_two_strip_contexts_given_the_same_call_equal_the_full_frame():
    sc0, cam = parts(), cornell_camera()
    cut = 24  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = clone(sc0), clone(sc0), clone(sc0)
    full = rend(sf, cam)
    up = rend(s_up, cam, row_begin=0, row_end=cut)
    dn = rend(s_dn, cam, row_begin=cut, row_end=VH)
    for hidden, f0 in (([1, 3], 2), ([3], 4)):
        for r in (full, up, dn):
            r.set_visible([1, 3], [k not in hidden for k in (1, 3)])
        for f, spp in ((f0, 1), (f0 + 1, 4)):
            a, u, d = frame(full, sf, cam, f, spp), frame(up, s_up, cam, f, spp), frame(dn, s_dn, cam, f, spp)
            for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
                assert np.array_equal(_bits(a[name]), _bits(np.concatenate([u[name], d[name]], axis=0))), (name, f)
            assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
            assert a["rays"] == u["rays"] + d["rays"]
            assert not np.isin(a["hits"]["geometry"][a["hits"]["t"] >= 0], hidden).any()
    for r in (full, up, dn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 10: svgf_motion
# ------------------------------------------------------------------------------------------------
def test_pixels_that_showed_a_hidden_submesh_start_their_history_again():
    """option svgf_motion: the frame after a hide, every pixel that showed the hidden submesh shows another surface (or none), the
    submesh-id test rejects its tap, and its history length is 1; the expectation is tests/motion_ref.py's, fed the library's planes"""
    sc0, cam = parts(), cornell_camera()
    sc = clone(sc0)
    r = motion_renderer(VW, VH)
    planes = []
    for f in (1, 2):
        if f == 2:
            r.set_visible([1], False)
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        r.submit_commands_gbuffer()
        planes.append(tuple(r.svgf.download(p) for p in (PLANE_DEPTH, PLANE_NORMAL, PLANE_SUBMESH_ID)))
    mats = np.stack([g["M"] for g in sc.geometries])
    rad_prev, rad_cur, mom, hlen = seeded_history(VW, VH, 7)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    got = outputs(r.svgf)
    r.destroy()
    want = reference(planes, (mats, mats), cam, cam, VW, VH, rad_prev, rad_cur, mom, hlen)
    was = planes[0][2] == 1
    assert was.sum() > 50 and not (planes[1][2] == 1).any()
    keep = ~want["near"]
    assert (want["hlen"][was & keep] == 1).all()  # the reference's own answer: every tap is rejected by the id test
    assert np.array_equal(got["hlen"][keep], want["hlen"][keep])
    assert (got["hlen"][was & keep] == 1).all()
    assert np.array_equal(got["radiance"][was & keep], rad_cur[was & keep])


# ------------------------------------------------------------------------------------------------
# 11: cost
# ------------------------------------------------------------------------------------------------
def test_hiding_and_showing_every_column_costs_less_device_time_than_a_build():
    """the condition of DESIGN.md 3.4a, as test_deform_gpu asserts it for its update: all 43 columns of atrium_small in one call, hidden
    and shown, each between two events, against neb_gi_build_ms of the same context (tools/visibility_times.py records the bench scene)"""
    make, cam, w, h = scenes()["atrium_small"]
    sc = clone(make())
    r = _renderer(sc, cam, w, h, exact=False, hits=False)
    build_ms = r.build_ms()
    columns = list(ATRIUM_COLUMNS)
    assert len(columns) == 43
    times = {False: [], True: []}
    for k in range(12):
        for flag in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.set_visible(columns, flag, stream=torch.cuda.current_stream().cuda_stream)
            e1.record()
            torch.cuda.synchronize()
            times[flag].append(e0.elapsed_time(e1))
    hide, show = float(np.median(times[False][2:])), float(np.median(times[True][2:]))
    print(f"[visibility cost] 43 columns of atrium_small: hide {hide * 1e3:.0f} us, show {show * 1e3:.0f} us on the device; neb_gi_build_ms {build_ms:.2f} ms")
    assert hide < build_ms, (hide, build_ms)
    assert show < build_ms, (show, build_ms)
    r.destroy()
