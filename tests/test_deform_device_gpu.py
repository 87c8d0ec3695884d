"""neb_gi_update_vertices_device: submeshes deformed from DEVICE buffers -- validated, scattered and boxed on the GPU.

The yardstick is the host-sourced path: two contexts on one scene given the same deformation, one through update_vertices, one through
update_vertices_device, hold the same tree and render the same frames bit for bit (no tie mask: nothing was built differently).  The
boxes the device reduces are checked on their own against numpy in float32 with the bake's operation order, and against a rebuild.
No test hands a host pointer in as a device pointer: the library's check of that is read in review, not provoked here."""
import ctypes as C

import numpy as np
import pytest
import torch

from nebulae_amd import _lib, scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE
from test_deform_gpu import ATRIUM_COLUMNS, ATRIUM_GRIDS, CASES, KEYS, atrium_case, clone, cornell_case, shaped, sine_along_normal, \
    twist_and_shear, update, with_arrays
from test_refit_gpu import H, _free_bytes, assert_same_frames, frame, make_renderer, moved_matrices, world_transform

pytestmark = pytest.mark.gpu

F = np.float32


def _renderer(*a, **k):
    r = make_renderer(*a, **k)
    r._hits_on = k.get("hits", True)
    return r


def on_device(kw):
    return {k: (torch.from_numpy(np.ascontiguousarray(v, F)).cuda() if k in KEYS else v) for k, v in kw.items()}


def update_device(r, calls, stream=None, mirror=True):
    for gi, kw in calls.items():
        r.update_vertices_device(gi, stream=stream, mirror=mirror, **on_device(kw))


def dev_entry(gi, positions, normals=None, tangents=None, first=0, n=None, strides=None):
    """one neb_vertex_update over device tensors (the caller keeps them alive)"""
    u = _lib.VertexUpdate(geometry=gi, firstVertex=first, numVertices=(positions.shape[0] if n is None else n))
    for k, (key, t, width) in enumerate((("positions", positions, 3), ("normals", normals, 3), ("tangents", tangents, 4))):
        if t is not None:
            setattr(u, key, t.data_ptr())
        setattr(u, key[:-1] + "Stride", 4 * width if strides is None else strides[k])
    return u


def same_frames(ra, sa, rb, sb, cam, what, frames=((5, 1, 2), (6, 4, 2), (7, 1, 4)), shadow_stats=False):
    for f, spp, mpv in frames:
        a, b = frame(ra, sa, cam, f, spp, mpv), frame(rb, sb, cam, f, spp, mpv)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_same_frames(a, b, f"{what} spp={spp} mpv={mpv}", ties_allowed=False, hits_visible=(mpv == 2))
        # (the same tree: the same walks.  With a table, which pass takes the shadow rays it leaves is decided by a measurement.)
        for key in ("rays", "bounce_nodes", "bounce_tris") + (("shadow_nodes", "shadow_tris") if shadow_stats else ()):
            assert a["stats"][key] == b["stats"][key], (what, key, a["stats"], b["stats"])


# ------------------------------------------------------------------------------------------------
# 1: device sources == host sources, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("shape", ["all", "positions", "partial"])
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_device_sources_equal_host_sources_bit_for_bit(name, shape, sun_table):
    sc0, cam, w, h, deform = CASES[name]()
    calls, arrays = shaped(sc0, deform, shape)
    sa, sb = clone(sc0), clone(sc0)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    frame(ra, sa, cam, 2), frame(rb, sb, cam, 2)
    update(ra, calls), update_device(rb, calls)
    assert all(np.array_equal(sb.geometries[gi][k], arrays[gi][k]) for gi in arrays for k in KEYS)  # mirror=True: the scene object followed
    if sun_table:  # the hold is two dispatches on both: the device context waits for its boxes where the table is built
        for f in (3, 4):
            frame(ra, sa, cam, f), frame(rb, sb, cam, f)
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 2
    same_frames(ra, sa, rb, sb, cam, f"device == host {name} {shape} table={sun_table}", shadow_stats=not sun_table)
    assert rb.update_status() == {"accepted": len(calls), "refused": 0}
    lo_a, hi_a = ra.scene_box()
    lo_b, hi_b = rb.scene_box()
    assert np.array_equal(lo_a, lo_b) and np.array_equal(hi_a, hi_b)
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 2: device-sourced update == rebuild (the boxes are conservative whatever the host path does)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_a_device_sourced_deformation_equals_a_rebuild(name, sun_table):
    sc0, cam, w, h, deform = CASES[name]()
    calls, arrays = shaped(sc0, deform, "all")
    sa, sb = clone(sc0), with_arrays(sc0, arrays)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    depth, info = ra.bvh_depth(), ra.scene_info()
    frame(ra, sa, cam, 2)
    update_device(ra, calls)
    assert ra.bvh_depth() == depth and ra.scene_info() == info
    if sun_table:
        for f in (3, 4):
            frame(ra, sa, cam, f), frame(rb, sb, cam, f)
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 1
    for f, spp, mpv in ((5, 1, 2), (6, 4, 2), (7, 1, 4)):
        a, b = frame(ra, sa, cam, f, spp, mpv), frame(rb, sb, cam, f, spp, mpv)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_same_frames(a, b, f"device deform == rebuild {name} table={sun_table} spp={spp} mpv={mpv}", hits_visible=(mpv == 2))
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 3: the boxes
# ------------------------------------------------------------------------------------------------
def numpy_scene_box(sc):
    """the union of the submeshes' world boxes over their REFERENCED vertices, float32, gi_bake_point's order: products and sums rounded
    one by one, left to right"""
    lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for g in sc.geometries:
        idx = np.unique(np.asarray(g["indices"]).astype(np.int64))
        if idx.size == 0:
            continue
        P, M = np.ascontiguousarray(g["positions"], F)[idx], np.ascontiguousarray(g["M"], F)
        Wd = np.stack([((P[:, 0] * M[0, c] + P[:, 1] * M[1, c]) + P[:, 2] * M[2, c]) + M[3, c] for c in range(3)], 1)
        assert Wd.dtype == F
        lo, hi = np.minimum(lo, Wd.min(0)), np.maximum(hi, Wd.max(0))
    return lo, hi


def assert_box(r, sc, what):
    lo, hi = r.scene_box()
    want_lo, want_hi = numpy_scene_box(sc)
    print(f"[box {what}] {lo} .. {hi}")
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (what, lo, hi, want_lo, want_hi)  # (numeric: -0 == +0)
    return lo, hi


def test_the_scene_box_reduced_on_the_device_is_the_exact_box_of_the_referenced_vertices():
    sc0, cam, w, h, _ = cornell_case()
    g1 = sc0.geometries[1]
    stray = {k: np.concatenate([g1[k], g1[k][:1]]) for k in KEYS + ("uvs",)}
    stray["positions"][-1] = (40.0, -55.0, 70.0)  # a vertex no triangle names, far outside the room: no part of any box
    sc0.geometries[1] = dict(g1, **stray)
    sa = clone(sc0)
    r = _renderer(sa, cam, w, h)
    lo0, hi0 = assert_box(r, sa, "as set (folded on the host)")
    assert np.abs(np.concatenate([lo0, hi0])).max() < 10.0
    P = stray["positions"].astype(np.float64)
    c = P[:-1].mean(0)
    grown = np.ascontiguousarray(np.concatenate([c + 4.0 * (P[:-1] - c), P[-1:]]), F)
    r.update_vertices_device(1, torch.from_numpy(grown).cuda())
    lo1, hi1 = assert_box(r, sa, "grown on the device")
    assert (lo1 < lo0).any() and (hi1 > hi0).any()
    r.update_vertices_device(1, torch.from_numpy(stray["positions"]).cuda())
    lo2, hi2 = assert_box(r, sa, "shrunk back on the device")
    assert np.array_equal(lo2, lo0) and np.array_equal(hi2, hi0)
    T = np.eye(4)
    T[3, :3] = (3.5, 0.25, -2.75)
    r.update_transforms([1], moved_matrices(sc0, [1], T))  # (its h_pos is stale: corners checked, box from the device)
    lo3, hi3 = assert_box(r, sa, "a transform of the stale submesh")
    assert hi3[0] > hi0[0]
    n = P.shape[0] - 1
    first, count = n // 4, n // 2
    part = np.ascontiguousarray(c + 2.5 * (P[first:first + count] - c), F)
    r.update_vertices(1, part, first_vertex=first)  # host-sourced, partial, on the stale submesh
    assert_box(r, sa, "a host-sourced partial range on the stale submesh")
    assert r.update_status() == {"accepted": 2, "refused": 0}
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 4: strided and partial sources
# ------------------------------------------------------------------------------------------------
def test_strided_views_of_one_interleaved_buffer_equal_contiguous_sources():
    sc0, cam, w, h, deform = cornell_case()
    d = deform[1]
    n = d["positions"].shape[0]
    first, count = n // 4, n // 2
    inter = torch.from_numpy(np.concatenate([d[k][first:first + count] for k in KEYS], axis=1)).cuda()
    assert inter.shape == (count, 10)
    views = dict(positions=inter[:, 0:3], normals=inter[:, 3:6], tangents=inter[:, 6:10])
    assert all(v.stride(0) == 10 and not v.is_contiguous() for v in views.values())
    sa, sb = clone(sc0), clone(sc0)
    ra, rb = _renderer(sa, cam, w, h), _renderer(sb, cam, w, h)
    ra.update_vertices_device(1, first_vertex=first, **views)
    rb.update_vertices_device(1, first_vertex=first, **{k: v.contiguous() for k, v in views.items()})
    assert all(np.array_equal(sa.geometries[1][k], sb.geometries[1][k]) for k in KEYS)
    assert not np.array_equal(sa.geometries[1]["positions"], sc0.geometries[1]["positions"])
    same_frames(ra, sa, rb, sb, cam, "strided == contiguous", frames=((2, 1, 2), (3, 4, 2)))
    assert ra.update_status() == {"accepted": 1, "refused": 0}
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 5: composition, a build afterwards, and back again
# ------------------------------------------------------------------------------------------------
def test_a_device_update_then_a_transform_then_a_host_partial_update_equal_the_final_scene():
    sc0, cam, w, h, deform = cornell_case()
    calls, arrays = shaped(sc0, deform, "all")
    mats = moved_matrices(sc0, [1], world_transform("translate"))
    mild = twist_and_shear(sc0, 1, 12.0, 0.04)
    part, _ = shaped(sc0, {1: mild}, "partial")
    final = {1: {k: arrays[1][k].copy() for k in KEYS}}
    f0 = part[1]["first_vertex"]
    for k in KEYS:
        final[1][k][f0:f0 + part[1][k].shape[0]] = part[1][k]
    sb = with_arrays(sc0, final, {1: mats[0]})
    sa = clone(sc0)
    ra, rb = _renderer(sa, cam, w, h), _renderer(sb, cam, w, h)
    update_device(ra, calls), ra.update_transforms([1], mats), update(ra, part)
    assert all(np.array_equal(sa.geometries[1][k], sb.geometries[1][k]) for k in KEYS + ("M",))
    for f, spp in ((2, 1), (3, 1), (4, 4)):
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp), f"device, transform, host partial spp={spp}")
    lo, hi = ra.scene_box()
    want = numpy_scene_box(sb)
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
    ra.destroy(), rb.destroy()


@pytest.mark.parametrize("sun_table", [0, 1])
def test_a_build_after_a_device_sourced_deformation_reads_the_positions_back(sun_table):
    sc0, cam, w, h, deform = atrium_case()
    calls, arrays = shaped(sc0, deform, "all")
    sa, sb = clone(sc0), with_arrays(sc0, arrays)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    update_device(ra, calls, mirror=False)
    assert all(np.array_equal(sa.geometries[gi][k], sc0.geometries[gi][k]) for gi in arrays for k in KEYS)  # mirror=False: untouched
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    assert ra.scene_info() == rb.scene_info() and ra.bvh_depth() == rb.bvh_depth()
    for f, spp in ((2, 1), (3, 4)):
        a, b = frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp)
        assert_same_frames(a, b, f"rebuilt after a device deformation table={sun_table} spp={spp}", ties_allowed=False)
        for key in ("rays", "bounce_nodes", "bounce_tris") + (("shadow_nodes", "shadow_tris") if not sun_table else ()):
            assert a["stats"][key] == b["stats"][key], (key, a["stats"], b["stats"])
    ra.destroy(), rb.destroy()


def test_deforming_on_the_device_and_back_restores_every_node_bit_for_bit():
    sc0, cam, w, h, deform = cornell_case()
    calls, _ = shaped(sc0, deform, "all")
    back = {gi: {k: sc0.geometries[gi][k] for k in KEYS} for gi in deform}
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, w, h, sun_table=0), _renderer(sn, cam, w, h, sun_table=0)
    update_device(ra, calls)
    moved = frame(ra, sa, cam, 2)
    update_device(ra, back)
    a, n = frame(ra, sa, cam, 3), frame(rn, sn, cam, 3)
    assert not np.array_equal(moved["depth"], a["depth"])
    assert_same_frames(a, n, "deformed on the device and back", ties_allowed=False)
    assert a["stats"] == n["stats"]  # (the traversal counts do depend on the boxes)
    ra.destroy(), rn.destroy()


# ------------------------------------------------------------------------------------------------
# 6: refused on the device
# ------------------------------------------------------------------------------------------------
def test_a_source_that_is_not_finite_is_refused_on_the_device_and_changes_nothing():
    sc0, cam, w, h, deform = cornell_case()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, w, h), _renderer(sn, cam, w, h)
    scaled = moved_matrices(sc0, [2], world_transform("scale"))  # (3e38 is finite, its world position under this matrix is not)
    ra.update_transforms([2], scaled), rn.update_transforms([2], scaled)
    d, d2 = deform[1], twist_and_shear(sc0, 2, 10.0, 0.02)
    nan = d["positions"].copy()
    nan[5, 1] = np.nan
    far = d2["positions"].copy()
    far[3] = (3.0e38, 3.0e38, 3.0e38)
    frame(ra, sa, cam, 2), frame(rn, sn, cam, 2)
    box = ra.scene_box()
    assert ra.update_status() == {"accepted": 0, "refused": 0}
    f = 3
    for k, (what, gi, bad, dd) in enumerate((("nan", 1, nan, d), ("world position not finite", 2, far, d2))):
        ra.update_vertices_device(gi, torch.from_numpy(bad).cuda(), normals=torch.from_numpy(dd["normals"]).cuda(), mirror=False)  # NEB_OK
        assert ra.update_status() == {"accepted": 0, "refused": k + 1}, what
        after = ra.scene_box()
        assert np.array_equal(after[0], box[0]) and np.array_equal(after[1], box[1]), what
        for spp in (1, 4):
            assert_same_frames(frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp), f"refused on the device: {what} spp={spp}", ties_allowed=False)
            f += 1
    calls, _ = shaped(sc0, {1: d}, "all")
    update_device(ra, calls), update(rn, calls)
    assert ra.update_status() == {"accepted": 1, "refused": 2}
    for spp in (1, 4):
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp), f"valid after refusals spp={spp}", ties_allowed=False)
        f += 1
    ra.destroy(), rn.destroy()


# ------------------------------------------------------------------------------------------------
# 7: refusals at the call
# ------------------------------------------------------------------------------------------------
def test_refusals_at_the_call_change_nothing():
    sc0, cam, w, h, deform = cornell_case()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, w, h), _renderer(sn, cam, w, h)
    lib, ctx = ra._lib, ra._ctx
    d, d2 = on_device(deform[1]), on_device(twist_and_shear(sc0, 2, 10.0, 0.02))
    nv = d["positions"].shape[0]
    wide = torch.zeros((nv, 4), dtype=torch.float32, device="cuda")  # rows of 16 bytes: room for a 14-byte stride and a pointer + 2

    def call(*entries):
        arr = (_lib.VertexUpdate * len(entries))(*entries)
        return lib.neb_gi_update_vertices_device(ctx, arr, len(entries), None)

    def E(gi, dd, **k):
        return dev_entry(gi, dd["positions"], dd["normals"], dd["tangents"], **k)

    no_pos = E(1, d)
    no_pos.positions = None
    off2 = dev_entry(1, wide, strides=(16, 12, 16))
    off2.positions = wide.data_ptr() + 2
    cases = [("null positions", lambda: call(E(2, d2), no_pos), -1),
             ("range beyond numVertices", lambda: call(E(2, d2), E(1, d, first=1)), -1),
             ("overlapping ranges", lambda: call(dev_entry(1, d["positions"][:10]), E(2, d2), dev_entry(1, d["positions"][9:20], first=9)), -1),
             ("position stride below the element", lambda: call(E(2, d2), E(1, d, strides=(8, 12, 16))), -1),
             ("tangent stride below the element", lambda: call(E(1, d, strides=(12, 12, 12))), -1),
             ("position stride no multiple of 4", lambda: call(dev_entry(1, wide, strides=(14, 12, 16))), -1),
             ("normal stride no multiple of 4", lambda: call(E(1, d, strides=(12, 13, 16))), -1),
             ("pointer no multiple of 4", lambda: call(E(2, d2), off2), -1)]
    status = ra.update_status()
    f = 2
    for what, fn, want in cases:
        assert fn() == want, what
        assert b"neb_gi_update_vertices_device" in lib.neb_last_error(ctx), what
        a, n = frame(ra, sa, cam, f), frame(rn, sn, cam, f)
        assert_same_frames(a, n, f"after refusal: {what}", ties_allowed=False)
        assert a["stats"] == n["stats"] and ra.sun_table_stats() == rn.sun_table_stats(), what
        assert ra.update_status() == status, what
        f += 1
    ra.destroy(), rn.destroy()
    # normals for a geometry that was set without an attribute stream; positions alone are accepted
    sv = S.Scene("no-tangents")
    sv.add_material(albedo=(0.5, 0.5, 0.5, 1))
    g1 = sc0.geometries[1]
    sv.add_geometry(g1["positions"], g1["normals"], g1["uvs"], g1["indices"], material=0, M=g1["M"], omit=("tangents",))
    r = _renderer(sv, cam, 64, 48)
    lib, ctx = r._lib, r._ctx
    assert call(dev_entry(0, d["positions"], d["normals"])) == -1 and b"neb_gi_update_vertices_device" in lib.neb_last_error(ctx)
    assert r.update_status() == {"accepted": 0, "refused": 0}
    assert call(dev_entry(0, d["positions"])) == 0
    assert r.update_status() == {"accepted": 1, "refused": 0}
    r.destroy()
    # before a successful build
    r = DeferredRenderer()
    r.init(64, 48)
    u = dev_entry(1, d["positions"])
    assert r._lib.neb_gi_update_vertices_device(r._ctx, C.byref(u), 1, None) == -4
    G, ng, M, nm, T, nt = sc0.descs()
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_update_vertices_device(r._ctx, C.byref(u), 1, None) == -4
    assert b"neb_gi_update_vertices_device" in r._lib.neb_last_error(r._ctx)
    assert r.update_status() == {"accepted": 0, "refused": 0}
    assert r._lib.neb_gi_build_bvh(r._ctx, None) == 0
    assert r._lib.neb_gi_update_vertices_device(r._ctx, C.byref(u), 1, None) == 0
    assert r.update_status() == {"accepted": 1, "refused": 0}
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 8: streams
# ------------------------------------------------------------------------------------------------
def test_device_sourced_updates_with_two_dispatches_in_flight_on_two_streams():
    """test_deform_gpu.test_vertex_updates_with_two_dispatches_in_flight_on_two_streams with the sources written by a torch kernel on a
    third stream: an event orders the update's stream behind the producer, the library orders everything else.  Every frame equals the
    serial context's, which takes the same arrays through the host-sourced call."""
    sc0, cam, w, h, _ = atrium_case([])
    outs = []
    for mode in ("plain", "two_streams"):
        sc = clone(sc0)
        r = DeferredRenderer()
        r.init(w, h, atrous_levels=4)
        main = torch.cuda.current_stream()
        sides = [torch.cuda.Stream() for _ in range(2)]
        mover, producer = torch.cuda.Stream(), torch.cuda.Stream()
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
        frames, keep = [], []
        for f in range(2, 11):
            if f in (4, 5, 6, 7):
                gi = ATRIUM_GRIDS[f % 4]
                d = sine_along_normal(sc0, gi, amplitude=2.0 + f, phase=0.3 * f)
                if mode == "two_streams":
                    staged = {k: torch.from_numpy(d[k]).pin_memory() for k in KEYS}
                    with torch.cuda.stream(producer):
                        src = {k: v.cuda(non_blocking=True) * 1.0 for k, v in staged.items()}  # (an exact product: the same bits)
                        ready = torch.cuda.Event()
                        ready.record(producer)
                    mover.wait_event(ready)
                    r.update_vertices_device(gi, stream=mover.cuda_stream, mirror=False, **src)
                    keep.append((staged, src))  # (alive until the device has passed the update)
                else:
                    r.update_vertices(gi, stream=main.cuda_stream, **d)
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
            frames.append(rad[cur].clone())
            r.end_frame()
        torch.cuda.synchronize()
        if mode == "two_streams":
            assert r.update_status() == {"accepted": 4, "refused": 0}
        outs.append([t.cpu().numpy() for t in frames])
        r.destroy()
    assert float(np.abs(outs[0][-1][..., :3]).max()) > 0.2
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), f"frame {k + 2}"


# ------------------------------------------------------------------------------------------------
# 9, 10: memory, cost
# ------------------------------------------------------------------------------------------------
def _device_update_many(sc0, indices, amplitude, phase, keep):
    """the entries of ONE call for many submeshes, positions + normals in device memory"""
    entries = []
    for gi in indices:
        d = sine_along_normal(sc0, gi, amplitude=amplitude, phase=phase)
        p, n = torch.from_numpy(d["positions"]).cuda(), torch.from_numpy(d["normals"]).cuda()
        keep.append((p, n))
        entries.append(dev_entry(gi, p, n))
    return (_lib.VertexUpdate * len(entries))(*entries)


def test_a_hundred_device_sourced_updates_hold_no_more_device_memory():
    sc0, cam, w, h, _ = atrium_case([])
    sc = clone(sc0)
    r = _renderer(sc, cam, w, h, exact=False, hits=False)
    keep = []
    poses = [_device_update_many(sc0, ATRIUM_COLUMNS[::3], 3.0 + k, 0.7 * k, keep) for k in range(4)]
    torch.cuda.synchronize()
    free = {}
    for k in range(104):
        arr = poses[k % 4]
        r._check(r._lib.neb_gi_update_vertices_device(r._ctx, arr, len(arr), None), "neb_gi_update_vertices_device")
        if k % 4 == 0 or 40 <= k < 50:
            out = frame(r, sc, cam, 2 + k)
            assert np.isfinite(out["radiance"]).all()
        if k in (3, 103):
            free[k] = _free_bytes()
    print(f"[device deform soak] free device memory after update 4 / 104: {free[3] >> 20} / {free[103] >> 20} MB; {r.update_status()}")
    assert free[3] - free[103] < 4 << 20, free  # test_refit_gpu's bar: steady state allocates nothing
    assert r.update_status() == {"accepted": 104, "refused": 0}
    r.destroy()


def test_a_device_sourced_deformation_costs_less_device_time_than_a_build():
    """the project's condition for a refit for the device-sourced chain: every column of atrium_small in one call"""
    sc0, cam, w, h, _ = atrium_case([])
    r = _renderer(clone(sc0), cam, w, h, exact=False, hits=False)
    build_ms = r.build_ms()
    keep = []
    poses = [_device_update_many(sc0, ATRIUM_COLUMNS, 4.0 + k, 0.5 * k, keep) for k in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    times = []
    for k in range(22):
        arr = poses[k % 2]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r._check(r._lib.neb_gi_update_vertices_device(r._ctx, arr, len(arr), C.c_void_p(st)), "neb_gi_update_vertices_device")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times[2:]))
    print(f"[device deform cost] update of {len(ATRIUM_COLUMNS)} submeshes from device memory: {med * 1e3:.0f} us on the device; neb_gi_build_ms {build_ms:.2f} ms")
    assert med < build_ms, (med, build_ms)
    assert r.update_status() == {"accepted": 22, "refused": 0}
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 11: strips
# ------------------------------------------------------------------------------------------------
def test_two_strip_contexts_given_the_same_device_sourced_deformation_equal_the_full_frame():
    sc0, cam, w, h, deform = cornell_case()
    calls, _ = shaped(sc0, deform, "all")
    cut = 88  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = clone(sc0), clone(sc0), clone(sc0)
    full = _renderer(sf, cam)
    up = _renderer(s_up, cam, row_begin=0, row_end=cut)
    dn = _renderer(s_dn, cam, row_begin=cut, row_end=H)
    for r in (full, up, dn):
        update_device(r, calls)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], x.shape[1], -1)
    for f, spp in ((2, 1), (3, 4)):
        a, u, d = frame(full, sf, cam, f, spp), frame(up, s_up, cam, f, spp), frame(dn, s_dn, cam, f, spp)
        for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
            assert np.array_equal(bits(a[name]), bits(np.concatenate([u[name], d[name]], axis=0))), (name, f)
        assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
        assert a["rays"] == u["rays"] + d["rays"]
    for r in (full, up, dn):
        r.destroy()
