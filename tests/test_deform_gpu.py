"""neb_gi_update_vertices: submeshes deformed per vertex, the BVH refitted in place, the shading records rewritten.

As in test_refit_gpu.py, a refitted tree renders what a tree built from the deformed scene renders, bit for bit, up to exact ties
between coincident hits (TIE_CAP, taken from there unchanged).  Scenes: the Cornell parts at the refit tests' size, with the short box
twisted about its vertical axis and sheared; atrium_small, with a sine displacement along the normal on some of its grid submeshes
(that scene's 60 submeshes are 17 planes and 43 columns: the stand-in's drapes come after them and exist only in the bench scene, so
the columns -- grids of 40 x 24 cells, like the drapes' 48 x 40 -- stand in for them here).  Normals are recomputed from the deformed
grid, tangents come from scene.generate_tangents."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nebulae_amd import _lib, scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import NebError, PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE
from oracle_lib import OracleTracer
from svgf_cases import rel_l2
from test_gi_gpu import scenes, upload_gbuffer
from test_refit_gpu import H, W, _free_bytes, assert_same_frames, cornell_camera, cornell_parts, frame, make_renderer, \
    moved_matrices, world_transform

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("positions", "normals", "tangents")
ATRIUM_GRIDS = [3, 27, 41, 58]                # a gallery floor and three columns of atrium_small
ATRIUM_COLUMNS = list(range(17, 60))          # every column of atrium_small (see the module docstring)


# ------------------------------------------------------------------------------------------------
# deformations
# ------------------------------------------------------------------------------------------------
def vertex_normals(P, I, like):
    """area-weighted vertex normals of the deformed mesh, on the side of the normals it had"""
    tri = np.asarray(I).reshape(-1, 3).astype(np.int64)
    P = P.astype(np.float64)
    fn = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    N = np.zeros_like(P)
    for k in range(3):
        np.add.at(N, tri[:, k], fn)
    N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-30)
    N *= np.where(np.sum(N * like, axis=1, keepdims=True) < 0.0, -1.0, 1.0)
    return np.ascontiguousarray(N, F)


def _finish(g, P):
    P = np.ascontiguousarray(P, F)
    N = vertex_normals(P, g["indices"], g["normals"])
    return dict(positions=P, normals=N, tangents=S.generate_tangents(P, N, g["uvs"], g["indices"]))


def twist_and_shear(sc, gi, angle_deg=25.0, shear=0.1):
    """a box twisted about the vertical axis through its centre (nothing at its foot, angle_deg at its top) and sheared along z;
    worked in world space and taken back to the submesh's object space"""
    g = sc.geometries[gi]
    M = g["M"].astype(np.float64)
    Pw = g["positions"].astype(np.float64) @ M[:3, :3] + M[3, :3]
    lo, hi = Pw.min(0), Pw.max(0)
    c = 0.5 * (lo + hi)
    a = math.radians(angle_deg) * (Pw[:, 1] - lo[1]) / (hi[1] - lo[1])
    x, z = Pw[:, 0] - c[0], Pw[:, 2] - c[2]
    Q = np.stack([c[0] + x * np.cos(a) + z * np.sin(a), Pw[:, 1], c[2] - x * np.sin(a) + z * np.cos(a) + shear * (Pw[:, 1] - lo[1])], 1)
    Minv = np.linalg.inv(M)
    return _finish(g, Q @ Minv[:3, :3] + Minv[3, :3])


def sine_along_normal(sc, gi, amplitude=6.0, wavelength=130.0, phase=0.0):
    """object units of the atrium (0.008 world units each): 6 units = 5 cm on cells of 7 x 20 units and more -- no triangle
    degenerates, and no displaced surface reaches a neighbour (the gallery's underside lies 20 units below its floor).  The phase is
    a function of the position alone: the duplicated vertices of a column's seam move together."""
    g = sc.geometries[gi]
    P, N = g["positions"].astype(np.float64), g["normals"].astype(np.float64)
    d = amplitude * np.sin(2.0 * math.pi / wavelength * (P @ np.array([0.55, 1.0, 0.35])) + phase)
    return _finish(g, P + d[:, None] * N)


def with_arrays(sc, arrays, mats=None):
    """a copy of the scene (everything else shared) with the named geometries' vertex arrays -- and matrices -- replaced"""
    out = S.Scene(sc.name + "-deformed")
    out.materials, out.textures = sc.materials, sc.textures
    out.geometries = [dict(g) for g in sc.geometries]
    for gi, a in arrays.items():
        out.geometries[gi].update({k: np.ascontiguousarray(v, F) for k, v in a.items()})
    for gi, m in (mats or {}).items():
        out.geometries[gi]["M"] = np.ascontiguousarray(m, F)
    return out


def clone(sc):
    return with_arrays(sc, {})


def shaped(sc, deform, shape):
    """-> ({gi: keyword arguments of update_vertices}, {gi: the arrays a scene rebuilt from the result holds})"""
    calls, arrays = {}, {}
    for gi, d in deform.items():
        g = sc.geometries[gi]
        if shape == "all":
            calls[gi] = dict(positions=d["positions"], normals=d["normals"], tangents=d["tangents"])
        elif shape == "positions":
            calls[gi] = dict(positions=d["positions"])
        elif shape == "partial":
            n = d["positions"].shape[0]
            first, count = n // 4, n // 2
            calls[gi] = dict(first_vertex=first, **{k: d[k][first:first + count] for k in KEYS})
        else:
            raise ValueError(shape)
        first = calls[gi].get("first_vertex", 0)
        arrays[gi] = {}
        for k in KEYS:
            full = g[k].copy()
            if k in calls[gi]:
                full[first:first + calls[gi][k].shape[0]] = calls[gi][k]
            arrays[gi][k] = full
    return calls, arrays


def update(r, calls, stream=None):
    for gi, kw in calls.items():
        r.update_vertices(gi, stream=stream, **kw)


def _renderer(*a, **k):
    r = make_renderer(*a, **k)
    r._hits_on = k.get("hits", True)
    return r


def _checked(sc0, deform, least_move):
    """(no degenerate triangle before or after, and a deformation that does move positions and normals)"""
    for gi, d in deform.items():
        g = sc0.geometries[gi]
        tri = g["indices"].reshape(-1, 3).astype(np.int64)
        for P in (g["positions"], d["positions"]):
            area = 0.5 * np.linalg.norm(np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]), axis=1)
            assert area.min() > 1e-3 * area.mean(), gi
        assert np.abs(d["positions"] - g["positions"]).max() > least_move
        assert np.abs(d["normals"] - g["normals"]).max() > 0.1
        assert np.isfinite(d["tangents"]).all() and np.abs(np.linalg.norm(d["normals"], axis=1) - 1.0).max() < 1e-5
    return deform


def cornell_case():
    sc0 = cornell_parts()
    return sc0, cornell_camera(), W, H, _checked(sc0, {1: twist_and_shear(sc0, 1)}, 0.05)


def atrium_case(indices=ATRIUM_GRIDS):
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    return sc0, cam, w, h, _checked(sc0, {gi: sine_along_normal(sc0, gi, phase=0.4 * k) for k, gi in enumerate(indices)}, 3.0)


CASES = {"cornell": cornell_case, "atrium_small": atrium_case}


# ------------------------------------------------------------------------------------------------
# 1, 2: deform == rebuild, in the three shapes of an update
# ------------------------------------------------------------------------------------------------
def _deform_against_rebuild(case, shape, sun_table, tag):
    sc0, cam, w, h, deform = case()
    calls, arrays = shaped(sc0, deform, shape)
    sa, sb = clone(sc0), with_arrays(sc0, arrays)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    depth, info = ra.bvh_depth(), ra.scene_info()
    frame(ra, sa, cam, 2)  # (a dispatch before the update: with the table on, it exists and is then invalidated)
    update(ra, calls)
    assert ra.bvh_depth() == depth and ra.scene_info() == info  # the tree is kept
    assert all(np.array_equal(sa.geometries[gi][k], sb.geometries[gi][k]) for gi in arrays for k in KEYS)  # the renderer's scene followed
    if sun_table:  # both contexts get to a table of the deformed scene: the hold is two dispatches
        for f in (3, 4):
            frame(ra, sa, cam, f), frame(rb, sb, cam, f)
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 1
    for f, spp, mpv in ((5, 1, 2), (6, 4, 2), (7, 1, 4)):
        a, b = frame(ra, sa, cam, f, spp, mpv), frame(rb, sb, cam, f, spp, mpv)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_same_frames(a, b, f"{tag} {shape} table={sun_table} spp={spp} mpv={mpv}", hits_visible=(mpv == 2))
    ra.destroy(), rb.destroy()


@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_deform_equals_rebuild(name, sun_table):
    _deform_against_rebuild(CASES[name], "all", sun_table, name)


@pytest.mark.parametrize("shape", ["positions", "partial"])
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_an_update_of_positions_only_and_of_a_partial_range_equal_a_rebuild(name, shape):
    """positions only: the rebuilt scene keeps the OLD normals and tangents on the new positions -- the records of the updated context
    must have kept them too.  partial: firstVertex > 0, half the vertices, every stream supplied."""
    _deform_against_rebuild(CASES[name], shape, 1, name)


# ------------------------------------------------------------------------------------------------
# 3: the records are rewritten
# ------------------------------------------------------------------------------------------------
def test_the_shading_normals_of_the_records_are_rewritten():
    """Three contexts: A updated with normals and tangents, C with positions only, B rebuilt from the deformed arrays.  A and C hold the
    same geometry (equal depth), so where their shading normals (normal.zw) differ, only the record rewrite made the difference: that
    set must be a good part of the box -- an update that rewrote nothing would leave it empty -- and there A also differs from its own
    frame before the update, and equals B bit for bit."""
    sc0, cam, w, h, deform = cornell_case()
    calls, arrays = shaped(sc0, deform, "all")
    pos_only, _ = shaped(sc0, deform, "positions")
    sa, sc_, sb = clone(sc0), clone(sc0), with_arrays(sc0, arrays)
    ra, rc, rb = (_renderer(s, cam, w, h, sun_table=0) for s in (sa, sc_, sb))
    before = frame(ra, sa, cam, 2)
    frame(rc, sc_, cam, 2), frame(rb, sb, cam, 2)
    update(ra, calls), update(rc, pos_only)
    a, c, b = frame(ra, sa, cam, 3), frame(rc, sc_, cam, 3), frame(rb, sb, cam, 3)
    sn = lambda fr: np.ascontiguousarray(fr["normal"]).view(np.uint16).reshape(h, w, 4)[..., 2:]
    assert np.array_equal(a["depth"], c["depth"])
    rewritten = (sn(a) != sn(c)).any(-1)
    on_box = a["depth"] != before["depth"]  # (pixels the box entered or left, or where its surface moved)
    print(f"[records] shading normal differs from the positions-only context at {int(rewritten.sum())} px; depth moved at {int(on_box.sum())} px")
    assert int(rewritten.sum()) > 200
    changed = (sn(a) != sn(before)).any(-1)
    assert changed[rewritten].mean() > 0.5
    assert np.array_equal(np.ascontiguousarray(a["normal"]).view(np.uint16), np.ascontiguousarray(b["normal"]).view(np.uint16))
    for r in (ra, rc, rb):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 4: the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_a_deformed_context_matches_the_oracle_on_the_deformed_scene(name):
    """test_refit_gpu.test_an_updated_context_matches_the_oracle_on_the_moved_scene, at its bars, for a context that reached the scene
    through a vertex update"""
    sc0, cam, w, h, deform = CASES[name]()
    calls, arrays = shaped(sc0, deform, "all")
    sa = clone(sc0)
    r = DeferredRenderer()
    r.init(w, h, atrous_levels=4)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=4))
    update(r, calls)
    sm = with_arrays(sc0, arrays)
    o = OracleTracer(sm)
    assert all(np.array_equal(g[k], q[k]) for g, q in zip(sa.geometries, sm.geometries) for k in KEYS)
    gb = o.gbuffer(w, h, cam)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=5))
    r.submit_commands_gbuffer()
    d = r.svgf.download(PLANE_DEPTH)
    covered = (d >> 24) == (gb["depth"] >> 24)
    assert covered.mean() >= 1.0 - 2e-4
    dz = np.abs((d & 0xFFFFFF).astype(np.int64) - (gb["depth"] & 0xFFFFFF).astype(np.int64))
    assert np.percentile(dz, 99.9) <= 4
    upload_gbuffer(r, gb)
    base = np.full((h, w, 4), 0.25, F)
    base[..., 3] = 1.0
    r.svgf.upload(PLANE_RADIANCE, -1, base)
    r.set_debug_hits(True)
    r.ray_count(reset=True)
    r.submit_commands_gi_pathtrace()
    got, hits, rays = r.svgf.download(PLANE_RADIANCE), r.download_hits(), r.ray_count()
    want, ohits, orays = o.gi(gb, r.global_constants(), radiance=base.copy())
    same = (hits["geometry"] == ohits["geometry"]) & (hits["primitive"] == ohits["primitive"]) & ((hits["flags"] & 1) == (ohits["flags"] & 1))
    print(f"[oracle {name}] hit mismatch {1.0 - same.mean():.2e}, rays {rays} / {orays}, rel-L2 {rel_l2(got[..., :3], want[..., :3]):.2e}, "
          f"on agreeing pixels {rel_l2(got[same][:, :3], want[same][:, :3]):.2e}")
    assert 1.0 - same.mean() <= 2e-4
    assert abs(rays - orays) <= max(4, 4e-4 * orays)
    assert rel_l2(got[..., :3], want[..., :3]) <= 2e-3
    assert rel_l2(got[same][:, :3], want[same][:, :3]) <= 2e-5
    t_err = np.abs(hits["t"][same] - ohits["t"][same]) / np.maximum(np.abs(ohits["t"][same]), 1e-6)
    assert t_err.max() <= 1e-4
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 5, 6, 7: back again; with transforms; a build afterwards
# ------------------------------------------------------------------------------------------------
def test_deforming_and_deforming_back_restores_every_node_bit_for_bit():
    sc0, cam, w, h, deform = cornell_case()
    calls, _ = shaped(sc0, deform, "all")
    back = {gi: {k: sc0.geometries[gi][k] for k in KEYS} for gi in deform}
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, w, h, sun_table=0), _renderer(sn, cam, w, h, sun_table=0)
    update(ra, calls)
    moved = frame(ra, sa, cam, 2)
    update(ra, back)
    a, n = frame(ra, sa, cam, 3), frame(rn, sn, cam, 3)
    assert not np.array_equal(moved["depth"], a["depth"])
    assert_same_frames(a, n, "deformed and back", ties_allowed=False)
    assert a["stats"] == n["stats"]  # (the traversal counts do depend on the boxes)
    ra.destroy(), rn.destroy()


def test_vertex_and_transform_updates_compose_in_either_order():
    sc0, cam, w, h, deform = cornell_case()
    calls, arrays = shaped(sc0, deform, "all")
    mats = moved_matrices(sc0, [1], world_transform("translate"))
    sb = with_arrays(sc0, arrays, {1: mats[0]})
    rb = _renderer(sb, cam, w, h)
    s1, s2 = clone(sc0), clone(sc0)
    r1, r2 = _renderer(s1, cam, w, h), _renderer(s2, cam, w, h)
    update(r1, calls), r1.update_transforms([1], mats)
    r2.update_transforms([1], mats), update(r2, calls)
    for f, spp in ((2, 1), (3, 1), (4, 4)):
        b = frame(rb, sb, cam, f, spp)
        for tag, r, s in (("vertices then transform", r1, s1), ("transform then vertices", r2, s2)):
            assert_same_frames(frame(r, s, cam, f, spp), b, f"{tag} spp={spp}")
    for r in (r1, r2, rb):
        r.destroy()


@pytest.mark.parametrize("sun_table", [0, 1])
def test_a_build_after_a_deformation_starts_from_the_deformed_vertices(sun_table):
    sc0, cam, w, h, deform = atrium_case()
    calls, arrays = shaped(sc0, deform, "all")
    sa, sb = clone(sc0), with_arrays(sc0, arrays)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    update(ra, calls)
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    assert ra.scene_info() == rb.scene_info() and ra.bvh_depth() == rb.bvh_depth()
    for f, spp in ((2, 1), (3, 4)):
        a, b = frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp)
        assert_same_frames(a, b, f"rebuilt after deformation table={sun_table} spp={spp}", ties_allowed=False)  # the same tree: no mask
        for key in ("rays", "bounce_nodes", "bounce_tris") + (("shadow_nodes", "shadow_tris") if not sun_table else ()):
            assert a["stats"][key] == b["stats"][key], (key, a["stats"], b["stats"])
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 8: streams
# ------------------------------------------------------------------------------------------------
def test_vertex_updates_with_two_dispatches_in_flight_on_two_streams():
    """test_refit_gpu.test_updates_with_two_dispatches_in_flight_on_two_streams with the scene deforming: one update per frame for four
    frames, enqueued on a stream of its own while the previous frame's dispatch is in flight on a side stream; nothing but the library
    orders them, and every frame equals the serial context's."""
    sc0, cam, w, h, _ = atrium_case([])
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
        frames = []
        for f in range(2, 11):
            if f in (4, 5, 6, 7):
                gi = ATRIUM_GRIDS[f % 4]
                r.update_vertices(gi, stream=(mover if mode == "two_streams" else main).cuda_stream,
                                  **sine_along_normal(sc0, gi, amplitude=2.0 + f, phase=0.3 * f))
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
            frames.append(rad[cur].clone())  # (on the main stream, behind the frame's last pass)
            r.end_frame()
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in frames])
        r.destroy()
    assert float(np.abs(outs[0][-1][..., :3]).max()) > 0.2
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), f"frame {k + 2}"


# ------------------------------------------------------------------------------------------------
# 9: refusals
# ------------------------------------------------------------------------------------------------
def _entry(gi, positions, normals=None, tangents=None, first=0, n=None, strides=(12, 12, 16), keep=None):
    u = _lib.VertexUpdate(geometry=gi, firstVertex=first, numVertices=(positions.shape[0] if n is None else n))
    for key, a, s in (("positions", positions, strides[0]), ("normals", normals, strides[1]), ("tangents", tangents, strides[2])):
        if a is not None:
            a = np.ascontiguousarray(a, F)
            keep.append(a)
            setattr(u, key, a.ctypes.data)
        setattr(u, key[:-1] + "Stride", s)
    return u


def test_refusals_change_nothing():
    sc0, cam, w, h, deform = cornell_case()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, w, h), _renderer(sn, cam, w, h)
    lib, ctx = ra._lib, ra._ctx
    # (the tall box scaled by 1.35 along y in both contexts: a position of 3e38 is finite, its world position is not)
    scaled = moved_matrices(sc0, [2], world_transform("scale"))
    ra.update_transforms([2], scaled), rn.update_transforms([2], scaled)
    d, d2 = deform[1], twist_and_shear(sc0, 2, 10.0, 0.02)
    nv = d["positions"].shape[0]
    keep = []

    def call(*entries, n=None):
        arr = (_lib.VertexUpdate * max(1, len(entries)))(*entries)
        return lib.neb_gi_update_vertices(ctx, arr if entries else None, len(entries) if n is None else n, None)

    def E(gi, dd, **k):
        return _entry(gi, dd["positions"], dd["normals"], dd["tangents"], keep=keep, **k)

    nan, inf = d["positions"].copy(), d["positions"].copy()
    nan[5, 1] = np.nan
    inf[nv - 1, 0] = np.inf
    far = d2["positions"].copy()
    far[3] = (3.0e38, 3.0e38, 3.0e38)
    no_pos = E(1, d)
    no_pos.positions = None
    # (cornell_parts has no geometry without attributes: the valid == 0 refusal has a scene of its own below)
    cases = [("null updates", lambda: call(n=1), -1),
             ("null positions", lambda: call(E(2, d2), no_pos), -1),
             ("geometry out of range", lambda: call(E(2, d2), E(5, d)), -1),
             ("geometry far out of range", lambda: call(E(0xFFFFFFFF, d)), -1),
             ("range beyond numVertices", lambda: call(E(2, d2), E(1, d, first=1)), -1),
             ("range beyond numVertices, wrapping", lambda: call(E(1, d, first=0xFFFFFFF0)), -1),
             ("first vertex beyond, empty range", lambda: call(E(1, d, first=nv + 1, n=0)), -1),
             ("overlapping ranges", lambda: call(_entry(1, d["positions"][:10], keep=keep), E(2, d2), _entry(1, d["positions"][9:20], first=9, keep=keep)), -1),
             ("the same range twice", lambda: call(E(1, d), E(1, d)), -1),
             ("position stride too small", lambda: call(E(2, d2), E(1, d, strides=(8, 12, 16))), -1),
             ("normal stride too small", lambda: call(E(1, d, strides=(12, 11, 16))), -1),
             ("tangent stride too small", lambda: call(E(1, d, strides=(12, 12, 12))), -1),
             ("nan", lambda: call(E(2, d2), _entry(1, nan, keep=keep)), -5),
             ("inf", lambda: call(_entry(1, inf, d["normals"], keep=keep)), -5),
             ("world position not finite", lambda: call(_entry(2, far, keep=keep)), -5),
             ("n == 0", lambda: call(), 0),
             ("n == 0 with a pointer", lambda: call(E(1, d), n=0), 0),
             ("every range empty", lambda: call(E(1, d, n=0), E(2, d2, first=3, n=0)), 0)]
    f = 2
    for what, fn, want in cases:
        assert fn() == want, what
        if want != 0:
            assert b"neb_gi_update_vertices" in lib.neb_last_error(ctx), what
        a, n = frame(ra, sa, cam, f), frame(rn, sn, cam, f)
        assert_same_frames(a, n, f"after refusal: {what}", ties_allowed=False)
        assert a["stats"] == n["stats"], what
        assert ra.sun_table_stats() == rn.sun_table_stats(), what
        f += 1
    with pytest.raises(NebError):
        ra.update_vertices(1, d["positions"], first_vertex=1)
    with pytest.raises(NebError):
        ra.update_vertices(1, d["positions"], normals=d["normals"][:-1])
    assert all(np.array_equal(g[k], q[k]) for g, q in zip(sa.geometries, sc0.geometries) for k in KEYS)  # (the Python scene follows accepted updates only)
    # adjacent ranges are no overlap: accepted, and the same as one range
    assert call(_entry(1, d["positions"][:10], keep=keep), _entry(1, d["positions"][10:], first=10, keep=keep)) == 0
    rn.update_vertices(1, d["positions"])
    assert_same_frames(frame(ra, sa, cam, f), frame(rn, sn, cam, f), "two adjacent ranges against one", ties_allowed=False)
    ra.destroy(), rn.destroy()
    # normals / tangents for a geometry that was set without an attribute stream (DevGeom::valid == 0); positions alone are accepted
    sv = S.Scene("no-tangents")
    sv.add_material(albedo=(0.5, 0.5, 0.5, 1))
    g1 = sc0.geometries[1]
    sv.add_geometry(g1["positions"], g1["normals"], g1["uvs"], g1["indices"], material=0, M=g1["M"], omit=("tangents",))
    r = _renderer(sv, cam, 64, 48)
    lib, ctx = r._lib, r._ctx
    assert call(_entry(0, d["positions"], d["normals"], keep=keep)) == -1 and b"neb_gi_update_vertices" in lib.neb_last_error(ctx)
    assert call(_entry(0, d["positions"], None, d["tangents"], keep=keep)) == -1
    assert call(_entry(0, d["positions"], keep=keep)) == 0
    r.destroy()
    # before a successful build: no scene at all, and a scene that has not been built
    r = DeferredRenderer()
    r.init(64, 48)
    u = _entry(1, d["positions"], keep=keep)
    assert r._lib.neb_gi_update_vertices(r._ctx, C.byref(u), 1, None) == -4
    G, ng, M, nm, T, nt = sc0.descs()
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_update_vertices(r._ctx, C.byref(u), 1, None) == -4
    assert b"neb_gi_update_vertices" in r._lib.neb_last_error(r._ctx)
    assert r._lib.neb_gi_build_bvh(r._ctx, None) == 0
    assert r._lib.neb_gi_update_vertices(r._ctx, C.byref(u), 1, None) == 0
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 10, 11: memory, cost
# ------------------------------------------------------------------------------------------------
def _update_many(sc0, indices, amplitude, phase, keep):
    """the entries of ONE call for many submeshes, positions + normals (the renderer's method takes one submesh per call)"""
    entries = []
    for gi in indices:
        d = sine_along_normal(sc0, gi, amplitude=amplitude, phase=phase)
        entries.append(_entry(gi, d["positions"], d["normals"], keep=keep))
    return (_lib.VertexUpdate * len(entries))(*entries)


def test_a_hundred_vertex_updates_hold_no_more_device_memory():
    sc0, cam, w, h, _ = atrium_case([])
    sc = clone(sc0)
    r = _renderer(sc, cam, w, h, exact=False, hits=False)
    poses = []
    for k in range(4):
        keep = []
        poses.append((_update_many(sc0, ATRIUM_COLUMNS[::3], 3.0 + k, 0.7 * k, keep), keep))
    free = {}
    for k in range(104):
        arr = poses[k % 4][0]
        r._check(r._lib.neb_gi_update_vertices(r._ctx, arr, len(arr), None), "neb_gi_update_vertices")
        if k % 4 == 0 or 40 <= k < 50:  # (rests of a few frames: tables are built and dropped along the way)
            out = frame(r, sc, cam, 2 + k)
            assert np.isfinite(out["radiance"]).all()
        if k in (3, 103):
            free[k] = _free_bytes()
    print(f"[deform soak] free device memory after update 4 / 104: {free[3] >> 20} / {free[103] >> 20} MB; sun table {r.sun_table_stats()}")
    assert free[3] - free[103] < 4 << 20, free  # test_refit_gpu's bar: steady state allocates nothing
    r.destroy()


def test_a_deformation_costs_less_device_time_than_a_build():
    """the project's condition for a refit: cheaper on the device than neb_gi_build_bvh was on the same scene in the
    same process.  Every column of atrium_small in one call, positions + normals: 43 submeshes, 44 075 vertices, 82 560 triangles
    (atrium_small has no drapes; the bench scene's six drapes are timed by tools/deform_times.py)."""
    sc0, cam, w, h, _ = atrium_case([])
    r = _renderer(clone(sc0), cam, w, h, exact=False, hits=False)
    build_ms = r.build_ms()
    poses = []
    for k in range(2):
        keep = []
        poses.append((_update_many(sc0, ATRIUM_COLUMNS, 4.0 + k, 0.5 * k, keep), keep))
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for k in range(22):
        arr = poses[k % 2][0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r._check(r._lib.neb_gi_update_vertices(r._ctx, arr, len(arr), C.c_void_p(st)), "neb_gi_update_vertices")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times[2:]))
    print(f"[deform cost] update of {len(ATRIUM_COLUMNS)} submeshes, positions + normals: {med * 1e3:.0f} us on the device; neb_gi_build_ms {build_ms:.2f} ms")
    assert med < build_ms, (med, build_ms)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 12: strips
# ------------------------------------------------------------------------------------------------
def test_two_strip_contexts_given_the_same_deformation_equal_the_full_frame():
    sc0, cam, w, h, deform = cornell_case()
    calls, _ = shaped(sc0, deform, "all")
    cut = 88  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = clone(sc0), clone(sc0), clone(sc0)
    full = _renderer(sf, cam)
    up = _renderer(s_up, cam, row_begin=0, row_end=cut)
    dn = _renderer(s_dn, cam, row_begin=cut, row_end=H)
    for r in (full, up, dn):
        update(r, calls)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], x.shape[1], -1)
    for f, spp in ((2, 1), (3, 4)):
        a, u, d = frame(full, sf, cam, f, spp), frame(up, s_up, cam, f, spp), frame(dn, s_dn, cam, f, spp)
        for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
            assert np.array_equal(bits(a[name]), bits(np.concatenate([u[name], d[name]], axis=0))), (name, f)
        assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
        assert a["rays"] == u["rays"] + d["rays"]
    for r in (full, up, dn):
        r.destroy()
