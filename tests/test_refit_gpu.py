"""neb_gi_update_transforms: submeshes moved by transform, the BVH refitted in place.

The traverser's results cannot depend on the boxes -- only the exact triangle tests decide a hit -- so a refitted tree renders what a
tree built from the moved scene renders, bit for bit, up to exact ties between coincident hits (two triangles at the same t: which one
is reported depends on the order the tree is walked in).  Ties are capped at TIE_CAP pixels per frame, the upper end of what the
project measures against its oracle at 1080p (test_gi_gpu.py: 7 of 2 073 600); these frames are 40 times smaller."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nebulae_amd import scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import NebError, PLANE_ALBEDO, PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE, PLANE_WORLDPOS
from oracle_lib import OracleTracer
from svgf_cases import rel_l2
from test_gi_gpu import scenes, upload_gbuffer

pytestmark = pytest.mark.gpu

TIE_CAP = 8
W, H = 256, 192
F = np.float32


# ------------------------------------------------------------------------------------------------
# scenes and transforms
# ------------------------------------------------------------------------------------------------
def cornell_parts(textured=True):
    """the Cornell stand-in of scene.cornell_standin with its two boxes as submeshes of their own: 0 shell, 1 short box, 2 tall box,
    3 red wall, 4 green wall"""
    sc = S.Scene("cornell-parts")
    s = math.sqrt(0.5)
    M = S._node_matrix({"rotation": [s, 0, 0, s]})
    if textured:
        ta, tn, tr = sc.add_texture(S._proc_texture("albedo", 11)), sc.add_texture(S._proc_texture("normal", 12)), \
            sc.add_texture(S._proc_texture("rm", 13))
        white = sc.add_material(textures=(ta, tn, tr))
    else:
        white = sc.add_material(albedo=(0.725, 0.71, 0.68, 1), rm=(1.0, 0.0))
    red = sc.add_material(albedo=(0.63, 0.065, 0.05, 1), rm=(1.0, 0.0))
    green = sc.add_material(albedo=(0.14, 0.45, 0.091, 1), rm=(1.0, 0.0))
    box_mat = sc.add_material(albedo=(0.5, 0.55, 0.7, 1), rm=(0.6, 0.0))
    Minv = np.linalg.inv(M.astype(np.float64)).astype(F)

    def to_local(part):
        P, N, UV, I = part
        return (P @ Minv[:3, :3] + Minv[3, :3]).astype(F), (N @ Minv[:3, :3]).astype(F), UV, I

    shell = [S._quad((-1, -1, -2), (1, -1, -2), (1, 1, -2), (-1, 1, -2)), S._quad((-1, -1, 0), (1, -1, 0), (1, -1, -2), (-1, -1, -2)),
             S._quad((-1, 1, -2), (1, 1, -2), (1, 1, 0), (-1, 1, 0))]
    sc.add_geometry(*to_local(S._merge(shell)), material=white, M=M)
    sc.add_geometry(*to_local(S._box((-0.7, -1.0, -1.3), (-0.1, -0.4, -0.7))), material=box_mat, M=M)
    sc.add_geometry(*to_local(S._box((0.1, -1.0, -1.9), (0.7, 0.2, -1.3))), material=white, M=M)
    sc.add_geometry(*to_local(S._quad((-1, -1, 0), (-1, -1, -2), (-1, 1, -2), (-1, 1, 0))), material=red, M=M)
    sc.add_geometry(*to_local(S._quad((1, -1, -2), (1, -1, 0), (1, 1, 0), (1, 1, -2))), material=green, M=M)
    return sc


def cornell_camera():
    # off every axis and off the room's diagonals: no ray runs along an edge two triangles share
    return S.orbit_camera(origin=(0.03, -0.07, -0.9), yaw_deg=13.7, pitch_deg=78.3, distance=3.4)


def world_transform(kind, k=0):
    """4x4 world-space motions (row-vector convention: world' = world * T)"""
    T = np.eye(4)
    if kind == "translate":
        T[3, :3] = (0.137 + 0.01 * k, 0.211, 0.093)
    elif kind == "rotate":
        a = math.radians(23.0 + 7.0 * k)
        c, s = math.cos(a), math.sin(a)
        R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])  # about y through the point p
        p = np.array([-0.4, -0.7, -1.0])
        T[:3, :3] = R
        T[3, :3] = p - p @ R
    elif kind == "scale":
        T[:3, :3] = np.diag([0.8, 1.35, 1.15])
        p = np.array([0.4, -1.0, -1.6])  # the scale keeps the floor contact of the tall box: y = -1 stays
        T[3, :3] = p - p @ T[:3, :3] + np.array([-0.05, 0.0, 0.11])
    else:
        raise ValueError(kind)
    return T


def moved_matrices(sc, indices, T):
    return np.stack([np.ascontiguousarray((sc.geometries[i]["M"].astype(np.float64) @ T).astype(F)) for i in indices])


def with_matrices(sc, indices, mats):
    """a copy of the scene (vertex streams shared) with the named geometries' matrices replaced"""
    out = S.Scene(sc.name + "-moved")
    out.materials, out.textures = sc.materials, sc.textures
    out.geometries = [dict(g) for g in sc.geometries]
    for i, m in zip(indices, mats):
        out.geometries[i]["M"] = np.ascontiguousarray(m, F)
    return out


def clone(sc):
    return with_matrices(sc, [], [])


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
def make_renderer(sc, cam, w=W, h=H, sun_table=1, exact=True, hits=True, **init):
    r = DeferredRenderer()
    r.init(w, h, atrous_levels=4, **init)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))  # uploads the scene and builds the tree
    if exact:
        r.svgf.set_option("gi_exact_shade", 1)
    if hits:
        r.set_debug_hits(True)
    r.svgf.set_option("gi_sun_table", sun_table)
    r.svgf.set_option("gi_sun_hold", 2)
    return r


def frame(r, sc, cam, f, spp=1, mpv=2, gbuffer=True):
    r.gi_ui.gi_samples_per_pixel, r.gi_ui.max_path_vertices = spp, mpv
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
    out = {}
    if gbuffer:
        r.submit_commands_gbuffer()
    rows = r.svgf.row_end - r.svgf.row_begin
    r.svgf.upload(PLANE_RADIANCE, -1, np.zeros((rows, r.width, 4), F))
    r.ray_count(reset=True)
    r.submit_commands_gi_pathtrace()
    out["radiance"] = r.svgf.download(PLANE_RADIANCE)
    for name, pl in (("depth", PLANE_DEPTH), ("normal", PLANE_NORMAL), ("world_pos", PLANE_WORLDPOS), ("albedo", PLANE_ALBEDO)):
        out[name] = r.svgf.download(pl, 0 if pl in (PLANE_WORLDPOS, PLANE_ALBEDO) else -1)
    if r._hits_on:
        out["hits"] = r.download_hits()
    out["rays"] = r.ray_count()
    out["stats"] = r.traversal_stats()
    r.end_frame()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)


def assert_same_frames(a, b, what, ties_allowed=True, hits_visible=True):
    """bit for bit, except (ties_allowed) exact ties: the GI pass -- both report the same t bits for different (geometry, primitive);
    the G-buffer -- identical depth bits, another plane different.  At most TIE_CAP of each per frame."""
    gb_diff = np.zeros(a["depth"].shape, bool)
    for name in ("normal", "world_pos", "albedo"):
        gb_diff |= (_bits(a[name]) != _bits(b[name])).any(-1)
    depth_diff = a["depth"] != b["depth"]
    print(f"[{what}] g-buffer: depth differs at {int(depth_diff.sum())} px, another plane at {int(gb_diff.sum())} px")
    assert not depth_diff.any(), f"{what}: depth differs at {int(depth_diff.sum())} pixels"
    assert int(gb_diff.sum()) <= (TIE_CAP if ties_allowed else 0), f"{what}: g-buffer ties {int(gb_diff.sum())}"
    rad_diff = (_bits(a["radiance"]) != _bits(b["radiance"])).any(-1)
    if "hits" in a and hits_visible:
        ha, hb = a["hits"], b["hits"]
        same_t = ha["t"].view(np.uint32) == hb["t"].view(np.uint32)
        same_id = (ha["geometry"] == hb["geometry"]) & (ha["primitive"] == hb["primitive"])
        same_flag = (ha["flags"] & 1) == (hb["flags"] & 1)
        tie = same_t & ~same_id
        bad = (~same_t | (same_id & ~same_flag) | rad_diff) & ~tie & ~gb_diff
        print(f"[{what}] GI: ties {int(tie.sum())}, other differing px {int(bad.sum())}, radiance differs at {int(rad_diff.sum())} px, "
              f"rays {a['rays']} / {b['rays']}")
        assert int(tie.sum()) <= (TIE_CAP if ties_allowed else 0), f"{what}: {int(tie.sum())} ties"
        assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ that are no ties"
        if not tie.any() and not gb_diff.any():
            assert a["rays"] == b["rays"], (what, a["rays"], b["rays"])
        else:  # (a tied pixel's path may end differently: at most one bounce and one shadow ray per path vertex and sample)
            assert abs(a["rays"] - b["rays"]) <= 2 * 4 * int(tie.sum() + gb_diff.sum()), (what, a["rays"], b["rays"])
    else:
        print(f"[{what}] GI (intermediate hits not visible): radiance differs at {int(rad_diff.sum())} px, rays {a['rays']} / {b['rays']}")
        assert int(rad_diff.sum()) <= (TIE_CAP if ties_allowed else 0), f"{what}: {int(rad_diff.sum())} pixels differ"


def _renderer(*a, **k):
    r = make_renderer(*a, **k)
    r._hits_on = k.get("hits", True)
    return r


def update(r, indices, mats, stream=None):
    r.update_transforms(indices, mats, stream=stream)


# ------------------------------------------------------------------------------------------------
# refit == rebuild
# ------------------------------------------------------------------------------------------------
def _refit_against_rebuild(sc0, cam, indices, T, sun_table, w, h, tag):
    mats = moved_matrices(sc0, indices, T)
    sa, sb = clone(sc0), with_matrices(sc0, indices, mats)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    depth, info = ra.bvh_depth(), ra.scene_info()
    frame(ra, sa, cam, 2)  # (a dispatch before the update: with the table on, it exists and is then invalidated)
    update(ra, indices, mats)
    assert ra.bvh_depth() == depth and ra.scene_info() == info  # the tree is kept: same nodes, same depth (the rebuilt one may differ)
    if sun_table:  # both contexts get to a table of the moved scene: the hold is two dispatches
        for f in (3, 4):
            frame(ra, sa, cam, f), frame(rb, sb, cam, f)
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 1
    for f, spp, mpv in ((5, 1, 2), (6, 4, 2), (7, 1, 4)):
        a, b = frame(ra, sa, cam, f, spp, mpv), frame(rb, sb, cam, f, spp, mpv)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_same_frames(a, b, f"{tag} table={sun_table} spp={spp} mpv={mpv}", hits_visible=(mpv == 2))
    ra.destroy(), rb.destroy()


@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("kind,indices", [("translate", [1]), ("rotate", [1, 2]), ("scale", [2])])
def test_refit_equals_rebuild_on_the_cornell_boxes(kind, indices, sun_table):
    _refit_against_rebuild(cornell_parts(), cornell_camera(), indices, world_transform(kind), sun_table, W, H, f"cornell {kind}")


@pytest.mark.parametrize("sun_table", [0, 1])
def test_refit_equals_rebuild_on_a_mid_sized_scene(sun_table):
    make, cam, w, h = scenes()["atrium_small"]
    T = np.eye(4)
    T[3, :3] = (0.31, 0.07, -0.23)
    _refit_against_rebuild(make(), cam, [3, 11, 12, 27, 41, 58], T, sun_table, w, h, "atrium_small translate")


def test_an_update_with_unchanged_matrices_changes_nothing():
    sc0, cam = cornell_parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam), _renderer(sn, cam)
    for f in (2, 3):
        frame(ra, sa, cam, f), frame(rn, sn, cam, f)
    update(ra, [0, 1, 2, 3, 4], np.stack([g["M"] for g in sa.geometries]))
    for f, spp in ((4, 1), (5, 4)):
        a, n = frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp)
        assert_same_frames(a, n, f"identity spp={spp}", ties_allowed=False)
        assert a["stats"] == n["stats"] and a["stats"]["bounce_nodes"] > 0
    assert ra.sun_table_stats() == rn.sun_table_stats()
    ra.destroy(), rn.destroy()


def test_moving_away_and_back_restores_every_node_bit_for_bit():
    """(the kernels' side of the identity: a move and its inverse are two real refits; the frames AND the traversal counts -- which
    do depend on the boxes -- return to those of a context that never moved)"""
    sc0, cam = cornell_parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam, sun_table=0), _renderer(sn, cam, sun_table=0)
    orig = np.stack([sa.geometries[i]["M"] for i in (1, 2)])
    update(ra, [1, 2], moved_matrices(sa, [1, 2], world_transform("rotate")))
    moved = frame(ra, sa, cam, 2)
    update(ra, [1, 2], orig)
    a, n = frame(ra, sa, cam, 3), frame(rn, sn, cam, 3)
    assert not np.array_equal(moved["depth"], a["depth"])
    assert_same_frames(a, n, "away and back", ties_allowed=False)
    assert a["stats"] == n["stats"]
    ra.destroy(), rn.destroy()


def test_a_chain_of_eight_updates_does_not_drift():
    sc0, cam = cornell_parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam), _renderer(sn, cam)
    orig = np.stack([sc0.geometries[i]["M"] for i in (1, 2)])
    mats = None
    for k in range(8):  # every transform is applied to the original object-space positions
        T = world_transform("rotate", k) @ world_transform("translate", k)
        mats = moved_matrices(sc0, [1, 2], T)
        update(ra, [1, 2], mats)
        a = frame(ra, sa, cam, 2 + k)
    sb = with_matrices(sc0, [1, 2], mats)
    rb = _renderer(sb, cam)
    for f in (2, 3, 4, 5, 6, 7, 8):
        frame(rb, sb, cam, f)  # (the same frame count: the contexts' plane slots alternate alike)
    b = frame(rb, sb, cam, 9)
    assert_same_frames(a, b, "chain: frame 8 against a fresh build")
    update(ra, [1, 2], orig)
    for f in range(2, 10):
        frame(rn, sn, cam, f)
    a, n = frame(ra, sa, cam, 10), frame(rn, sn, cam, 10)
    assert_same_frames(a, n, "chain: restored against never moved")
    ra.destroy(), rb.destroy(), rn.destroy()


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_parts", "atrium_small"])
def test_an_updated_context_matches_the_oracle_on_the_moved_scene(name):
    """test_gi_gpu.test_gi_matches_oracle, at its bars, for a context that reached the scene through an update: the result is pinned
    to the checker, not only to this back end's own rebuild"""
    if name == "cornell_parts":
        sc0, cam, w, h, indices, T = cornell_parts(), cornell_camera(), W, H, [1, 2], world_transform("rotate")
    else:
        make, cam, w, h = scenes()["atrium_small"]
        sc0, indices, T = make(), [3, 11, 12, 27, 41, 58], np.eye(4)
        T[3, :3] = (0.31, 0.07, -0.23)
    mats = moved_matrices(sc0, indices, T)
    sa = clone(sc0)
    r = DeferredRenderer()
    r.init(w, h, atrous_levels=4)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=4))
    r.update_transforms(indices, mats)
    sm = with_matrices(sc0, indices, mats)
    o = OracleTracer(sm)
    assert all(np.array_equal(g["M"], q["M"]) for g, q in zip(sa.geometries, sm.geometries))  # the renderer's scene followed the update
    gb = o.gbuffer(w, h, cam)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=5))
    # the G-buffer of the updated context against the oracle's (test_gbuffer_raycast_matches_oracle's bars)
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
# the sun table
# ------------------------------------------------------------------------------------------------
def test_the_sun_table_is_dropped_by_an_update_and_comes_back_after_the_hold():
    sc0, cam = cornell_parts(), cornell_camera()
    s1, s0 = clone(sc0), clone(sc0)
    r1, r0 = _renderer(s1, cam, sun_table=1), _renderer(s0, cam, sun_table=0)
    for f in (2, 3):
        a, b = frame(r1, s1, cam, f), frame(r0, s0, cam, f)
    st = r1.sun_table_stats()
    assert st["builds"] == 1 and st["lit_plus"] + st["lit_minus"] > 0
    mats = moved_matrices(sc0, [1], world_transform("translate"))
    update(r1, [1], mats), update(r0, [1], mats)
    st = r1.sun_table_stats()
    assert st["lit_plus"] == 0 and st["lit_minus"] == 0 and st["builds"] == 1, st  # no valid table from the moment of the call
    a, b = frame(r1, s1, cam, 4), frame(r0, s0, cam, 4)  # first dispatch after the update: the new scene seen once, every ray traced
    assert r1.sun_table_stats()["builds"] == 1
    assert_same_frames(a, b, "right after the update: table on / off", ties_allowed=False)
    assert a["stats"] == b["stats"]
    a, b = frame(r1, s1, cam, 5), frame(r0, s0, cam, 5)  # second: the hold is over, a table of the moved scene
    st = r1.sun_table_stats()
    assert st["builds"] == 2 and st["lit_plus"] + st["lit_minus"] > 0, st
    assert_same_frames(a, b, "after the hold: table on / off", ties_allowed=False)
    r1.ray_count()
    assert r1.sun_table_stats()["rays_answered"] > 0
    # a move that takes the scene box past +-218 units: no certificate there, no table
    far = np.eye(4)
    far[3, :3] = (300.0, 0.0, 0.0)
    mats = moved_matrices(sc0, [2], far)
    update(r1, [2], mats), update(r0, [2], mats)
    for f in (6, 7, 8):
        a, b = frame(r1, s1, cam, f), frame(r0, s0, cam, f)
        assert_same_frames(a, b, f"far box, frame {f}: table on / off", ties_allowed=False)
    st = r1.sun_table_stats()
    assert st["builds"] == 2 and st["lit_plus"] == 0 and st["lit_minus"] == 0, st
    r1.destroy(), r0.destroy()


# ------------------------------------------------------------------------------------------------
# streams
# ------------------------------------------------------------------------------------------------
def test_updates_with_two_dispatches_in_flight_on_two_streams():
    """test_sun_table_gpu.test_a_new_sun_with_two_dispatches_in_flight_on_two_streams with the scene moving: the update is enqueued on a
    stream of its own while the previous frame's dispatch is in flight on a side stream ("gi_defer_resolve" = 2), and the next dispatch
    goes to the other side stream.  Nothing but the library orders the three; the denoised sequence equals the serial one."""
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    moving = [3, 11, 12, 27, 41, 58]
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
                T = np.eye(4)
                T[3, :3] = (0.05 * f, 0.01 * f, -0.03 * f)
                r.update_transforms(moving, moved_matrices(sc0, moving, T), stream=(mover if mode == "two_streams" else main).cuda_stream)
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
        outs.append(r.svgf.download(PLANE_RADIANCE))
        r.destroy()
    assert float(np.abs(outs[0][..., :3]).max()) > 0.2
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------
# rebuild after an update; strips
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
def test_a_build_after_an_update_starts_from_the_updated_transforms(sun_table):
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    indices, T = [3, 11, 12, 27, 41, 58], np.eye(4)
    T[:3, :3] = np.diag([1.1, 0.9, 1.2])
    T[3, :3] = (0.31, 0.07, -0.23)
    mats = moved_matrices(sc0, indices, T)
    sa, sb = clone(sc0), with_matrices(sc0, indices, mats)
    ra, rb = _renderer(sa, cam, w, h, sun_table=sun_table), _renderer(sb, cam, w, h, sun_table=sun_table)
    update(ra, indices, mats)
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    assert ra.scene_info() == rb.scene_info() and ra.bvh_depth() == rb.bvh_depth()
    for f, spp in ((2, 1), (3, 4)):
        a, b = frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp)
        assert_same_frames(a, b, f"rebuilt after update table={sun_table} spp={spp}", ties_allowed=False)  # the same tree: no mask
        print(f"[rebuilt after update table={sun_table} spp={spp}] traversal {a['stats']} / {b['stats']}")
        # the walk of the same tree: the closest-hit counts always; the any-hit counts with the table off (with it on, which hint answers a
        # shadow ray first is not part of what the table promises)
        for key in ("rays", "bounce_nodes", "bounce_tris") + (("shadow_nodes", "shadow_tris") if not sun_table else ()):
            assert a["stats"][key] == b["stats"][key], (key, a["stats"], b["stats"])
    ra.destroy(), rb.destroy()


def test_two_strip_contexts_given_the_same_update_equal_the_full_frame():
    sc0, cam = cornell_parts(), cornell_camera()
    mats = moved_matrices(sc0, [1, 2], world_transform("rotate"))
    cut = 88  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = clone(sc0), clone(sc0), clone(sc0)
    full = _renderer(sf, cam)
    up = _renderer(s_up, cam, row_begin=0, row_end=cut)
    dn = _renderer(s_dn, cam, row_begin=cut, row_end=H)
    for r in (full, up, dn):
        update(r, [1, 2], mats)
    for f, spp in ((2, 1), (3, 4)):
        a, u, d = frame(full, sf, cam, f, spp), frame(up, s_up, cam, f, spp), frame(dn, s_dn, cam, f, spp)
        for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
            assert np.array_equal(_bits(a[name]), _bits(np.concatenate([u[name], d[name]], axis=0))), (name, f)
        assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
        assert a["rays"] == u["rays"] + d["rays"]
    for r in (full, up, dn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# refusals; soak
# ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    sc0, cam = cornell_parts(), cornell_camera()
    sa, sn = clone(sc0), clone(sc0)
    ra, rn = _renderer(sa, cam), _renderer(sn, cam)
    lib, ctx = ra._lib, ra._ctx
    eye = np.stack([g["M"] for g in sa.geometries])
    moved = moved_matrices(sc0, [0, 1, 2, 3, 4], world_transform("translate"))

    def call(idx, m, n=None):
        idx = np.asarray(idx, np.uint32)
        m = np.ascontiguousarray(m, F)
        return lib.neb_gi_update_transforms(ctx, idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx.size else None,
                                            m.ctypes.data_as(C.POINTER(C.c_float)) if m.size else None, len(idx) if n is None else n, None)

    nan, inf, big = moved[1].copy(), moved[1].copy(), moved[2].copy()
    nan[1, 2] = np.nan
    inf[3, 0] = np.inf
    big[:3, :3] *= F(3.0e38)  # finite entries, but the tall box reaches 1.9 units from its origin: its corners go to infinity
    cases = [("null indices", lambda: lib.neb_gi_update_transforms(ctx, None, moved.ctypes.data_as(C.POINTER(C.c_float)), 1, None), -1),
             ("null matrices", lambda: lib.neb_gi_update_transforms(ctx, np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), None, 1, None), -1),
             ("index out of range", lambda: call([1, 5], moved[:2]), -1),
             ("index far out of range", lambda: call([0xFFFFFFFF], moved[:1]), -1),
             ("index twice", lambda: call([1, 2, 1], moved[:3]), -1),
             ("more entries than geometries", lambda: call([0, 1, 2, 3, 4, 0], np.concatenate([moved, moved[:1]])), -1),
             ("nan", lambda: call([2, 1], np.stack([moved[2], nan])), -5),
             ("inf", lambda: call([1], inf[None]), -5),
             ("box to infinity", lambda: call([2], big[None]), -5),
             ("n == 0", lambda: call([], np.zeros((0, 4, 4), F)), 0),
             ("n == 0 with pointers", lambda: call([1], moved[1:2], n=0), 0)]
    f = 2
    for what, fn, want in cases:
        assert fn() == want, what
        if want != 0:
            assert b"neb_gi_update_transforms" in lib.neb_last_error(ctx), what
        a, n = frame(ra, sa, cam, f), frame(rn, sn, cam, f)
        assert_same_frames(a, n, f"after refusal: {what}", ties_allowed=False)
        assert a["stats"] == n["stats"], what
        assert ra.sun_table_stats() == rn.sun_table_stats(), what
        f += 1
    with pytest.raises(NebError):
        ra.update_transforms([1, 1], moved[:2])
    assert all(np.array_equal(g["M"], m) for g, m in zip(sa.geometries, eye))  # (the Python scene follows accepted updates only)
    ra.destroy(), rn.destroy()
    # before a successful build: no scene at all, and a scene that has not been built
    r = DeferredRenderer()
    r.init(64, 48)
    idx, m = np.zeros(1, np.uint32), np.eye(4, dtype=F)
    args = (idx.ctypes.data_as(C.POINTER(C.c_uint32)), m.ctypes.data_as(C.POINTER(C.c_float)), 1, None)
    assert r._lib.neb_gi_update_transforms(r._ctx, *args) == -4
    G, ng, M, nm, T, nt = sc0.descs()
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_update_transforms(r._ctx, *args) == -4
    assert r._lib.neb_gi_build_bvh(r._ctx, None) == 0
    assert r._lib.neb_gi_update_transforms(r._ctx, *args) == 0
    r.destroy()


def _free_bytes():  # (tests/test_soak_gpu.py's query)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_a_hundred_updates_hold_no_more_device_memory():
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    sc = clone(sc0)
    r = _renderer(sc, cam, w, h, exact=False, hits=False)
    moving = list(range(0, len(sc0.geometries), 3))
    free = {}
    for k in range(104):
        T = np.eye(4)
        T[3, :3] = (0.2 * math.sin(0.3 * k), 0.02 * (k % 5), 0.2 * math.cos(0.3 * k))
        update(r, moving if k % 10 else list(range(len(sc0.geometries))), moved_matrices(sc0, moving if k % 10 else list(range(len(sc0.geometries))), T))
        if k % 4 == 0 or 40 <= k < 50:  # (rests of a few frames: tables are built and dropped along the way)
            out = frame(r, sc, cam, 2 + k)
            assert np.isfinite(out["radiance"]).all()
        if k in (3, 103):
            free[k] = _free_bytes()
    print(f"[refit soak] free device memory after update 4 / 104: {free[3] >> 20} / {free[103] >> 20} MB; sun table {r.sun_table_stats()}")
    assert free[3] - free[103] < 4 << 20, free  # test_soak_gpu.py's bar: steady state allocates nothing (the sun table's one list aside)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# cost
# ------------------------------------------------------------------------------------------------
def test_an_update_costs_less_device_time_than_a_build():
    """the condition of DESIGN.md 3.4a: moving every submesh of a scene takes less device time than neb_gi_build_bvh took on the same
    scene in the same process (tools/refit_times.py records the real ratio on the bench scene)"""
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    sc = clone(sc0)
    r = _renderer(sc, cam, w, h, exact=False, hits=False)
    build_ms = r.build_ms()
    everything = list(range(len(sc0.geometries)))
    times = []
    for k in range(12):
        T = np.eye(4)
        T[3, :3] = (0.01 * (k + 1), 0.0, 0.0)
        mats = moved_matrices(sc0, everything, T)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        update(r, everything, mats, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times[2:]))
    print(f"[refit cost] update of all {len(everything)} submeshes: {med * 1e3:.0f} us on the device; neb_gi_build_ms {build_ms:.2f} ms")
    assert med < build_ms, (med, build_ms)
    r.destroy()
