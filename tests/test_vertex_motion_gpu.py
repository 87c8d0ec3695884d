"""GPU tests of option svgf_vertex_motion: option and plane state, the static scene, the previous-point plane against
the float64 reference (tests/vertex_motion_ref.py) for every way a deformation can arrive, the third arm of the temporal kernel
against the CPU reference on the device's own planes, the roll, streams, the painted object, what a user sees, memory.

The scenes, cameras and deformations are tests/vertex_motion_cases.py's; tests/test_vertex_motion_cpu.py shows on reference-made
G-buffers that they leave fewer than 0.1 % of the pixels near a threshold and keep history on at least 90 % of the deformed submesh."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as M
import reproject_ref as R
import vertex_motion_ref as VM
import views_ref as V
from motion_cases import small_transform
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import (PLANE_DEPTH, PLANE_HISTORY_LENGTH, PLANE_MOMENTS, PLANE_NORMAL, PLANE_PREV_POINT, PLANE_RADIANCE,
                              PLANE_SUBMESH_ID, PLANE_VARIANCE, SLOT_CURRENT, SLOT_HISTORY, NebError, SVGFDenoiser)
from svgf_cases import half_ulp_mismatch, rel_l2
from test_deform_device_gpu import update_device
from test_deform_gpu import shaped, twist_and_shear, update, with_arrays
from test_refit_gpu import TIE_CAP, _free_bytes, clone, cornell_camera, cornell_parts, moved_matrices
from test_reproject_gpu import seeded_history
from vertex_motion_cases import CAMERA_MOVE, CASE_IDS, CASES, SCENES, SHORT_BOX, cameras, cornell_case, matrices, room_camera, room_case, twisted

pytestmark = pytest.mark.gpu
NEB_ERR_INVALID_ARG, NEB_ERR_STATE = -1, -4
F = np.float32
NEAR_CAP = 1e-3    # of the compared pixels (test_vertex_motion_cpu.py)
KEPT_FLOOR = 0.9
# |P_h(device) - P_h(float64)| over the linear depth of the pixel's point.  Measured on an MI355X over the seven cases of
# test_plane_against_float64 as first written: 3.18e-7 at worst (the two cases that also move the box; 2.95e-7 in the other five -- fp32 barycentrics
# of the device's hit against float64 ones), times 4.  A tenth of kReprojPlaneTol = 1e-3 is the most the plane test could bear: beyond
# that it is a bug, not a tolerance.
P_BAR = 1.27e-6
assert P_BAR < 0.1 * float(R.PLANE_TOL)


def vm_renderer(w, h, vertex=True):
    r = DeferredRenderer()
    r.temporal_reprojection = True
    r.motion_vectors = True
    r.vertex_motion = vertex
    r.init(w, h)
    return r


def is_sentinel(plane):
    return np.ascontiguousarray(plane[..., 3]).view(np.uint32) == VM.NO_PREV_POINT


def all_sentinel(plane):
    return bool(is_sentinel(plane).all()) and not plane[..., :3].any()


def raycast(r, sc, cam, f):
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
    r.submit_commands_gbuffer()
    return tuple(r.svgf.download(p) for p in (PLANE_DEPTH, PLANE_NORMAL, PLANE_SUBMESH_ID))


def two_frames(sc0, apply, cam_prev, cam_cur, w, h, vertex=True):
    """frame 1 at cam_prev, apply(renderer) -- the updates between the frames --, frame 2 at cam_cur, through neb_gbuffer_raycast.
    -> (renderer at frame 2, [(depth, normal, id)] of the two frames, the previous-point plane of frame 2 (None with the option off),
        (m_hist, m_cur), the scene as the updates left it)"""
    sc = clone(sc0)
    r = vm_renderer(w, h, vertex)
    planes = [raycast(r, sc, cam_prev, 1)]
    m_hist = matrices(sc)
    apply(r)
    planes.append(raycast(r, sc, cam_cur, 2))
    return r, planes, (r.svgf.download(PLANE_PREV_POINT) if vertex else None), (m_hist, matrices(sc)), sc


def seed_planes(d, rad_prev, rad_cur, mom, hlen):
    d.upload(PLANE_RADIANCE, SLOT_CURRENT, rad_cur)
    d.upload(PLANE_RADIANCE, SLOT_HISTORY, rad_prev)
    d.upload(PLANE_MOMENTS, SLOT_HISTORY, mom)
    d.upload(PLANE_HISTORY_LENGTH, SLOT_HISTORY, hlen)


def outputs(d):
    return dict(radiance=d.download(PLANE_RADIANCE), moments=d.download(PLANE_MOMENTS), variance=d.download(PLANE_VARIANCE),
                hlen=d.download(PLANE_HISTORY_LENGTH))


def reference(planes, plane, mats, cam_prev, cam_cur, w, h, rad_prev, rad_cur, mom, hlen, **kw):
    (d0, n0, i0), (d1, n1, i1) = planes
    return VM.reproject(R.Camera(cam_cur, w, h), R.Camera(cam_prev, w, h), rad_cur, rad_prev, d1, d0, n1, n0, mom, hlen, i1, i0, plane,
                        table=M.delta_table(mats[1], mats[0]), **kw)


# ------------------------------------------------------------------------------------------------
# 1: option state
# ------------------------------------------------------------------------------------------------
def test_option_and_plane_state():
    w, h = 64, 48
    lib = _lib.load()
    d = SVGFDenoiser()
    d.init(w, h)
    ctx = d._ctx
    ptr, size, rows = C.c_void_p(), C.c_size_t(), C.c_uint32()
    get = lambda: lib.neb_get_plane(ctx, PLANE_PREV_POINT, 0, C.byref(ptr), C.byref(size), C.byref(rows))  # noqa: E731
    buf = np.zeros((h, w, 4), F)
    assert lib.neb_set_option(ctx, b"svgf_vertex_motion", 1) == NEB_ERR_STATE and b"svgf_motion" in lib.neb_last_error(ctx)
    d.set_option("svgf_reproject", 1)
    assert lib.neb_set_option(ctx, b"svgf_vertex_motion", 1) == NEB_ERR_STATE  # reprojection alone is not enough
    # the plane is absent with the option off, for every entry point
    assert get() != 0 and b"svgf_vertex_motion" in lib.neb_last_error(ctx)
    assert lib.neb_upload_rows(ctx, PLANE_PREV_POINT, 0, 0, h, buf.ctypes.data_as(C.c_void_p), None) != 0
    assert lib.neb_download_rows(ctx, PLANE_PREV_POINT, 0, 0, h, buf.ctypes.data_as(C.c_void_p), None) != 0
    assert lib.neb_svgf_snapshot_vertices(ctx, None) == NEB_ERR_STATE
    d.set_option("svgf_motion", 1)
    for bad in (2, -1):
        assert lib.neb_set_option(ctx, b"svgf_vertex_motion", bad) == NEB_ERR_INVALID_ARG
    assert get() != 0
    d.set_option("svgf_vertex_motion", 1)
    assert get() == 0 and size.value == 16 * w and rows.value == h
    assert (d.download(PLANE_PREV_POINT, 0).view(np.uint8) == 0xFF).all()  # unwritten: every pixel the sentinel, not a point at the origin
    assert lib.neb_get_plane(ctx, PLANE_PREV_POINT, 1, C.byref(ptr), C.byref(size), C.byref(rows)) == NEB_ERR_INVALID_ARG  # one slot
    assert lib.neb_set_option(ctx, b"svgf_motion", 0) == NEB_ERR_STATE and b"svgf_vertex_motion" in lib.neb_last_error(ctx)
    assert get() == 0 and d.download(PLANE_SUBMESH_ID).shape == (h, w)  # (the refusal turned nothing off)
    assert lib.neb_svgf_snapshot_vertices(ctx, None) == 0  # no scene: nothing to roll, no error
    # upload and download, then neb_resize re-creates the plane, all-sentinel, at the new size
    d.upload(PLANE_PREV_POINT, 0, np.full((h, w, 4), 3.0, F))
    assert (d.download(PLANE_PREV_POINT, 0) == 3.0).all()
    d.resize(w + 8, h)
    assert d.download(PLANE_PREV_POINT, 0).shape == (h, w + 8, 4) and (d.download(PLANE_PREV_POINT, 0).view(np.uint8) == 0xFF).all()
    d.set_option("svgf_vertex_motion", 0)
    assert get() != 0
    d.set_option("svgf_motion", 0)
    d.destroy()
    # through the renderer: needs motion_vectors; present and all-sentinel after a raycast with nothing deformed
    r = DeferredRenderer()
    r.temporal_reprojection = True
    r.vertex_motion = True
    with pytest.raises(NebError):
        r.init(w, h)
    sc = clone(cornell_parts(textured=False))
    r = vm_renderer(w, h)
    for f in (1, 2):
        raycast(r, sc, cornell_camera(), f)
        assert all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: nothing deformed -- svgf_motion = 1 alone, bit for bit
# ------------------------------------------------------------------------------------------------
def test_with_nothing_deformed_every_pixel_equals_svgf_motion_alone():
    from motion_cases import H, W
    sc0 = cornell_parts()
    cam_prev, cam_cur = cameras("cornell", CAMERA_MOVE)
    mats = moved_matrices(sc0, [2], small_transform("rotate"))
    r, planes, plane, mm, _ = two_frames(sc0, lambda r: r.update_transforms([2], mats), cam_prev, cam_cur, W, H)
    assert all_sentinel(plane) and not np.array_equal(mm[0], mm[1])
    rad_prev, rad_cur, mom, hlen = seeded_history(W, H, 23)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    on = outputs(r.svgf)
    r.svgf.set_option("svgf_vertex_motion", 0)  # the same planes through the per-submesh arm
    r.svgf.upload(PLANE_RADIANCE, SLOT_CURRENT, rad_cur)
    r.svgf.submit_temporal_accumulation()
    off = outputs(r.svgf)
    r.destroy()
    assert (off["hlen"][planes[1][2] == 2] > 1).mean() > 0.5  # (the moved box does take history: the arms are not trivially equal)
    for k in on:
        assert np.array_equal(on[k].view(np.uint8), off[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------
# 3: the plane against float64
# ------------------------------------------------------------------------------------------------
def _updates(kind, sc0, deform):
    """-> apply(renderer): the updates of one way a deformation arrives, between the two raycasts"""
    shift = moved_matrices(sc0, [SHORT_BOX], small_transform("translate"))
    if kind in ("all", "positions", "partial"):
        return lambda r: update(r, shaped(sc0, deform, kind)[0])
    if kind == "two updates":
        half = {SHORT_BOX: twist_and_shear(sc0, SHORT_BOX, angle_deg=1.0, shear=0.005)}
        return lambda r: (update(r, shaped(sc0, half, "all")[0]), update(r, shaped(sc0, deform, "all")[0]))
    if kind == "two ranges":  # two disjoint partial ranges of the one geometry in two calls: the roll's span is their union, gap included
        d = deform[SHORT_BOX]
        n = d["positions"].shape[0]
        parts = [{SHORT_BOX: dict(first_vertex=a, **{k: d[k][a:b] for k in ("positions", "normals", "tangents")})} for a, b in ((n // 8, n // 4), (n // 2, 3 * n // 4))]
        return lambda r: (update(r, parts[1]), update(r, parts[0]))
    if kind == "deform then move":
        return lambda r: (update(r, shaped(sc0, deform, "all")[0]), r.update_transforms([SHORT_BOX], shift))
    if kind == "move then deform":
        return lambda r: (r.update_transforms([SHORT_BOX], shift), update(r, shaped(sc0, deform, "all")[0]))
    if kind == "device":
        return lambda r: update_device(r, shaped(sc0, deform, "all")[0])
    raise ValueError(kind)


PLANE_KINDS = ["all", "positions", "partial", "two updates", "two ranges", "deform then move", "move then deform", "device"]


@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_plane_against_float64(kind):
    """The plane read back after a deformation between two raycasts against vertex_motion_ref.prev_point_plane on the scene the updates
    left.  The flagged mask may differ on silhouette pixels where the two casters pick different triangles: at no more than
    test_refit_gpu.TIE_CAP pixels.  On every pixel both flag, the oct16 normal is within one code per component and P_h is within P_BAR
    of the point's linear depth.  A further raycast with no update in between is all-sentinel: the roll has taken every updated range."""
    sc0, deform, _, w, h = cornell_case()
    cam = cornell_camera()
    r, planes, plane, mm, sc = two_frames(sc0, _updates(kind, sc0, deform), cam, cam, w, h)
    raycast(r, sc, cam, 3)
    rolled = all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    r.destroy()
    ref = VM.prev_point_plane(sc0, sc, mm[0], cam, w, h, dirty=[SHORT_BOX])
    Pg, eg, has = VM.plane_fields(plane)
    assert np.array_equal(has, ~is_sentinel(plane)) and not plane[~has][:, :3].any()
    assert not has[planes[1][2] != SHORT_BOX].any()  # only the deformed submesh's pixels
    both = has & ref["flagged"]
    mask_diff = int((has != ref["flagged"]).sum())
    codes = np.abs(VM.half_order(eg[both]) - VM.half_order(VM.oct16_codes(ref["N"][both]))).max(axis=-1)
    normal_diff = int((codes > 1).sum())
    rel = np.linalg.norm(Pg[both].astype(np.float64) - ref["P"][both], axis=-1) / ref["depth"][both]
    print(f"[plane, {kind}] {int(both.sum())} px flagged by both, mask differs at {mask_diff}, normal off by more than one code at {normal_diff}; "
          f"worst |dP| / depth {rel.max():.3e}")
    assert both.sum() > 1000
    assert mask_diff <= TIE_CAP
    assert normal_diff == 0
    assert rel.max() <= P_BAR, rel.max()
    assert rolled


# ------------------------------------------------------------------------------------------------
# 4: the kernel against the reference, on the device's own planes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda k: CASE_IDS[k])
def test_kernel_matches_reference(case):
    name, cam_move = CASES[case]
    sc0, deform, _, w, h = SCENES[name]()
    cam_prev, cam_cur = cameras(name, cam_move)
    r, planes, plane, mm, _ = two_frames(sc0, lambda r: update(r, shaped(sc0, deform, "all")[0]), cam_prev, cam_cur, w, h)
    rad_prev, rad_cur, mom, hlen = seeded_history(w, h, 87 + case)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    got = outputs(r.svgf)
    r.destroy()
    want = reference(planes, plane, mm, cam_prev, cam_cur, w, h, rad_prev, rad_cur, mom, hlen)
    hd, wd = h // 8 * 8, w // 8 * 8
    keep = ~want["near"]
    n_near = int(want["near"].sum())
    on = np.isin(planes[1][2], list(deform))[:hd, :wd]
    took = want["n_prev"] > 0
    print(f"[{CASE_IDS[case]}] deformed submesh covers {int(on.sum())} px, per-vertex motion on {int(want['per_vertex'].sum())}, history taken on "
          f"{took[on].mean():.3f} of them; {n_near} pixels ({n_near / (hd * wd):.2e}) near a threshold, left out")
    assert n_near < NEAR_CAP * hd * wd
    assert on.sum() > 100 and np.array_equal(want["per_vertex"], on)
    assert took[on].mean() >= KEPT_FLOOR
    g, x = got["radiance"][:hd, :wd][keep], want["radiance"][:hd, :wd][keep]
    bad = np.abs(g - x) > 1e-5 * np.abs(x) + 1e-7
    assert not bad.any(), f"{int(bad.any(axis=-1).sum())} pixels off by > 1e-5 relative, worst {np.abs(g - x).max():.3e}"
    for k in ("moments", "variance"):
        assert half_ulp_mismatch(got[k][:hd, :wd][keep], want[k][:hd, :wd][keep]) == 0.0, k
    assert np.array_equal(got["hlen"][:hd, :wd][keep], want["hlen"][:hd, :wd][keep])


# ------------------------------------------------------------------------------------------------
# 5: the roll
# ------------------------------------------------------------------------------------------------
def test_roll():
    sc0, deform, _, w, h = cornell_case(textured=False)
    cam = cornell_camera()
    calls = shaped(sc0, deform, "all")[0]
    # deform -> raycast -> raycast with no further update: the second plane is all-sentinel
    r, _, plane, _, sc = two_frames(sc0, lambda r: update(r, calls), cam, cam, w, h)
    assert (~is_sentinel(plane)).sum() > 1000
    raycast(r, sc, cam, 3)
    assert all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    # a device-sourced update refused on the device marks nothing
    nan = deform[SHORT_BOX]["positions"].copy()
    nan[5, 1] = np.nan
    r.update_vertices_device(SHORT_BOX, torch.from_numpy(nan).cuda(), mirror=False)
    raycast(r, sc, cam, 4)
    assert all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    assert r.update_status() == {"accepted": 0, "refused": 1}
    def assert_plane(plane, sc_prev, sc_cur):
        ref = VM.prev_point_plane(sc_prev, sc_cur, matrices(sc_prev), cam, w, h, dirty=[SHORT_BOX])
        Pg, _, has = VM.plane_fields(plane)
        both = has & ref["flagged"]
        assert both.sum() > 1000 and int((has != ref["flagged"]).sum()) <= TIE_CAP
        rel = np.linalg.norm(Pg[both].astype(np.float64) - ref["P"][both], axis=-1) / ref["depth"][both]
        assert rel.max() <= P_BAR, rel.max()

    # snapshot_vertices without a raycast: the box goes back to its first pose (the previous pools hold the twisted one), the snapshot
    # takes that pose and clears the flags -- the next raycast is all-sentinel, and the one after a further update compares against
    # the pose the snapshot saw, not against the twisted one
    back = {SHORT_BOX: {k: sc0.geometries[SHORT_BOX][k] for k in ("positions", "normals", "tangents")}}
    update(r, shaped(sc, back, "all")[0])
    r.svgf.snapshot_vertices()
    at_snapshot = clone(sc)
    raycast(r, sc, cam, 5)
    assert all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    update(r, calls)
    raycast(r, sc, cam, 6)
    assert_plane(r.svgf.download(PLANE_PREV_POINT), at_snapshot, sc)
    # neb_gi_set_scene resets the pools and the spans: a new scene in another pose, an update still unrolled when it is set
    update(r, shaped(sc, back, "all")[0])
    posed = with_arrays(sc0, {SHORT_BOX: twisted(sc0, 3)})
    sc2 = clone(posed)
    for f in (7, 8):
        raycast(r, sc2, cam, f)
        assert all_sentinel(r.svgf.download(PLANE_PREV_POINT))
    update(r, calls)
    raycast(r, sc2, cam, 9)
    plane = r.svgf.download(PLANE_PREV_POINT)
    r.destroy()
    assert_plane(plane, posed, sc2)


# ------------------------------------------------------------------------------------------------
# 6: two streams
# ------------------------------------------------------------------------------------------------
def test_an_update_on_a_side_stream_gives_the_single_stream_plane():
    sc0, _, _, w, h = cornell_case(textured=False)
    cam = cornell_camera()
    outs = []
    for mode in ("single", "side"):
        sc = clone(sc0)
        r = vm_renderer(w, h)
        main, side = torch.cuda.current_stream(), torch.cuda.Stream()
        planes = []
        for f in range(1, 6):
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f, stream=main.cuda_stream))
            if f > 1:
                update(r, shaped(sc0, {SHORT_BOX: twisted(sc0, f - 1)}, "all")[0], stream=(side if mode == "side" else main).cuda_stream)
            r.submit_commands_gbuffer()
            planes.append(r.svgf.download(PLANE_PREV_POINT, 0, stream=main.cuda_stream))
        torch.cuda.synchronize()
        r.destroy()
        outs.append(planes)
    assert (~is_sentinel(outs[0][-1])).sum() > 1000
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------
# 7: painted object
# ------------------------------------------------------------------------------------------------
def _painted(rest, sc, cam, depth, ids, w, h):
    """f of the REST-POSE object point on the patch (the same for a material point however the patch is deformed), of the world point
    elsewhere"""
    P = R.world_points64(cam, depth)
    eye = [np.eye(4)] * len(rest.geometries)
    rest_pt = VM.prev_point_plane(rest, sc, eye, cam, w, h, dirty=[V.RUG])
    sel = (ids == V.RUG) & rest_pt["flagged"]
    P[sel] = rest_pt["P"][sel]
    return R.paint(P), sel


def test_painted_patch_follows_its_deformation():
    """radiance[hist] = f(rest-pose object point each pixel of the patch saw in the previous frame), radiance[cur] = f at this frame's;
    alpha = 1, n = 255, static camera.  On patch pixels with four valid taps the worst error of the new arm is at most a tenth of the
    worst error of the same planes through svgf_motion = 1 alone (DESIGN.md 3.6a recorded factors of 40 - 200 for rigid moves).
    Measured on an MI355X: see DESIGN.md 3.6b."""
    sc0, deform, _, w, h = room_case()
    rest = V.beamed_room()
    cam = room_camera()
    r, planes, plane, mm, sc = two_frames(sc0, lambda r: update(r, shaped(sc0, deform, "all")[0]), cam, cam, w, h)
    f_prev, s_prev = _painted(rest, sc0, cam, planes[0][0], planes[0][2], w, h)
    f_cur, s_cur = _painted(rest, sc, cam, planes[1][0], planes[1][2], w, h)
    mom = np.zeros((h, w, 2), np.float16)
    hlen = np.full((h, w), 255, np.uint8)
    d = r.svgf
    d.set_constants(alpha=1.0)
    seed_planes(d, f_prev, f_cur, mom, hlen)
    d.submit_temporal_accumulation()
    got = d.download(PLANE_RADIANCE)
    d.set_option("svgf_vertex_motion", 0)  # the same planes through svgf_motion = 1 alone
    d.upload(PLANE_RADIANCE, SLOT_CURRENT, f_cur)
    d.submit_temporal_accumulation()
    alone = d.download(PLANE_RADIANCE)
    r.destroy()
    want = reference(planes, plane, mm, cam, cam, w, h, f_prev, f_cur, mom, hlen, alpha=1.0)
    hd, wd = h // 8 * 8, w // 8 * 8
    # four valid taps, each on a patch pixel of the previous frame whose rest-pose point is known
    all4 = np.zeros((h, w), bool)
    all4[:hd, :wd] = want["valid"].all(axis=0)
    all4 &= s_cur
    fx, fy = want["q"]
    ys, xs = np.nonzero(all4)
    x0, y0 = np.floor(fx[ys, xs]).astype(int), np.floor(fy[ys, xs]).astype(int)
    taps_known = np.ones(len(ys), bool)
    for t in range(4):
        taps_known &= s_prev[np.clip(y0 + (t >> 1), 0, h - 1), np.clip(x0 + (t & 1), 0, w - 1)]
    all4[ys[~taps_known], xs[~taps_known]] = False
    assert all4.sum() >= 0.5 * s_cur.sum(), (all4.sum(), s_cur.sum())
    ref = f_cur[all4][:, :3].astype(np.float64)
    rel = np.abs(got[all4][:, :3] - ref) / ref
    rel_alone = np.abs(alone[all4][:, :3] - ref) / ref
    print(f"[painted patch] four valid taps on {all4.sum() / s_cur.sum():.3f} of the patch's {int(s_cur.sum())} px; vertex motion max rel error "
          f"{rel.max():.2e} (mean {rel.mean():.2e}); svgf_motion alone max {rel_alone.max():.2e} (mean {rel_alone.mean():.2e})")
    assert rel.max() <= 0.1 * rel_alone.max(), (rel.max(), rel_alone.max())


# ------------------------------------------------------------------------------------------------
# 8: what a user sees
# ------------------------------------------------------------------------------------------------
def _twist_pose(sc0, f):
    """the short box at frame f: 2 degrees per frame, back and forth between +6 and -6 degrees"""
    k = ((f + 3) % 12) - 3
    k = k if k <= 3 else 6 - k
    return twist_and_shear(sc0, SHORT_BOX, angle_deg=2.0 * k, shear=0.01 * k)


def _render_twisting_box(sc0, cam, w, h, frames, mode):
    sc = clone(sc0)
    r = DeferredRenderer()
    r.temporal_reprojection = mode != "undenoised"
    r.motion_vectors = mode != "undenoised"
    r.vertex_motion = mode == "vertex"
    r.init(w, h)
    for f in range(1, frames + 1):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        update(r, shaped(sc0, {SHORT_BOX: _twist_pose(sc0, f)}, "all")[0])
        r.submit_commands_gbuffer()
        r.submit_commands_pbr_lighting()
        r.submit_commands_gi_pathtrace()
        if mode != "undenoised":
            assert r.submit_commands_svgf_denoising()
        r.end_frame()
    img = r.svgf.download(PLANE_RADIANCE)
    ids = r.svgf.download(PLANE_SUBMESH_ID) if mode != "undenoised" else None
    r.destroy()
    return img, ids


def test_what_the_user_sees_when_a_box_twists_every_frame():
    """Cornell parts (textured), 256 x 256, static camera, the short box twisting 2 degrees per frame back and forth for 16 frames, 1 spp
    GI + SVGF through DeferredRenderer; the last frame against 256 spp at the final pose (16 dispatches of 16 spp, no SVGF), relative L2
    over the box's pixels.  Required: vertex_motion strictly below motion_vectors alone.  Measured on an MI355X: see DESIGN.md 3.6b.
    The short box wears the tall box's textured material here: its own has no albedo map, and neb_gbuffer_raycast writes the albedo of
    such a material as zero -- the box is black in every arm and in the converged image, and a relative error over its pixels is 0 / 0."""
    w = h = 256
    n = 16
    sc0 = cornell_parts()
    sc0.geometries[SHORT_BOX]["material"] = sc0.geometries[2]["material"]
    cam = cornell_camera()
    conv_sc = with_arrays(sc0, {SHORT_BOX: _twist_pose(sc0, n)})
    conv = DeferredRenderer()
    conv.init(w, h)
    conv.gi_ui.gi_samples_per_pixel = 16
    acc = np.zeros((h, w, 4), np.float64)
    for k in range(16):
        conv.begin_frame(RenderInfo(scene=conv_sc, camera=cam, frame_index=1000 + k))
        conv.submit_commands_gbuffer()
        conv.submit_commands_pbr_lighting()
        conv.submit_commands_gi_pathtrace()
        acc += conv.svgf.download(PLANE_RADIANCE)
        conv.end_frame()
    conv.destroy()
    ref = (acc / 16)[..., :3]
    img, ids = {}, None
    for mode in ("vertex", "motion", "undenoised"):
        img[mode], i = _render_twisting_box(sc0, cam, w, h, n, mode)
        ids = i if i is not None else ids
    box = ids == SHORT_BOX
    assert box.sum() > 1000
    err = {m: rel_l2(img[m][box][:, :3], ref[box]) for m in img}
    print(f"[twisting box, {n} frames, 256x256] relative L2 to 256 spp over the box's {int(box.sum())} pixels: vertex_motion {err['vertex']:.4f}, "
          f"motion_vectors alone {err['motion']:.4f}, undenoised {err['undenoised']:.4f}")
    assert err["vertex"] < err["motion"]


# ------------------------------------------------------------------------------------------------
# 9: memory
# ------------------------------------------------------------------------------------------------
def test_a_hundred_deformations_hold_no_more_device_memory():
    sc0, _, _, w, h = cornell_case(textured=False)
    cam = cornell_camera()
    poses = [shaped(sc0, {SHORT_BOX: twisted(sc0, k)}, "all")[0] for k in range(-3, 4)]
    warm = vm_renderer(w, h)
    raycast(warm, clone(sc0), cam, 1)
    warm.destroy()
    before = _free_bytes()
    sc = clone(sc0)
    r = vm_renderer(w, h)
    free = {}
    for f in range(1, 105):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        update(r, poses[f % len(poses)])
        r.submit_commands_gbuffer()
        if f in (4, 104):
            free[f] = _free_bytes()
    assert (~is_sentinel(r.svgf.download(PLANE_PREV_POINT))).sum() > 1000
    r.svgf.set_option("svgf_vertex_motion", 0)  # gives the plane and the pools back
    off = _free_bytes()
    r.destroy()
    after = _free_bytes()
    print(f"[vertex motion soak] free device memory after cycle 4 / 104: {free[4] >> 20} / {free[104] >> 20} MB; with the option off "
          f"{off >> 20} MB; before init / after destroy: {before >> 20} / {after >> 20} MB")
    assert free[4] - free[104] < 4 << 20, free
    assert off >= free[104], (off, free[104])
    assert before - after < 4 << 20, (before, after)
