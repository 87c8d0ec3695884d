"""GPU tests of option svgf_motion: the delta kernel and the motion arm of the reprojecting temporal kernel against
the CPU reference (tests/motion_ref.py) on G-buffers and ids from the library's own producer with an update_transforms between the two
frames, the painted object, the static scene, the option's off state, the id plane, what a user sees when a box moves every frame,
streams, lifetime and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import motion_ref as M
import reproject_ref as R
from motion_cases import BOXES, CORNELL_CASES, H, W, cameras, small_transform
from nebulae_amd import _lib
from nebulae_amd import scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import (PLANE_DEPTH, PLANE_HISTORY_LENGTH, PLANE_MOMENTS, PLANE_NORMAL, PLANE_RADIANCE, PLANE_SUBMESH_ID,
                              PLANE_VARIANCE, SLOT_CURRENT, SLOT_HISTORY, NebError, SVGFDenoiser)
from svgf_cases import half_ulp_mismatch, rel_l2
from test_refit_gpu import TIE_CAP, _free_bytes, clone, cornell_camera, cornell_parts, moved_matrices, with_matrices, world_transform
from test_reproject_cpu import moved as moved_camera
from test_reproject_gpu import _frames, _scene, seeded_history

pytestmark = pytest.mark.gpu
NEB_ERR_INVALID_ARG, NEB_ERR_STATE = -1, -4
F = np.float32


def motion_renderer(w, h, motion=True):
    r = DeferredRenderer()
    r.temporal_reprojection = True
    r.motion_vectors = motion
    r.init(w, h)
    return r


def two_frames(sc0, indices, mats, cam_prev, cam_cur, w, h):
    """frame 1 at cam_prev, update_transforms, frame 2 at cam_cur, through neb_gbuffer_raycast with the option on.
    -> (renderer at frame 2 (cur = 0, hist = 1), planes [(depth, normal, id)] of the two frames, (m_hist, m_cur))"""
    sc = clone(sc0)
    r = motion_renderer(w, h)
    planes = []
    m_hist = np.stack([g["M"] for g in sc.geometries])
    for f, cam in ((1, cam_prev), (2, cam_cur)):
        if f == 2 and len(indices):
            r.update_transforms(indices, mats)
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        r.submit_commands_gbuffer()
        planes.append(tuple(r.svgf.download(p) for p in (PLANE_DEPTH, PLANE_NORMAL, PLANE_SUBMESH_ID)))
    m_cur = np.stack([g["M"] for g in sc.geometries])
    return r, planes, (m_hist, m_cur)


def seed_planes(d, rad_prev, rad_cur, mom, hlen):
    d.upload(PLANE_RADIANCE, SLOT_CURRENT, rad_cur)
    d.upload(PLANE_RADIANCE, SLOT_HISTORY, rad_prev)
    d.upload(PLANE_MOMENTS, SLOT_HISTORY, mom)
    d.upload(PLANE_HISTORY_LENGTH, SLOT_HISTORY, hlen)


def outputs(d):
    return dict(radiance=d.download(PLANE_RADIANCE), moments=d.download(PLANE_MOMENTS), variance=d.download(PLANE_VARIANCE),
                hlen=d.download(PLANE_HISTORY_LENGTH))


def reference(planes, mats, cam_prev, cam_cur, w, h, rad_prev, rad_cur, mom, hlen, table=True, **kw):
    (d0, n0, i0), (d1, n1, i1) = planes
    return M.reproject(R.Camera(cam_cur, w, h), R.Camera(cam_prev, w, h), rad_cur, rad_prev, d1, d0, n1, n0, mom, hlen, i1, i0,
                       table=M.delta_table(mats[1], mats[0]) if table else None, **kw)


# ------------------------------------------------------------------------------------------------
# the delta table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["translate", "rotate", "scale"])
def test_delta_table_has_the_bits_of_the_float64_reference(kind):
    sc0 = cornell_parts(textured=False)
    cam = cornell_camera()
    for T in (world_transform(kind), small_transform(kind)):
        mats = moved_matrices(sc0, BOXES, T)
        r, _, (m_hist, m_cur) = two_frames(sc0, BOXES, mats, cam, cam, 64, 48)
        got = r.svgf.debug_delta_table(len(sc0.geometries))
        want = M.delta_table(m_cur, m_hist)
        r.destroy()
        assert (want["flag"] == [0, 1, 1, 0, 0]).all()
        assert np.array_equal(got.view(np.uint32), want["entries"].view(np.uint32)), np.abs(got - want["entries"]).max()


def test_delta_table_flags_a_singular_matrix():
    sc0 = cornell_parts(textured=False)
    cam = cornell_camera()
    flat = np.eye(4)
    flat[1, 1] = 0.0
    mats = moved_matrices(sc0, BOXES, flat)
    r, _, (m_hist, m_cur) = two_frames(sc0, BOXES, mats, cam, cam, 64, 48)
    got = r.svgf.debug_delta_table(len(sc0.geometries))
    want = M.delta_table(m_cur, m_hist)
    assert (want["flag"] == [0, 2, 2, 0, 0]).all()
    assert np.array_equal(got.view(np.uint32), want["entries"].view(np.uint32))
    # its pixels take no history: the output is the current frame, history length 1
    rad_prev, rad_cur, mom, hlen = seeded_history(64, 48, 3)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, np.maximum(hlen, 1))
    r.svgf.submit_temporal_accumulation()
    out = outputs(r.svgf)
    ids = r.svgf.download(PLANE_SUBMESH_ID)
    r.destroy()
    on = np.isin(ids, BOXES)
    assert on.sum() > 0
    assert np.array_equal(out["radiance"][on], rad_cur[on]) and (out["hlen"][on] == 1).all()


# ------------------------------------------------------------------------------------------------
# the kernel against the reference
# ------------------------------------------------------------------------------------------------
def _parity(tag, sc0, indices, T, cam_prev, cam_cur, w, h, seed):
    mats = moved_matrices(sc0, indices, T)
    r, planes, mm = two_frames(sc0, indices, mats, cam_prev, cam_cur, w, h)
    rad_prev, rad_cur, mom, hlen = seeded_history(w, h, seed)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    got = outputs(r.svgf)
    r.destroy()
    want = reference(planes, mm, cam_prev, cam_cur, w, h, rad_prev, rad_cur, mom, hlen)
    hd, wd = h // 8 * 8, w // 8 * 8
    keep = ~want["near"]
    n_near = int(want["near"].sum())
    on = np.isin(planes[1][2], indices)[:hd, :wd]
    took = want["n_prev"] > 0
    print(f"[{tag}] moved objects cover {int(on.sum())} px, history taken on {took[on].mean():.3f} of them; {n_near} pixels "
          f"({n_near / (w * h):.2e} of the image) near a threshold, excluded")
    assert n_near <= 5e-4 * w * h
    assert on.sum() > 0 and want["moved"][on & R.surface(planes[1][0])[:hd, :wd]].all()
    assert took[on].mean() >= 0.5
    g, x = got["radiance"][:hd, :wd][keep], want["radiance"][:hd, :wd][keep]
    bad = np.abs(g - x) > 1e-5 * np.abs(x) + 1e-7
    assert not bad.any(), f"{int(bad.any(axis=-1).sum())} pixels off by > 1e-5 relative, worst {np.abs(g - x).max():.3e}"
    for k in ("moments", "variance"):
        assert half_ulp_mismatch(got[k][:hd, :wd][keep], want[k][:hd, :wd][keep]) == 0.0, k
    assert np.array_equal(got["hlen"][:hd, :wd][keep], want["hlen"][:hd, :wd][keep])


@pytest.mark.parametrize("case", range(len(CORNELL_CASES)), ids=lambda k: f"{CORNELL_CASES[k][0]}-{'pan' if CORNELL_CASES[k][1] else 'static'}")
def test_kernel_matches_reference_on_the_cornell_parts(case):
    kind, cam_move = CORNELL_CASES[case]
    cam_prev, cam_cur = cameras(cam_move)
    _parity(f"cornell parts {kind}, camera {cam_move}", cornell_parts(), BOXES, small_transform(kind), cam_prev, cam_cur, W, H, 41 + case)


def test_kernel_matches_reference_on_the_sponza_standin_at_1080p():
    sc0 = _scene("sponza")
    moving = list(range(4, len(sc0.geometries), 9))[:11]
    assert len(moving) == 11
    T = np.eye(4)
    T[3, :3] = (0.03, 0.0, 0.04)  # 5 cm
    cam_prev = S.sponza_camera()
    cam_cur = moved_camera(cam_prev, pan=(0.05, 0.0, 0.0), yaw_deg=0.2)
    _parity("sponza stand-in 1080p, 11 submeshes moved 5 cm", sc0, moving, T, cam_prev, cam_cur, 1920, 1080, 77)


# ------------------------------------------------------------------------------------------------
# painted object
# ------------------------------------------------------------------------------------------------
def _painted(cam, depth, ids, mats):
    Pw = R.world_points64(cam, depth)
    P = Pw.copy()
    for gi in BOXES:
        sel = ids == gi
        P[sel] = M.object_points64(Pw, ids, gi, mats[gi])[sel]
    return R.paint(P)


@pytest.mark.parametrize("kind", ["translate", "rotate", "scale"])
def test_painted_object_follows_its_box(kind):
    """radiance[hist] = f(object-space point each pixel of the moved boxes saw in the previous frame), radiance[cur] = f at this frame's
    points; alpha = 1, n = 255, static camera, the boxes moved a few pixels: on box pixels with four valid taps the output is f at the
    current points to <= 1e-3 relative; the same planes through svgf_motion = 0 (plain reprojection, which still passes its normal and
    plane tests for so small a step and so takes the history of the wrong surface point) miss by >= 20 x that in the mean.
    The CPU reference on oracle G-buffers (test_motion_cpu.py): motion mean 3.4e-6 / 2.9e-6 / 3.3e-6, plain 1.6e-3 / 5.4e-4 / 6.9e-4."""
    sc0 = cornell_parts()
    cam = cornell_camera()
    mats = moved_matrices(sc0, BOXES, small_transform(kind))
    r, planes, mm = two_frames(sc0, BOXES, mats, cam, cam, W, H)
    f_prev, f_cur = _painted(cam, planes[0][0], planes[0][2], mm[0]), _painted(cam, planes[1][0], planes[1][2], mm[1])
    mom = np.zeros((H, W, 2), np.float16)
    hlen = np.full((H, W), 255, np.uint8)
    d = r.svgf
    d.set_constants(alpha=1.0)
    seed_planes(d, f_prev, f_cur, mom, hlen)
    d.submit_temporal_accumulation()
    got = d.download(PLANE_RADIANCE)
    d.set_option("svgf_motion", 0)  # the same planes through plain reprojection
    d.upload(PLANE_RADIANCE, SLOT_CURRENT, f_cur)
    d.submit_temporal_accumulation()
    plain = d.download(PLANE_RADIANCE)
    r.destroy()
    want = reference(planes, mm, cam, cam, W, H, f_prev, f_cur, mom, hlen, alpha=1.0)
    on = np.isin(planes[1][2], BOXES)
    all4 = want["valid"].all(axis=0) & on
    assert all4.sum() >= 0.5 * on.sum()
    ref = f_cur[all4][:, :3].astype(np.float64)
    rel = np.abs(got[all4][:, :3] - ref) / ref
    rel_plain = np.abs(plain[all4][:, :3] - ref) / ref
    print(f"[painted object {kind}] four valid taps on {all4.sum() / on.sum():.3f} of the boxes' pixels; motion max rel error {rel.max():.2e} "
          f"(mean {rel.mean():.2e}); svgf_motion = 0 max {rel_plain.max():.2e} (mean {rel_plain.mean():.2e})")
    assert rel.max() <= 1e-3, rel.max()
    assert rel_plain.mean() >= 20 * rel.mean()


# ------------------------------------------------------------------------------------------------
# static scene; option off
# ------------------------------------------------------------------------------------------------
def test_static_scene_equals_plain_reprojection_where_the_taps_carry_the_pixels_own_id():
    sc0 = cornell_parts()
    cam_prev, cam_cur = cameras(dict(pan=(0.04, 0.0, 0.0), yaw_deg=-0.4))
    r, planes, mm = two_frames(sc0, [], None, cam_prev, cam_cur, W, H)
    assert np.array_equal(mm[0], mm[1])
    rad_prev, rad_cur, mom, hlen = seeded_history(W, H, 19)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    on = outputs(r.svgf)
    r.svgf.set_option("svgf_motion", 0)
    r.svgf.upload(PLANE_RADIANCE, SLOT_CURRENT, rad_cur)
    r.svgf.submit_temporal_accumulation()
    off = outputs(r.svgf)
    r.destroy()
    want = reference(planes, mm, cam_prev, cam_cur, W, H, rad_prev, rad_cur, mom, hlen, table=False)
    same = np.ones((H, W), bool)
    for k in on:
        same &= (on[k].view(np.uint8).reshape(H, W, -1) == off[k].view(np.uint8).reshape(H, W, -1)).all(axis=-1)
    print(f"[static scene] {int((~same).sum())} pixels differ from svgf_motion = 0; ids differ among the taps of {int((~want['tap_ids_equal']).sum())}")
    assert same[want["tap_ids_equal"]].all()


@pytest.mark.parametrize("fuse", [1, 0])
def test_option_switched_on_and_off_is_today(fuse):
    w, h = 136, 96
    fresh = SVGFDenoiser()
    fresh.init(w, h)
    toggled = SVGFDenoiser()
    toggled.init(w, h)
    toggled.set_option("svgf_reproject", 1)
    toggled.set_option("svgf_motion", 1)
    assert toggled.download(PLANE_SUBMESH_ID).shape == (h, w) and not toggled.download(PLANE_SUBMESH_ID, SLOT_HISTORY).any()
    toggled.snapshot_transforms(SLOT_CURRENT)  # (no scene: nothing to remember, no error)
    toggled.set_option("svgf_motion", 0)
    toggled.set_option("svgf_reproject", 0)
    with pytest.raises(NebError):
        toggled.get_plane(PLANE_SUBMESH_ID)  # (the plane is gone again)
    a, b = _frames(fresh, w, h, 5, fuse), _frames(toggled, w, h, 5, fuse)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    fresh.destroy()
    toggled.destroy()


# ------------------------------------------------------------------------------------------------
# the id plane
# ------------------------------------------------------------------------------------------------
def test_id_plane_against_the_cpu_primary_hit():
    """surface <=> id != 0xFFFFFFFF exactly; ids equal those of a float64 ray caster over the scene's triangles (motion_ref.primary_ids)
    except where a primary ray passes an edge between two submeshes within rounding -- reported, and capped as test_refit_gpu caps ties."""
    sc0 = cornell_parts()
    cam = cornell_camera()
    mats = moved_matrices(sc0, BOXES, world_transform("rotate"))
    r, planes, _ = two_frames(sc0, BOXES, mats, cam, cam, W, H)
    r.destroy()
    for (depth, _, ids), sc in zip(planes, (sc0, with_matrices(sc0, BOXES, mats))):
        surf = R.surface(depth)
        assert np.array_equal(surf, ids != M.NO_SUBMESH)
        want, _ = M.primary_ids(sc, cam, W, H)
        diff = surf & (want != M.NO_SUBMESH) & (ids != want)
        print(f"[id plane] {int(surf.sum())} surface pixels, ids {sorted(set(ids[surf].tolist()))}; {int(diff.sum())} differ from the CPU primary hit")
        assert {0, 1, 2} <= set(ids[surf].tolist()) <= {0, 1, 2, 3, 4}
        assert int(diff.sum()) <= TIE_CAP


# ------------------------------------------------------------------------------------------------
# what a user sees
# ------------------------------------------------------------------------------------------------
def _box_pose(sc0, k):
    """the tall box after k steps: turned 1.2 degrees per step about a vertical axis through itself and slid 6 mm per step"""
    a = math.radians(1.2 * k)
    c, s = math.cos(a), math.sin(a)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    p = np.array([0.4, -1.0, -1.6])
    T[3, :3] = p - p @ T[:3, :3] + np.array([-0.006 * k, 0.0, 0.004 * k])
    return moved_matrices(sc0, [2], T)


def _render_moving_box(sc0, cam, w, h, frames, mode):
    sc = clone(sc0)
    r = DeferredRenderer()
    r.temporal_reprojection = mode in ("motion", "reproject")
    r.motion_vectors = mode == "motion"
    r.init(w, h)
    hist_len = None
    for f in range(1, frames + 1):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        r.update_transforms([2], _box_pose(sc0, f))
        r.submit_commands_gbuffer()
        r.submit_commands_pbr_lighting()
        r.submit_commands_gi_pathtrace()
        if mode != "undenoised":
            assert r.submit_commands_svgf_denoising()
        r.end_frame()
    img = r.svgf.download(PLANE_RADIANCE)
    if mode != "undenoised":
        hist_len = r.svgf.download(PLANE_HISTORY_LENGTH)
    ids = r.svgf.download(PLANE_SUBMESH_ID) if mode == "motion" else None
    r.destroy()
    return img, hist_len, ids


def test_what_the_user_sees_when_a_box_moves_every_frame():
    """Cornell parts (textured), 256 x 256, static camera, the tall box turning 1.2 degrees and sliding ~7 mm per frame for 16 frames, 1 spp
    GI + SVGF through DeferredRenderer; the last frame against a converged image at the final pose (mean of 16 dispatches of 16-spp GI, no
    SVGF), relative L2 over the pixels showing the moved box and over the whole image; arms: motion_vectors, temporal_reprojection only
    (the behaviour before the option), undenoised.  The frames are deterministic (seeded RNG).
    Required: over the box's pixels, motion is below reprojection only and below undenoised.  Whole image: the squared error may exceed
    reprojection only's by no more than the undenoised squared error of the pixels whose history the id test removed (they fall back to
    the frame's own sample at worst) -- the test prints that share.
    Measured on an MI355X, over the box's 2883 pixels: motion 0.504, reprojection only 0.632, undenoised 2.008 -- motion / reprojection only
    = 0.797; whole image: motion 0.368, reprojection only 0.387, undenoised 1.395, and the id test had removed no pixel's history in the last
    frame.  The gain on the box is modest: at this step plain reprojection mostly still finds (a neighbouring point's) history."""
    w = h = 256
    n = 16
    sc0 = cornell_parts()
    cam = cornell_camera()
    conv_sc = with_matrices(sc0, [2], _box_pose(sc0, n))
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
    img, hl, ids = {}, {}, None
    for mode in ("motion", "reproject", "undenoised"):
        img[mode], hl[mode], i = _render_moving_box(sc0, cam, w, h, n, mode)
        ids = i if i is not None else ids
    box = ids == 2
    assert box.sum() > 2000
    err_box = {m: rel_l2(img[m][box][:, :3], ref[box]) for m in img}
    err_all = {m: rel_l2(img[m][..., :3], ref) for m in img}
    removed = (hl["motion"] == 1) & (hl["reproject"] > 1)
    norm2 = float((ref.astype(np.float64) ** 2).sum())
    removed_err2 = float(((img["undenoised"][removed][:, :3].astype(np.float64) - ref[removed]) ** 2).sum()) / norm2
    print(f"[moving box, {n} frames, 256x256] relative L2 to the converged image over the box's {int(box.sum())} pixels: motion {err_box['motion']:.4f}, "
          f"reprojection only {err_box['reproject']:.4f}, undenoised {err_box['undenoised']:.4f}; motion / reprojection only = "
          f"{err_box['motion'] / err_box['reproject']:.3f}.  Whole image: motion {err_all['motion']:.4f}, reprojection only {err_all['reproject']:.4f}, "
          f"undenoised {err_all['undenoised']:.4f}; the id test removed the history of {removed.mean():.2e} of the pixels "
          f"(undenoised squared error there {removed_err2:.3e} of the image's)")
    assert err_box["motion"] < err_box["reproject"]
    assert err_box["motion"] < err_box["undenoised"]
    assert err_all["motion"] ** 2 <= err_all["reproject"] ** 2 + removed_err2


# ------------------------------------------------------------------------------------------------
# streams, lifetime
# ------------------------------------------------------------------------------------------------
def test_an_update_on_a_side_stream_equals_the_single_stream_run():
    sc0 = cornell_parts()
    cam = cornell_camera()
    outs = []
    for mode in ("single", "side"):
        sc = clone(sc0)
        r = motion_renderer(W, H)
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        for f in range(1, 7):
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f, stream=main.cuda_stream))
            if f > 1:
                r.update_transforms(BOXES, moved_matrices(sc0, BOXES, world_transform("rotate", f - 6)),
                                    stream=(side if mode == "side" else main).cuda_stream)
            r.submit_commands_gbuffer()
            r.submit_commands_pbr_lighting()
            r.submit_commands_gi_pathtrace()
            r.submit_commands_svgf_denoising()
            r.end_frame()
        torch.cuda.synchronize()
        outs.append([r.svgf.download(p) for p in (PLANE_RADIANCE, PLANE_MOMENTS, PLANE_HISTORY_LENGTH, PLANE_SUBMESH_ID)])
        r.destroy()
    assert float(np.abs(outs[0][0][..., :3]).max()) > 0.05
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_hundred_frames_with_an_update_each_hold_no_more_device_memory():
    sc0 = cornell_parts()
    cam = cornell_camera()
    warm = motion_renderer(W, H)
    warm.begin_frame(RenderInfo(scene=clone(sc0), camera=cam, frame_index=1))
    warm.destroy()
    before = _free_bytes()
    sc = clone(sc0)
    r = motion_renderer(W, H)
    free = {}
    for f in range(1, 105):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        r.update_transforms(BOXES, moved_matrices(sc0, BOXES, world_transform("rotate", (f % 13) - 6)))
        r.submit_commands_gbuffer()
        r.submit_commands_pbr_lighting()
        r.submit_commands_gi_pathtrace()
        r.submit_commands_svgf_denoising()
        r.end_frame()
        if f in (4, 104):
            free[f] = _free_bytes()
    assert np.isfinite(r.svgf.download(PLANE_RADIANCE)).all()
    r.destroy()
    after = _free_bytes()
    print(f"[motion soak] free device memory after frame 4 / 104: {free[4] >> 20} / {free[104] >> 20} MB; before init / after destroy: "
          f"{before >> 20} / {after >> 20} MB")
    assert free[4] - free[104] < 4 << 20, free
    assert before - after < 4 << 20, (before, after)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_unchanged():
    w, h = 64, 48
    lib = _lib.load()
    strip = SVGFDenoiser()
    strip.init(w, h, row_begin=0, row_end=32)
    assert lib.neb_set_option(strip._ctx, b"svgf_motion", 1) == NEB_ERR_STATE  # (a strip cannot turn reprojection on, so not this either)
    strip.destroy()
    d = SVGFDenoiser()
    d.init(w, h)
    ctx = d._ctx
    ptr, size, rows = C.c_void_p(), C.c_size_t(), C.c_uint32()
    get_id = lambda: lib.neb_get_plane(ctx, PLANE_SUBMESH_ID, SLOT_CURRENT, C.byref(ptr), C.byref(size), C.byref(rows))  # noqa: E731
    assert lib.neb_set_option(ctx, b"svgf_motion", 1) == NEB_ERR_STATE  # without svgf_reproject
    assert b"svgf_reproject" in lib.neb_last_error(ctx)
    assert get_id() == NEB_ERR_STATE and b"svgf_motion" in lib.neb_last_error(ctx)
    assert lib.neb_svgf_snapshot_transforms(ctx, 0, None) == NEB_ERR_STATE
    buf = np.zeros((h, w), np.uint32)
    assert lib.neb_upload_rows(ctx, PLANE_SUBMESH_ID, SLOT_CURRENT, 0, h, buf.ctypes.data_as(C.c_void_p), None) == NEB_ERR_STATE
    assert lib.neb_get_plane(ctx, 13, SLOT_CURRENT, C.byref(ptr), C.byref(size), C.byref(rows)) == NEB_ERR_INVALID_ARG
    d.set_option("svgf_reproject", 1)
    for bad in (2, -1):
        assert lib.neb_set_option(ctx, b"svgf_motion", bad) == NEB_ERR_INVALID_ARG
    assert get_id() == NEB_ERR_STATE  # (the refused values turned nothing on)
    d.set_option("svgf_motion", 1)
    assert get_id() == 0 and size.value == 4 * w and rows.value == h
    assert lib.neb_set_option(ctx, b"svgf_reproject", 0) == NEB_ERR_STATE  # turn motion off first
    assert get_id() == 0 and d.download(PLANE_HISTORY_LENGTH).shape == (h, w)  # (both planes still there)
    for bad in (2, -3, 7):
        assert lib.neb_svgf_snapshot_transforms(ctx, bad, None) == NEB_ERR_INVALID_ARG
    assert lib.neb_svgf_snapshot_transforms(ctx, SLOT_CURRENT, None) == 0  # no scene: nothing moved, no error
    n = C.c_uint32()
    tab = np.zeros((8, 32), F)
    assert lib.neb_svgf_debug_delta_table(ctx, tab.ctypes.data_as(C.POINTER(C.c_float)), 8, C.byref(n), None) == NEB_ERR_STATE
    # resize re-creates the id plane (zeroed, new size)
    d.upload(PLANE_SUBMESH_ID, SLOT_CURRENT, np.full((h, w), 7, np.uint32))
    d.resize(w + 8, h)
    assert d.download(PLANE_SUBMESH_ID).shape == (h, w + 8) and not d.download(PLANE_SUBMESH_ID).any()
    d.set_option("svgf_motion", 0)
    d.set_option("svgf_reproject", 0)
    assert get_id() == NEB_ERR_STATE
    d.destroy()
    r = DeferredRenderer()
    r.motion_vectors = True
    with pytest.raises(NebError):
        r.init(w, h)  # motion_vectors needs temporal_reprojection
