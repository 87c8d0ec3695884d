"""GPU tests of albedo demodulation (option svgf_demodulate): the demodulating temporal arms and the remodulating last
level against tests/demod_ref.py (the unchanged references fed demodulated planes), the reprojection arms, seeding, the option's off
state, the refusals, and what a user sees on a textured scene.

Inputs: svgf_cases.frame_inputs' G-buffers and radiance, the radiance multiplied by the divisor of a random R11G11B10_FLOAT albedo plane
(exact zeros, values below the floor and above 1 among its fields) -- a textured frame, whose demodulated signal is frame_inputs' own."""
import ctypes as C

import numpy as np
import pytest

import demod_ref as D
import motion_ref as M
import reproject_ref as R
import vertex_motion_ref as VM
from nebulae_amd import _lib
from nebulae_amd import scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import (PLANE_ALBEDO, PLANE_DEMOD, PLANE_DEPTH, PLANE_HISTORY_LENGTH, PLANE_MOMENTS, PLANE_NORMAL, PLANE_RADIANCE,
                              PLANE_VARIANCE, SLOT_CURRENT, SLOT_HISTORY, SVGFDenoiser)
from svgf_cases import frame_inputs, half_ulp_mismatch, rel_l2

pytestmark = pytest.mark.gpu
NEB_ERR_INVALID_ARG, NEB_ERR_STATE = -1, -4
TOL_PASS = 2e-5  # the suite's bars (tests/test_svgf_gpu.py)
TOL_E2E = 1e-4
F = np.float32


def make(W, H, L, demod=True, **options):
    d = SVGFDenoiser()
    d.init(W, H, atrous_levels=L)
    for k, v in options.items():
        d.set_option(k, v)
    if demod:
        d.set_option("svgf_demodulate", 1)
    return d


def inputs(W, H, f, shift=3):
    """-> G-buffer, textured radiance (a recognisable alpha), albedo words; the albedo plane changes with the G-buffer on the shift frame"""
    g, rad = frame_inputs(W, H, f, shift)
    albedo = D.random_albedo(np.random.default_rng(W + 7 * (f >= shift)), H, W)
    rad = rad.copy()
    rad[..., :3] = rad[..., :3] * D.divisor(albedo)
    rad[..., 3] = np.random.default_rng(100 + f).uniform(0.0, 2.0, (H, W)).astype(F)
    return g, rad, albedo


def feed(d, f, g, rad, albedo):
    d.begin_frame(f)
    d.upload(PLANE_DEPTH, SLOT_CURRENT, g["depth"])
    d.upload(PLANE_NORMAL, SLOT_CURRENT, g["normal"])
    d.upload(PLANE_RADIANCE, SLOT_CURRENT, rad)
    d.upload(PLANE_ALBEDO, 0, albedo)


def moments_tol(rad, albedo):
    return 4e-7 * float(D.demodulate(rad, D.divisor(albedo))[..., :3].max()) ** 2 + 1e-6  # test_svgf_gpu.py's formula, on the demodulated radiance


def check_temporal(tag, d, want, rad, albedo):
    got = d.download(PLANE_RADIANCE)
    tol = moments_tol(rad, albedo)
    e = rel_l2(got, want["radiance"])
    em = half_ulp_mismatch(d.download(PLANE_MOMENTS), want["moments"], abs_tol=tol)
    ev = half_ulp_mismatch(d.download(PLANE_VARIANCE), want["variance"], abs_tol=tol)
    print(f"[{tag}] temporal: radiance rel L2 {e:.3e} (bar {TOL_PASS}), moments mismatch {em:.2e}, variance mismatch {ev:.2e} (bar 1e-3)")
    assert e < TOL_PASS, (tag, e)
    assert em < 1e-3 and ev < 1e-3, (tag, em, ev)


def run_parity(W, H, L, variant, frames=4):
    d = make(W, H, L, atrous_variant=variant, svgf_profile=1)
    ref = D.DemodSVGF(W, H, L)
    for f in range(1, frames + 1):
        g, rad, albedo = inputs(W, H, f)
        feed(d, f, g, rad, albedo)
        ref.begin_frame(f, g["depth"], g["normal"], rad, albedo)  # (frame 1: the seed of a zeroed radiance[hist] is the oracle's zeroed history)
        d.submit_temporal_accumulation()
        check_temporal(f"{W}x{H} L{L} variant {variant} frame {f}", d, ref.temporal(), rad, albedo)
        d.submit_atrous_compute_wavelet()
        want = ref.atrous()
        e_demod = rel_l2(d.download(PLANE_DEMOD, 0)[..., :3], want["demod"][..., :3])
        e_rad = rel_l2(d.download(PLANE_RADIANCE), want["radiance"])
        print(f"[{W}x{H} L{L} variant {variant} frame {f}] chain: demod plane rel L2 {e_demod:.3e}, radiance[cur] {e_rad:.3e} (bar {TOL_E2E})")
        assert e_demod < TOL_E2E and e_rad < TOL_E2E, (f, e_demod, e_rad)
        assert np.array_equal(d.download(PLANE_RADIANCE)[..., 3], rad[..., 3])  # alpha carried
        d.end_frame()
    assert d.level_times()[-1] == 1.0  # the seed kernel ran for frame 1 and never again
    ref.close()
    d.destroy()


# ------------------------------------------------------------------------------------------------
# 1 / 2: the kernels against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 0], ids=["lds", "direct"])
@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_kernel_parity(L, variant):
    """96 x 64: the smallest image with an interior LDS tile and a tile boundary; the three shapes of chain_link and the default depth"""
    run_parity(96, 64, L, variant)


@pytest.mark.parametrize("variant", [1, 0], ids=["lds", "direct"])
def test_ragged_size(variant):
    """72 x 40: no multiple of the 64 x 8 tile; every pixel lies in the Dispatch(W/8, H/8) region"""
    run_parity(72, 40, 3, variant, frames=3)


def test_pixels_outside_the_dispatch_region_stay_untouched():
    W, H, L = 76, 43, 2
    d = make(W, H, L)
    g, rad, albedo = inputs(W, H, 1)
    feed(d, 1, g, rad, albedo)
    d.submit_temporal_accumulation()
    d.submit_atrous_compute_wavelet()
    out, dem = d.download(PLANE_RADIANCE), d.download(PLANE_DEMOD, 0)
    outside = np.ones((H, W), bool)
    outside[:H // 8 * 8, :W // 8 * 8] = False
    assert np.array_equal(out[outside].view(np.uint32), rad[outside].view(np.uint32))
    assert not dem[outside][..., :3].any()  # (the seed of the zeroed radiance[hist])
    d.destroy()


# ------------------------------------------------------------------------------------------------
# 3: the reprojection arms
# ------------------------------------------------------------------------------------------------
def check_reprojected(tag, got, want, w, h):
    hd, wd = h // 8 * 8, w // 8 * 8
    keep = ~want["near"]
    n_near = int(want["near"].sum())
    print(f"[{tag}] {n_near} pixels ({n_near / (w * h):.2e} of the image) within 1e-4 of a validity threshold, left out; history taken on "
          f"{(want['n_prev'] > 0).mean():.3f} of the region")
    assert n_near <= 1e-4 * w * h, n_near
    assert (want["n_prev"] > 0).mean() > 0.3
    g, x = got["radiance"][:hd, :wd][keep], want["radiance"][:hd, :wd][keep]
    bad = np.abs(g - x) > 1e-5 * np.abs(x) + 1e-7
    assert not bad.any(), f"{int(bad.any(axis=-1).sum())} pixels off by > 1e-5 relative, worst {np.abs(g - x).max():.3e}"
    for k in ("moments", "variance"):
        assert half_ulp_mismatch(got[k][:hd, :wd][keep], want[k][:hd, :wd][keep]) == 0.0, k
    assert np.array_equal(got["hlen"][:hd, :wd][keep], want["hlen"][:hd, :wd][keep])


def outputs(d):
    return dict(radiance=d.download(PLANE_RADIANCE), moments=d.download(PLANE_MOMENTS), variance=d.download(PLANE_VARIANCE),
                hlen=d.download(PLANE_HISTORY_LENGTH))


def seeded(w, h, seed):
    """test_reproject_gpu.seeded_history with textured radiance; the seed kernel turns the uploaded radiance[hist] into the history"""
    from test_reproject_gpu import seeded_history
    rad_prev, rad_cur, mom, hlen = seeded_history(w, h, seed)
    albedo = D.random_albedo(np.random.default_rng(seed), h, w)
    d = D.divisor(albedo)
    rad_prev[..., :3] *= d
    rad_cur[..., :3] *= d
    return rad_prev, rad_cur, mom, hlen, albedo, D.demodulate(rad_prev, d)


def test_reproject_arm():
    from test_reproject_gpu import CASES, _scene, render_gbuffers, reproject_context
    from test_reproject_cpu import moved
    name, W, H, cam_fn, move = CASES[0]
    cam_prev = cam_fn()
    cam_cur = moved(cam_prev, **move)
    gb_prev, gb_cur = render_gbuffers(_scene(name), W, H, [cam_prev, cam_cur])
    rad_prev, rad_cur, mom, hlen, albedo, demod_hist = seeded(W, H, 11)
    d = reproject_context(W, H, cam_prev, cam_cur, gb_prev, gb_cur, rad_prev, rad_cur, mom, hlen)
    d.set_option("svgf_demodulate", 1)
    d.upload(PLANE_ALBEDO, 0, albedo)
    d.submit_temporal_accumulation()
    got = outputs(d)
    d.destroy()
    want = D.reproject(R.reproject, R.Camera(cam_cur, W, H), R.Camera(cam_prev, W, H), rad_cur, demod_hist, albedo, gb_cur[0], gb_prev[0],
                       gb_cur[1], gb_prev[1], mom, hlen)
    check_reprojected(f"svgf_reproject {name} {W}x{H}", got, want, W, H)


def test_motion_arm():
    from motion_cases import BOXES, CORNELL_CASES, H, W, cameras, small_transform
    from test_motion_gpu import seed_planes, two_frames
    from test_refit_gpu import cornell_parts, moved_matrices
    kind, cam_move = next(c for c in CORNELL_CASES if c[1] is not None)
    cam_prev, cam_cur = cameras(cam_move)
    sc0 = cornell_parts()
    r, planes, mm = two_frames(sc0, BOXES, moved_matrices(sc0, BOXES, small_transform(kind)), cam_prev, cam_cur, W, H)
    rad_prev, rad_cur, mom, hlen, albedo, demod_hist = seeded(W, H, 41)
    r.svgf.set_option("svgf_demodulate", 1)
    r.svgf.upload(PLANE_ALBEDO, 0, albedo)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    got = outputs(r.svgf)
    r.destroy()
    (d0, n0, i0), (d1, n1, i1) = planes
    want = D.reproject(M.reproject, R.Camera(cam_cur, W, H), R.Camera(cam_prev, W, H), rad_cur, demod_hist, albedo, d1, d0, n1, n0, mom, hlen,
                       i1, i0, table=M.delta_table(mm[1], mm[0]))
    assert want["moved"].any()
    check_reprojected(f"svgf_motion cornell parts {kind}, camera {cam_move}", got, want, W, H)


def test_vertex_motion_arm():
    from test_deform_gpu import shaped, update
    from test_vertex_motion_gpu import seed_planes, two_frames
    from vertex_motion_cases import CASE_IDS, CASES, SCENES, cameras
    case = next(k for k, c in enumerate(CASES) if c[0] == "cornell" and c[1] is not None)
    name, cam_move = CASES[case]
    sc0, deform, _, w, h = SCENES[name]()
    cam_prev, cam_cur = cameras(name, cam_move)
    r, planes, plane, mm, _ = two_frames(sc0, lambda r: update(r, shaped(sc0, deform, "all")[0]), cam_prev, cam_cur, w, h)
    rad_prev, rad_cur, mom, hlen, albedo, demod_hist = seeded(w, h, 87)
    r.svgf.set_option("svgf_demodulate", 1)
    r.svgf.upload(PLANE_ALBEDO, 0, albedo)
    seed_planes(r.svgf, rad_prev, rad_cur, mom, hlen)
    r.svgf.submit_temporal_accumulation()
    got = outputs(r.svgf)
    r.destroy()
    (d0, n0, i0), (d1, n1, i1) = planes
    want = D.reproject(VM.reproject, R.Camera(cam_cur, w, h), R.Camera(cam_prev, w, h), rad_cur, demod_hist, albedo, d1, d0, n1, n0, mom, hlen,
                       i1, i0, plane, table=M.delta_table(mm[1], mm[0]))
    assert want["per_vertex"].sum() > 100
    check_reprojected(f"svgf_vertex_motion {CASE_IDS[case]}", got, want, w, h)


# ------------------------------------------------------------------------------------------------
# 4: seeding
# ------------------------------------------------------------------------------------------------
def test_seeding():
    """Whenever the demod plane does not hold the last denoised frame -- the option switched on mid-sequence, a reset_history, an upload
    into radiance[hist], a bracket without a denoise -- the next temporal pass equals the reference fed radiance[hist] / d as its
    history; and the seed kernel runs then and at no other time."""
    W, H, L = 96, 64, 3
    d = make(W, H, L, demod=False, svgf_profile=1)
    events = {2: "option on", 4: "reset_history", 6: "upload into radiance[hist]", 8: "no denoise", 9: "after a bracket without a denoise"}
    seeds, g_prev = 0, None
    for f in range(1, 11):
        g, rad, albedo = inputs(W, H, f, shift=5)
        feed(d, f, g, rad, albedo)
        what = events.get(f)
        if what == "option on":
            d.set_option("svgf_demodulate", 1)
        elif what == "reset_history":
            d.reset_history()
        elif what == "upload into radiance[hist]":
            d.upload(PLANE_RADIANCE, SLOT_HISTORY, inputs(W, H, 40)[1])
        elif what == "no denoise":
            d.end_frame()
            g_prev = g
            continue
        if what:
            hist = d.download(PLANE_RADIANCE, SLOT_HISTORY)
            ref = D.DemodSVGF(W, H, L)
            ref.begin_frame(f, g["depth"], g["normal"], rad, albedo, history=D.demodulate(hist, D.divisor(albedo)))
            o = ref.o
            o.depth[o.hist][...], o.normal[o.hist][...] = g_prev["depth"], g_prev["normal"]
            o.moments[o.hist][...] = d.download(PLANE_MOMENTS, SLOT_HISTORY)
            want = ref.temporal()
            ref.close()
            seeds += 1
        d.submit_temporal_accumulation()
        if what:
            check_temporal(f"frame {f}: {what}", d, want, rad, albedo)
            seeded_plane = d.download(PLANE_DEMOD, 0)[..., :3]
            assert np.array_equal(seeded_plane.view(np.uint32), D.demodulate(hist, D.divisor(albedo))[..., :3].view(np.uint32))
        d.submit_atrous_compute_wavelet()
        if f >= 2:
            assert d.level_times()[-1] == float(seeds), (f, d.level_times()[-1], seeds)
        d.end_frame()
        g_prev = g
    assert seeds == 4
    d.destroy()


# ------------------------------------------------------------------------------------------------
# 5: off means off; fused call order = separate call order
# ------------------------------------------------------------------------------------------------
def _denoise(d, f, W, H):
    g, rad, albedo = inputs(W, H, f)
    feed(d, f, g, rad, albedo)
    d.submit_temporal_accumulation()
    d.submit_atrous_compute_wavelet()
    d.end_frame()
    return [d.download(p) for p in (PLANE_RADIANCE, PLANE_MOMENTS, PLANE_VARIANCE)]


@pytest.mark.parametrize("fuse", [0, 1])
def test_off_means_off(fuse):
    """Option on for two frames, then off: the plane is gone, and from the same history planes (the two contexts' differ after two frames
    filtered differently, so the never-on context's are copied over) the following frames equal that context's bit for bit."""
    W, H, L = 136, 96, 4
    fresh, toggled = make(W, H, L, demod=False, svgf_fuse=fuse), make(W, H, L, demod=True, svgf_fuse=fuse)
    for f in (1, 2):
        _denoise(fresh, f, W, H)
        _denoise(toggled, f, W, H)
    toggled.set_option("svgf_demodulate", 0)
    with pytest.raises(_lib.NebError):
        toggled.get_plane(PLANE_DEMOD, 0)
    for plane in (PLANE_RADIANCE, PLANE_MOMENTS):
        for slot in (0, 1):
            toggled.upload(plane, slot, fresh.download(plane, slot))
    for f in (3, 4, 5):
        for x, y in zip(_denoise(fresh, f, W, H), _denoise(toggled, f, W, H)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f
    fresh.destroy()
    toggled.destroy()


def test_with_the_option_on_svgf_fuse_changes_nothing():
    W, H, L = 136, 96, 4
    a, b = make(W, H, L, svgf_fuse=1), make(W, H, L, svgf_fuse=0)
    for f in (1, 2, 3):
        for x, y in zip(_denoise(a, f, W, H), _denoise(b, f, W, H)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f
        assert np.array_equal(a.download(PLANE_DEMOD, 0)[..., :3].view(np.uint8), b.download(PLANE_DEMOD, 0)[..., :3].view(np.uint8))
    # neb_svgf_denoise is the same chain
    g, rad, albedo = inputs(W, H, 4)
    for d in (a, b):
        feed(d, 4, g, rad, albedo)
    a.submit_denoising()
    b.submit_temporal_accumulation()
    b.submit_atrous_compute_wavelet()
    assert np.array_equal(a.download(PLANE_RADIANCE).view(np.uint8), b.download(PLANE_RADIANCE).view(np.uint8))
    a.destroy()
    b.destroy()


# ------------------------------------------------------------------------------------------------
# 6: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals():
    W, H = 64, 48
    lib = _lib.load()
    strip = SVGFDenoiser()
    strip.init(W, H, row_begin=0, row_end=32)
    assert lib.neb_set_option(strip._ctx, b"svgf_demodulate", 1) == NEB_ERR_STATE
    assert b"row strips are not supported" in lib.neb_last_error(strip._ctx)
    strip.destroy()
    d = make(W, H, 2, demod=False, svgf_profile=1)
    ctx = d._ctx
    assert lib.neb_set_option(ctx, b"svgf_demodulate", 2) == NEB_ERR_INVALID_ARG
    assert lib.neb_set_option(ctx, b"svgf_demodulate", -1) == NEB_ERR_INVALID_ARG
    # with the option off, plane 14 answers exactly as an index no plane has
    ptr, size, rows = C.c_void_p(), C.c_size_t(), C.c_uint32()
    buf = np.zeros((H, W, 4), F)

    def answers(plane):
        out = []
        for call in (lambda: lib.neb_get_plane(ctx, plane, 0, C.byref(ptr), C.byref(size), C.byref(rows)),
                     lambda: lib.neb_upload_rows(ctx, plane, 0, 0, H, buf.ctypes.data_as(C.c_void_p), None),
                     lambda: lib.neb_download_rows(ctx, plane, 0, 0, H, buf.ctypes.data_as(C.c_void_p), None)):
            out.append((call(), lib.neb_last_error(ctx)))
        return out
    assert answers(PLANE_DEMOD) == answers(15) and all(rc == NEB_ERR_INVALID_ARG for rc, _ in answers(PLANE_DEMOD))
    d.set_option("svgf_demodulate", 1)
    assert lib.neb_get_plane(ctx, PLANE_DEMOD, 0, C.byref(ptr), C.byref(size), C.byref(rows)) == 0 and size.value == W * 16 and rows.value == H
    assert lib.neb_get_plane(ctx, PLANE_DEMOD, 1, C.byref(ptr), C.byref(size), C.byref(rows)) == NEB_ERR_INVALID_ARG  # one slot
    assert not d.download(PLANE_DEMOD, 0).any()  # allocated zeroed
    # a context without a-trous levels has no last level to multiply the albedo back
    none = SVGFDenoiser()
    none.init(W, H, atrous_levels=0)
    assert lib.neb_set_option(none._ctx, b"svgf_demodulate", 1) == NEB_ERR_STATE
    none.destroy()
    # resize: the plane is there again, zeroed, and the next frame seeds it
    _denoise(d, 1, W, H)
    _denoise(d, 2, W, H)
    assert d.download(PLANE_DEMOD, 0).any() and d.level_times()[-1] == 1.0
    W2, H2 = 80, 56
    d.resize(W2, H2)
    assert d.download(PLANE_DEMOD, 0).shape == (H2, W2, 4) and not d.download(PLANE_DEMOD, 0).any()
    _denoise(d, 3, W2, H2)
    assert d.level_times()[-1] == 2.0
    _denoise(d, 4, W2, H2)
    assert d.level_times()[-1] == 2.0
    d.destroy()


# ------------------------------------------------------------------------------------------------
# 7: what the user sees
# ------------------------------------------------------------------------------------------------
def _box5(img):
    p = np.pad(img, ((2, 2), (2, 2), (0, 0)), mode="edge")
    acc = np.zeros_like(img, dtype=np.float64)
    for dy in range(5):
        for dx in range(5):
            acc += p[dy:dy + img.shape[0], dx:dx + img.shape[1]]
    return acc / 25.0


def _metrics(img, ref, surf):
    """relative L2 over the surface pixels of the image, and of its high-pass part (image minus its 5 x 5 box mean)"""
    img, ref = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return rel_l2(img[surf], ref[surf]), rel_l2((img - _box5(img))[surf], (ref - _box5(ref))[surf])


def _converged(sc, cam, W, H):
    """the mean of 16 dispatches of 16-spp GI without SVGF at `cam` (test_what_the_user_sees_over_a_camera_pan's reference) -> image, surface mask"""
    conv = DeferredRenderer()
    conv.init(W, H)
    conv.gi_ui.gi_samples_per_pixel = 16
    acc = np.zeros((H, W, 4), np.float64)
    for k in range(16):
        conv.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1000 + k))
        conv.submit_commands_gbuffer()
        conv.submit_commands_pbr_lighting()
        conv.submit_commands_gi_pathtrace()
        acc += conv.svgf.download(PLANE_RADIANCE)
        conv.end_frame()
    surf = R.surface(conv.svgf.download(PLANE_DEPTH))
    conv.destroy()
    return acc / 16, surf


def _render(sc, cams, W, H, first_index, demod, reproject):
    """1 spp GI + SVGF through DeferredRenderer over the cameras given -> the denoised image of every frame SVGF ran on"""
    r = DeferredRenderer()
    r.temporal_reprojection = reproject
    r.albedo_demodulation = demod
    r.init(W, H)
    out = []
    for k, cam in enumerate(cams):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=first_index + k))
        r.submit_commands_gbuffer()
        r.submit_commands_pbr_lighting()
        r.submit_commands_gi_pathtrace()
        if r.submit_commands_svgf_denoising():
            out.append(r.svgf.download(PLANE_RADIANCE))
        r.end_frame()
    r.destroy()
    return out


@pytest.fixture(scope="module")
def user_scene():
    from test_reproject_gpu import _pan_camera
    W, H, N = 256, 256, 16
    sc = S.cornell_standin(textured=True)
    static_cam = _pan_camera(0)
    return dict(W=W, H=H, N=N, sc=sc, static_cam=static_cam, pan=[_pan_camera(f) for f in range(1, N + 1)],
                static_ref=_converged(sc, static_cam, W, H), pan_ref=_converged(sc, _pan_camera(N), W, H))


STARTS = [1, 101, 1001]


@pytest.mark.parametrize("start", STARTS)
def test_what_the_user_sees_with_a_static_camera_after_a_reset(user_scene, start):
    """cornell_standin(textured=True), 256 x 256, 1 spp GI + SVGF, DeferredRenderer's own policy: the first frame counts as moved (no
    SVGF), the second resets the history -- frames 1 - 4 after that reset, the two metrics averaged over the four, option on strictly
    below option off (= the behaviour without this option) in the same run.  Figures: DESIGN.md 3.7."""
    u = user_scene
    ref, surf = u["static_ref"]
    cams = [u["static_cam"]] * 5
    m = {}
    for demod in (False, True):
        frames = _render(u["sc"], cams, u["W"], u["H"], start, demod, reproject=False)
        assert len(frames) == 4
        m[demod] = np.mean([_metrics(img, ref, surf) for img in frames], axis=0)
    print(f"[static camera, frames 1-4 after a reset, frameIndex from {start}] relative L2 off {m[False][0]:.4f} on {m[True][0]:.4f}; "
          f"high-pass relative L2 off {m[False][1]:.4f} on {m[True][1]:.4f}")
    assert m[True][0] < m[False][0] and m[True][1] < m[False][1], (m[False], m[True])


@pytest.mark.parametrize("start", STARTS)
def test_what_the_user_sees_over_a_camera_pan(user_scene, start):
    """the 16-frame pan of test_reproject_gpu with temporal_reprojection, the last frame against the converged image at the final camera:
    both metrics, option on strictly below option off in the same run.  Figures: DESIGN.md 3.7."""
    u = user_scene
    ref, surf = u["pan_ref"]
    m = {}
    for demod in (False, True):
        frames = _render(u["sc"], u["pan"], u["W"], u["H"], start, demod, reproject=True)
        assert len(frames) == u["N"]
        m[demod] = _metrics(frames[-1], ref, surf)
    print(f"[16-frame pan with temporal_reprojection, frameIndex from {start}] relative L2 off {m[False][0]:.4f} on {m[True][0]:.4f}; "
          f"high-pass relative L2 off {m[False][1]:.4f} on {m[True][1]:.4f}")
    assert m[True][0] < m[False][0] and m[True][1] < m[False][1], (m[False], m[True])
