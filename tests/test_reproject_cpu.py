"""CPU tests of temporal reprojection (option svgf_reproject): the C ABI declares and exports it, and the CPU reference
(tests/reproject_ref.py) behaves as the mode promises on oracle G-buffers of the cornell box (tests/golden/cornell_box.glb)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import reproject_ref as R
from nebulae_amd import _lib, build
from nebulae_amd import scene as S
from oracle import svgf_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H = 96, 64


def test_set_camera_and_history_plane_are_declared_and_exported():
    from test_abi import declared_symbols
    assert "neb_svgf_set_camera" in declared_symbols()
    assert "neb_svgf_set_camera" in _lib.exported_symbols()
    build.build()
    assert hasattr(C.CDLL(build.LIB_PATH), "neb_svgf_set_camera")
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    assert "NEB_PLANE_HISTORY_LENGTH = 11" in text and "NEB_PLANE_COUNT = 12" in text
    from nebulae_amd.svgf import PLANE_HISTORY_LENGTH, PLANE_LAYOUT
    assert PLANE_HISTORY_LENGTH == 11 and PLANE_LAYOUT[PLANE_HISTORY_LENGTH] == (np.uint8, 1)


def test_set_camera_validates_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.neb_svgf_set_camera(None, 0, None) == -1


def test_constants_come_from_the_one_header():
    assert R.NORMAL_COS == np.float32(0.9) and R.PLANE_TOL == np.float32(0.01)
    hits = []
    for d, _, files in os.walk(os.path.join(ROOT, "nebulae_amd")):
        for f in files:
            if f.endswith((".hip", ".h", ".py")) and f != "svgf_reproject.h":
                text = open(os.path.join(d, f)).read()
                hits += [f for name in ("kReprojNormalCos =", "kReprojPlaneTol =") if name in text]
    assert not hits, hits


_SCENE = []


def _tracer():
    from oracle_lib import OracleTracer
    if not _SCENE:
        sc = S.load_gltf(os.path.join(GOLDEN, "cornell_box.glb"))
        _SCENE.append((sc, OracleTracer(sc)))
    return _SCENE[0][1]


def base_camera():
    return S.orbit_camera(origin=(0.0, 1.0, 0.0), distance=3.5)  # the file's own camera node


def moved(cam, pan=(0.0, 0.0, 0.0), yaw_deg=0.0):
    """the camera translated by `pan` (eye and target) and turned by yaw_deg about the world up axis through the eye"""
    eye = np.array(list(cam.eye), np.float64) + pan
    fwd = np.array(list(cam.target), np.float64) - np.array(list(cam.eye), np.float64)
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    fwd = np.array([c * fwd[0] + s * fwd[2], fwd[1], -s * fwd[0] + c * fwd[2]])
    out = S.CameraDesc()
    out.eye[:] = [float(v) for v in eye]
    out.target[:] = [float(v) for v in eye + fwd]
    out.up[:] = list(cam.up)
    out.vfov_deg, out.znear, out.zfar = cam.vfov_deg, cam.znear, cam.zfar
    return out


# pans of ~1.5 .. 6 px at the back wall (one pixel is ~0.063 world units there) and turns of ~1 .. 5 px
MOVES = [dict(pan=(0.1, 0.0, 0.0)), dict(pan=(-0.25, 0.1, 0.0)), dict(pan=(0.0, 0.0, -0.3)), dict(yaw_deg=1.0), dict(yaw_deg=-4.0),
         dict(pan=(0.2, 0.0, 0.1), yaw_deg=2.5)]


def _run(cam_prev, cam_cur, gb_prev, gb_cur, rad_prev, rad_cur, hlen, alpha=0.9, seed=3):
    rng = np.random.default_rng(seed)
    mom = rng.uniform(0.1, 2.0, (H, W, 2)).astype(np.float16)
    out = R.reproject(R.Camera(cam_cur, W, H), R.Camera(cam_prev, W, H), rad_cur, rad_prev, gb_cur["depth"], gb_prev["depth"],
                      gb_cur["normal"], gb_prev["normal"], mom, hlen, alpha=alpha)
    return out, mom


def test_identity_camera_maps_every_pixel_to_its_own_centre():
    o = _tracer()
    cam = base_camera()
    gb = o.gbuffer(W, H, cam)
    rng = np.random.default_rng(1)
    rad = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    hlen = np.full((H, W), 7, np.uint8)
    out, _ = _run(cam, cam, gb, gb, rad, rad.copy(), hlen)
    surf = R.surface(gb["depth"])
    fx, fy = out["q"]
    ys, xs = np.nonzero(surf)
    assert len(ys) > 0.25 * W * H
    assert float(np.abs(fx[ys, xs] - xs).max()) <= 1e-3 and float(np.abs(fy[ys, xs] - ys).max()) <= 1e-3
    # the pixel's own tap is valid and carries (almost) all the weight; away from silhouettes and creases all four taps are valid
    x0, y0 = np.floor(fx[ys, xs]).astype(int), np.floor(fy[ys, xs]).astype(int)
    own = (xs - x0) + 2 * (ys - y0)
    assert out["valid"][own, ys, xs].all()
    assert float(out["weights"][own, ys, xs].min()) >= 0.999
    all4 = out["valid"][:, ys, xs].all(axis=0)
    assert all4.mean() >= 0.75, all4.mean()  # (at 96 x 64 a fifth of the box's pixels touch an edge)
    assert (out["n_prev"][ys, xs] == 7).all() and (out["hlen"][ys, xs] == 8).all()
    # history = current: the blend returns the frame (to rounding)
    np.testing.assert_allclose(out["radiance"][ys, xs, :3], rad[ys, xs, :3], rtol=1e-4, atol=1e-4)
    # no surface: no history
    assert (out["n_prev"][~surf] == 0).all() and (out["radiance"][~surf] == rad[~surf]).all()


@pytest.mark.parametrize("move", range(len(MOVES)))
def test_painted_world_is_reprojected_and_same_pixel_history_is_not(move):
    """radiance[hist] = f(world point each pixel saw in the previous frame), radiance[cur] = f(this frame's): with n = 255 and
    alpha = 1 the output is f at the current pixels' world points to <= 1e-3 relative wherever four taps are valid, while the
    same-pixel pass (svgf_np.temporal) misses by far more on the same input."""
    o = _tracer()
    cam_prev = base_camera()
    cam_cur = moved(cam_prev, **MOVES[move])
    gb_prev, gb_cur = o.gbuffer(W, H, cam_prev), o.gbuffer(W, H, cam_cur)
    f_prev = R.paint(R.world_points64(cam_prev, gb_prev["depth"]))
    f_cur = R.paint(R.world_points64(cam_cur, gb_cur["depth"]))
    hlen = np.full((H, W), 255, np.uint8)
    out, mom = _run(cam_prev, cam_cur, gb_prev, gb_cur, f_prev, f_cur.copy(), hlen, alpha=1.0)
    surf = R.surface(gb_cur["depth"])
    all4 = out["valid"].all(axis=0) & surf
    assert all4.sum() >= 0.5 * surf.sum(), all4.sum() / surf.sum()
    got = out["radiance"][all4][:, :3].astype(np.float64)
    want = f_cur[all4][:, :3].astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    # same-pixel pass, alpha = 1: keeps the history of the same pixel wherever depth and normals agree (quirk 2 elsewhere)
    p = dict(svgf_np.DEFAULT_PARAMS, alpha=np.float32(1.0))
    same, _, _ = svgf_np.temporal(f_cur, f_prev, gb_cur["depth"], gb_prev["depth"], gb_cur["normal"], gb_prev["normal"], mom, p=p)
    rel_same = np.abs(same[all4][:, :3].astype(np.float64) - want) / np.abs(want)
    print(f"move {MOVES[move]}: four valid taps on {all4.sum() / surf.sum():.3f} of the surface pixels; reprojected max rel error {rel.max():.2e}, "
          f"same-pixel max {rel_same.max():.2e} (mean {rel.mean():.2e} against {rel_same.mean():.2e})")
    assert rel.max() <= 1e-3, rel.max()
    assert rel_same.mean() >= 20 * rel.mean() and rel_same.max() >= 20 * rel.max()


def test_disocclusion_takes_no_history():
    """A pan that uncovers the wall behind the tall block: where the previous frame saw the block in front of the point, the
    pixel takes no history (n = 0), its output is the current value exactly and its history length restarts at 1."""
    o = _tracer()
    cam_prev = base_camera()
    cam_cur = moved(cam_prev, pan=(0.35, 0.0, 0.0))
    gb_prev, gb_cur = o.gbuffer(W, H, cam_prev), o.gbuffer(W, H, cam_cur)
    rng = np.random.default_rng(5)
    rad_prev = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    rad_cur = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    hlen = np.full((H, W), 30, np.uint8)
    out, _ = _run(cam_prev, cam_cur, gb_prev, gb_cur, rad_prev, rad_cur, hlen)
    # occluded in the previous frame (float64): every in-image tap of the point's previous position saw a surface nearer by > 10 %
    P = R.world_points64(cam_cur, gb_cur["depth"])
    Pp = R.world_points64(cam_prev, gb_prev["depth"])
    c = R.Camera(cam_prev, W, H)
    ez, eye = np.asarray(c.z, np.float64), np.asarray(c.eye, np.float64)
    zl = -((P - eye) @ ez)
    zprev = -((Pp - eye) @ ez)
    fx, fy = out["q"]
    occluded = np.zeros((H, W), bool)
    inside = np.isfinite(fx) & (fx > 0) & (fx < W - 1) & (fy > 0) & (fy < H - 1) & R.surface(gb_cur["depth"])
    ys, xs = np.nonzero(inside)
    x0, y0 = np.floor(fx[ys, xs]).astype(int), np.floor(fy[ys, xs]).astype(int)
    occ = np.ones(len(ys), bool)
    for t in range(4):
        tz = zprev[y0 + (t >> 1), x0 + (t & 1)]
        occ &= np.isfinite(tz) & (tz < 0.9 * zl[ys, xs])
    occluded[ys[occ], xs[occ]] = True
    assert occluded.sum() >= 10, occluded.sum()
    assert (out["n_prev"][occluded] == 0).all()
    assert np.array_equal(out["radiance"][occluded], rad_cur[occluded])
    assert (out["hlen"][occluded] == 1).all()
    # and elsewhere history is taken
    assert (out["n_prev"][R.surface(gb_cur["depth"])] == 30).mean() > 0.8
