"""CPU tests of option svgf_motion (reprojection that follows moved submeshes): the C ABI declares and exports it,
the delta table of the CPU reference (tests/motion_ref.py) behaves as promised, and the reference alone -- on the CPU oracle's
G-buffers of the cornell parts, ids from a float64 ray caster -- satisfies what tests/test_motion_gpu.py asks of the device for
the same scenes, cameras and moves, including the share of pixels it excludes as too close to a threshold.
(The 1080p sponza stand-in case has no CPU pre-check: its ids need the device's G-buffer producer.)"""
import ctypes as C
import os

import numpy as np
import pytest

import motion_ref as M
import reproject_ref as R
from motion_cases import BOXES, CORNELL_CASES, H, W, cameras, small_transform
from nebulae_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEAR_CAP = 5e-4


def _parts():
    from test_refit_gpu import cornell_parts, moved_matrices, with_matrices, world_transform
    return cornell_parts, moved_matrices, with_matrices, world_transform


def test_option_plane_and_snapshot_are_declared_and_exported():
    from test_abi import declared_symbols
    assert "neb_svgf_snapshot_transforms" in declared_symbols()
    assert "neb_svgf_snapshot_transforms" in _lib.exported_symbols()
    build.build()
    assert hasattr(C.CDLL(build.LIB_PATH), "neb_svgf_snapshot_transforms")
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    assert "#define NEB_PLANE_SUBMESH_ID 12" in text and "NEB_PLANE_COUNT = 12" in text
    assert '"svgf_motion"' in text
    from nebulae_amd.svgf import PLANE_LAYOUT, PLANE_SUBMESH_ID
    assert PLANE_SUBMESH_ID == 12 and PLANE_LAYOUT[PLANE_SUBMESH_ID] == (np.uint32, 1)
    assert (M.ENTRY_FLOAT4, M.SAME, M.MOVED, M.SINGULAR) == (8, 0, 1, 2)


def test_snapshot_validates_arguments_without_a_gpu():
    assert _lib.load().neb_svgf_snapshot_transforms(None, 0, None) == -1


def test_delta_of_equal_matrices_is_flag_0_and_of_a_singular_one_flag_2():
    cornell_parts, moved_matrices, _, world_transform = _parts()
    sc = cornell_parts(textured=False)
    m = np.stack([g["M"] for g in sc.geometries])
    t = M.delta_table(m, m.copy())
    assert (t["flag"] == M.SAME).all()
    assert (t["D"][:, :3] == np.eye(3, dtype=F)).all() and (t["D"][:, 3] == 0).all() and (t["K"] == np.eye(3, dtype=F)).all()
    flat, nan, inf = m.copy(), m.copy(), m.copy()
    flat[1, :3, 1] = 0.0          # a box squashed to a plane
    flat[2, 0, :3] = flat[2, 1, :3]  # two equal rows
    nan[1, 2, 2] = nan[2, 3, 1] = np.nan
    inf[1, 0, 0] = inf[2, 3, 0] = np.inf
    for bad in (flat, nan, inf):
        for a, b in ((bad, m), (m, bad)):  # singular on either side
            t = M.delta_table(a, b)
            assert (t["flag"][[1, 2]] == M.SINGULAR).all() and (t["flag"][[0, 3, 4]] == M.SAME).all(), t["flag"]
            assert not t["D"][[1, 2]].any() and not t["K"][[1, 2]].any()
    # -0.0 against +0.0 is "moved" (bit for bit), with an identity result
    neg = m.copy()
    neg[0][neg[0] == 0] = F(-0.0)
    t = M.delta_table(neg, m)
    assert t["flag"][0] == M.MOVED and np.allclose(t["D"][0, :3], np.eye(3), atol=1e-6)


@pytest.mark.parametrize("kind", ["translate", "rotate", "scale"])
def test_delta_carries_baked_points_back_to_the_previous_bake(kind):
    """D applied to the world points of a moved box (baked in float32 as the library bakes them) gives the points baked under the
    previous matrix to fp32 rounding; K carries the baked normals back the same way."""
    cornell_parts, moved_matrices, _, world_transform = _parts()
    sc = cornell_parts(textured=False)
    m_hist = np.stack([sc.geometries[i]["M"] for i in BOXES])
    m_cur = moved_matrices(sc, BOXES, world_transform(kind))
    t = M.delta_table(m_cur, m_hist)
    assert (t["flag"] == M.MOVED).all()
    for k, gi in enumerate(BOXES):
        P = sc.geometries[gi]["positions"].astype(F)
        bake = lambda m: (P @ m[:3, :3] + m[3, :3]).astype(F)  # noqa: E731
        w_cur, w_hist = bake(m_cur[k]), bake(m_hist[k])
        back = w_cur.astype(np.float64) @ t["D"][k, :3].astype(np.float64) + t["D"][k, 3]
        scale = np.abs(w_hist).max()
        assert np.abs(back - w_hist).max() <= 8 * np.finfo(F).eps * scale, np.abs(back - w_hist).max()
        N = sc.geometries[gi]["normals"].astype(np.float64)
        inv_t = lambda m: np.linalg.inv(m[:3, :3].astype(np.float64)).T  # noqa: E731
        n_cur, n_hist = N @ inv_t(m_cur[k]), N @ inv_t(m_hist[k])
        n_back = n_cur @ t["K"][k].astype(np.float64)
        unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
        assert np.abs(unit(n_back) - unit(n_hist)).max() <= 1e-5


# ---- the reference on oracle G-buffers ----
_CACHE = {}


def oracle_frames(kind, cam_move, T=None):
    """two frames of the cornell parts: boxes 1 and 2 moved by `T` (default: the small transform of `kind`) between them
    -> dict(cams, gb (oracle G-buffers), ids, mats (hist, cur), scenes)"""
    key = (kind, str(cam_move), None if T is None else T.tobytes())
    if key not in _CACHE:
        from oracle_lib import OracleTracer
        cornell_parts, moved_matrices, with_matrices, _ = _parts()
        sc0 = cornell_parts(textured=False)
        mats = moved_matrices(sc0, BOXES, small_transform(kind) if T is None else T)
        sc1 = with_matrices(sc0, BOXES, mats)
        cam_prev, cam_cur = cameras(cam_move)
        gb = [OracleTracer(sc0).gbuffer(W, H, cam_prev), OracleTracer(sc1).gbuffer(W, H, cam_cur)]
        ids = []
        for sc, cam, g in ((sc0, cam_prev, gb[0]), (sc1, cam_cur, gb[1])):
            i, _ = M.primary_ids(sc, cam, W, H)
            i[~R.surface(g["depth"])] = M.NO_SUBMESH
            ids.append(i)
        m_hist, m_cur = [np.stack([g["M"] for g in s.geometries]) for s in (sc0, sc1)]
        _CACHE[key] = dict(cams=(cam_prev, cam_cur), gb=gb, ids=ids, mats=(m_hist, m_cur), scenes=(sc0, sc1))
    return _CACHE[key]


def seeded(seed):
    rng = np.random.default_rng(seed)
    rad_prev = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    rad_cur = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    mom = np.stack([rng.uniform(0.05, 2.0, (H, W)), rng.uniform(0.05, 4.0, (H, W))], axis=-1).astype(np.float16)
    hlen = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return rad_prev, rad_cur, mom, hlen


def run_reference(fr, rad_prev, rad_cur, mom, hlen, motion=True, **kw):
    cam_prev, cam_cur = fr["cams"]
    args = (R.Camera(cam_cur, W, H), R.Camera(cam_prev, W, H), rad_cur, rad_prev, fr["gb"][1]["depth"], fr["gb"][0]["depth"],
            fr["gb"][1]["normal"], fr["gb"][0]["normal"], mom, hlen)
    if not motion:
        return R.reproject(*args, **kw)
    return M.reproject(*args, fr["ids"][1], fr["ids"][0], table=M.delta_table(fr["mats"][1], fr["mats"][0]), **kw)


@pytest.mark.parametrize("case", range(len(CORNELL_CASES)), ids=lambda k: f"{CORNELL_CASES[k][0]}-{'pan' if CORNELL_CASES[k][1] else 'static'}")
def test_near_share_of_the_gpu_cases_stays_under_the_cap(case):
    """the pixels the GPU parity test will exclude (within 1e-4 of a validity threshold, or a moved pixel's tap position within
    1e-4 of an integer), on the oracle's G-buffers of the same case: at most 5e-4 of the image; and the moved boxes keep history"""
    kind, cam_move = CORNELL_CASES[case]
    fr = oracle_frames(kind, cam_move)
    out = run_reference(fr, *seeded(31 + case))
    on_box = np.isin(fr["ids"][1], BOXES)
    took = out["n_prev"] > 0
    share = out["near"].sum() / (W * H)
    print(f"[{kind}, camera {cam_move}] near share {share:.2e}; moved pixels {int(out['moved'].sum())}, history taken on "
          f"{took[on_box].mean():.3f} of the boxes' pixels")
    assert share <= NEAR_CAP, share
    assert out["moved"][on_box].all() and not out["moved"][~on_box].any()
    assert took[on_box].mean() >= 0.5


# Moves of a few pixels: small enough that plain reprojection's normal and plane tests still pass on the boxes, so that it DOES take the
# history -- of the wrong surface point.  (A large step fails those tests instead: the box then takes no history at all and returns the
# current frame exactly, which is the other half of the defect and shows as lost history, not as a wrong value.)
PAINT_MOVES = ["translate", "rotate", "scale"]


@pytest.mark.parametrize("kind", PAINT_MOVES)
def test_painted_object_follows_its_box_and_plain_reprojection_does_not(kind):
    """radiance[hist] = f(object-space point each pixel of the moved boxes saw in the previous frame), radiance[cur] = f at this frame's
    points (f of the world point elsewhere); alpha = 1, n = 255: wherever a box pixel has four valid taps the motion reference returns f
    at the current points to <= 1e-3 relative, and the reference without motion (svgf_motion = 0) misses by >= 20 x that in the mean."""
    fr = oracle_frames(kind, None)
    f_prev, f_cur = painted(fr, 0), painted(fr, 1)
    mom = np.zeros((H, W, 2), np.float16)
    hlen = np.full((H, W), 255, np.uint8)
    out = run_reference(fr, f_prev, f_cur, mom, hlen, alpha=1.0)
    plain = run_reference(fr, f_prev, f_cur, mom, hlen, motion=False, alpha=1.0)
    on_box = np.isin(fr["ids"][1], BOXES)
    all4 = out["valid"].all(axis=0) & on_box
    assert all4.sum() >= 0.5 * on_box.sum(), all4.sum() / on_box.sum()
    want = f_cur[all4][:, :3].astype(np.float64)
    rel = np.abs(out["radiance"][all4][:, :3] - want) / want
    rel_plain = np.abs(plain["radiance"][all4][:, :3] - want) / want
    print(f"[painted object, {kind}] four valid taps on {all4.sum() / on_box.sum():.3f} of the boxes' pixels; motion max rel error {rel.max():.2e} "
          f"(mean {rel.mean():.2e}); without motion max {rel_plain.max():.2e} (mean {rel_plain.mean():.2e})")
    assert rel.max() <= 1e-3, rel.max()
    assert rel_plain.mean() >= 20 * rel.mean()


def painted(fr, which):
    """f of the object-space point on the moved boxes, of the world point elsewhere (frame `which`: 0 = hist, 1 = cur)"""
    Pw = R.world_points64(fr["cams"][which], fr["gb"][which]["depth"])
    P = Pw.copy()
    for gi in BOXES:
        sel = fr["ids"][which] == gi
        P[sel] = M.object_points64(Pw, fr["ids"][which], gi, fr["mats"][which][gi])[sel]
    return R.paint(P)


def test_id_test_keeps_an_uncovered_wall_from_the_object_that_left():
    """the tall box slides sideways in front of the back wall: wall pixels it uncovered, whose taps in the history frame all show the box,
    take no history -- also where the box's face and the wall are parallel and close enough for the plane test alone to pass"""
    T = np.eye(4)
    T[3, :3] = (-0.12, 0.0, 0.0)
    fr = oracle_frames("slide", None, T=T)
    rad_prev, rad_cur, mom, hlen = seeded(5)
    hlen[:] = 30
    out = run_reference(fr, rad_prev, rad_cur, mom, hlen)
    fx, fy = out["q"]
    uncovered = np.zeros((H, W), bool)
    cand = (~np.isin(fr["ids"][1], BOXES)) & R.surface(fr["gb"][1]["depth"]) & np.isfinite(fx) & (fx > 0) & (fx < W - 1) & (fy > 0) & (fy < H - 1)
    ys, xs = np.nonzero(cand)
    x0, y0 = np.floor(fx[ys, xs]).astype(int), np.floor(fy[ys, xs]).astype(int)
    all_box = np.ones(len(ys), bool)
    for t in range(4):
        all_box &= np.isin(fr["ids"][0][y0 + (t >> 1), x0 + (t & 1)], BOXES)
    uncovered[ys[all_box], xs[all_box]] = True
    assert uncovered.sum() >= 10, uncovered.sum()
    assert (out["n_prev"][uncovered] == 0).all() and (out["hlen"][uncovered] == 1).all()
    assert np.array_equal(out["radiance"][uncovered], rad_cur[uncovered])


def test_static_scene_differs_from_plain_reprojection_only_where_ids_differ_among_the_taps():
    fr = oracle_frames("translate", dict(pan=(0.04, 0.0, 0.0), yaw_deg=-0.4), T=np.eye(4))
    assert np.array_equal(fr["mats"][0], fr["mats"][1])
    planes = seeded(9)
    out, plain = run_reference(fr, *planes), run_reference(fr, *planes, motion=False)
    assert not out["moved"].any() and not out["frozen"].any()
    same = np.ones((H, W), bool)
    for k in ("radiance", "moments", "variance", "hlen"):
        a, b = out[k].view(np.uint8).reshape(H, W, -1), plain[k].view(np.uint8).reshape(H, W, -1)
        same &= (a == b).all(axis=-1)
    print(f"[static scene] {int((~same).sum())} pixels differ from plain reprojection; ids differ among the taps of {int((~out['tap_ids_equal']).sum())}")
    assert same[out["tap_ids_equal"]].all()
