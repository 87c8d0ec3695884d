"""Option svgf_vertex_motion on the CPU: the float64 reference of the previous-point plane agrees with the
per-submesh rule where a "deformation" is rigid, and the two conditions the GPU tests rely on hold on reference-made G-buffers for the
very cases they run -- few pixels near a threshold, and history kept on the deformed submesh."""
import numpy as np
import pytest

import motion_ref as M
import reproject_ref as R
import vertex_motion_ref as VM
from motion_cases import small_transform
from vertex_motion_cases import CASE_IDS, CASES, SCENES, SHORT_BOX, cameras, matrices

F = np.float32
NEAR_CAP = 1e-3   # of the compared pixels: within 1e-4 of a validity threshold, or a tap position within 1e-4 of an integer
KEPT_FLOOR = 0.9  # of the deformed submesh's pixels take history in the reference (94.8 - 100 % for rigid moves of this size)


def test_plane_option_and_entry_point_are_declared_and_exported():
    import os
    import re
    from nebulae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nebulae_hip.h")).read()
    assert re.search(r"#define\s+NEB_PLANE_PREV_POINT\s+13\b", header)
    assert _lib.PLANE_PREV_POINT == 13
    assert "neb_svgf_snapshot_vertices" in header and "neb_svgf_snapshot_vertices" in _lib.exported_symbols()
    assert '"svgf_vertex_motion"' in header
    assert VM.NO_PREV_POINT == 0xFFFFFFFF


@pytest.mark.parametrize("kind", ["translate", "rotate", "scale"])
def test_a_rigid_deformation_gives_the_points_of_the_delta_table(kind):
    """The short box "deformed" by a rigid motion T (translate, 2 degrees, 3 %), handed over as new vertices in float64: object-space
    vertices p' = p . (M T M^-1).  The same frame pair described per submesh is M_cur = M . T with the old vertices.  The plane's
    points (vertex route, float64) equal motion_ref.map_point_normal through delta_table (fp32 kernel arithmetic) to 1e-6 relative."""
    from test_deform_gpu import with_arrays
    from test_refit_gpu import cornell_camera, cornell_parts, moved_matrices, with_matrices
    from motion_cases import H, W
    sc0 = cornell_parts(textured=False)
    cam = cornell_camera()
    T = small_transform(kind)
    g = sc0.geometries[SHORT_BOX]
    M0 = g["M"].astype(np.float64)
    Tobj = M0 @ T @ np.linalg.inv(M0)
    P1 = g["positions"].astype(np.float64) @ Tobj[:3, :3] + Tobj[3, :3]
    N1 = g["normals"].astype(np.float64) @ np.linalg.inv(Tobj[:3, :3]).T
    sc1 = with_arrays(sc0, {})
    sc1.geometries[SHORT_BOX].update(positions=P1, normals=N1 / np.linalg.norm(N1, axis=1, keepdims=True))  # (kept in float64)
    ref = VM.prev_point_plane(sc0, sc1, matrices(sc0), cam, W, H, dirty=[SHORT_BOX])
    on = ref["flagged"]
    assert on.sum() > 1000 and np.array_equal(on, ref["covered"] & (ref["geometry"] == SHORT_BOX))
    # the per-submesh description of the same pair of frames, fed the current world points of the same hits
    m_cur = moved_matrices(sc0, [SHORT_BOX], T)
    table = M.delta_table(matrices(with_matrices(sc0, [SHORT_BOX], m_cur)), matrices(sc0))
    c = R.Camera(cam, W, H)
    hit = VM.V.primary(sc1, cam, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xa, ya, za, eye = [np.asarray(v, np.float64) for v in (c.x, c.y, c.z, c.eye)]
    d = xa * (((xs + 0.5) / W * 2.0 - 1.0) * float(c.sx))[..., None] + ya * ((1.0 - (ys + 0.5) / H * 2.0) * float(c.sy))[..., None] - za
    d /= np.sqrt(np.sum(d * d, -1, keepdims=True))
    Pw = eye + d * np.where(on, hit["t"], 0.0)[..., None]
    # current geometric normal of the hits: the current vertex normals interpolated as prev_point_plane interpolates the previous ones
    cur_as_prev = VM.prev_point_plane(sc1, sc1, matrices(sc1), cam, W, H, dirty=[SHORT_BOX])
    Ncur = np.where(on[..., None], cur_as_prev["N"], 0.0).astype(F)
    assert np.abs(cur_as_prev["P"][on] - Pw[on]).max() <= 1e-9  # (interpolating the current vertices gives the hit point itself)
    P_h, N_h, moved, frozen = M.map_point_normal(tuple(Pw[..., k].astype(F) for k in range(3)), Ncur, hit["geometry"], table)
    assert moved[on].all() and not frozen.any()
    got = np.stack(P_h, -1).astype(np.float64)[on]
    rel = np.linalg.norm(got - ref["P"][on], axis=-1) / np.linalg.norm(ref["P"][on], axis=-1)
    cosn = np.sum(N_h[on].astype(np.float64) * ref["N"][on], -1)
    print(f"[rigid {kind}] {int(on.sum())} px; worst relative distance between the two routes {rel.max():.2e}; worst normal angle "
          f"{np.degrees(np.arccos(np.clip(cosn.min(), -1, 1))):.2e} degrees")
    assert rel.max() <= 1e-6, rel.max()
    assert cosn.min() >= 1.0 - 1e-6


_CACHE = {}


def reference_frames(name, cam_move):
    """two frames of a case on the CPU oracle's G-buffers, ids from the float64 caster, the plane from prev_point_plane"""
    key = (name, str(cam_move))
    if key not in _CACHE:
        from oracle_lib import OracleTracer
        sc0, deform, sc1, w, h = SCENES[name]()
        cam_prev, cam_cur = cameras(name, cam_move)
        gb = [OracleTracer(sc0).gbuffer(w, h, cam_prev), OracleTracer(sc1).gbuffer(w, h, cam_cur)]
        ids = []
        for sc, cam, g in ((sc0, cam_prev, gb[0]), (sc1, cam_cur, gb[1])):
            i = VM.V.primary(sc, cam, w, h)["geometry"].copy()
            i[~R.surface(g["depth"])] = M.NO_SUBMESH
            ids.append(i)
        ref = VM.prev_point_plane(sc0, sc1, matrices(sc0), cam_cur, w, h, dirty=list(deform))
        ref["flagged"] &= R.surface(gb[1]["depth"])
        _CACHE[key] = dict(cams=(cam_prev, cam_cur), gb=gb, ids=ids, plane=VM.pack_plane(ref), ref=ref, size=(w, h), deformed=list(deform))
    return _CACHE[key]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda k: CASE_IDS[k])
def test_the_conditions_of_the_gpu_tests_hold_on_reference_made_gbuffers(case):
    name, cam_move = CASES[case]
    fr = reference_frames(name, cam_move)
    w, h = fr["size"]
    rng = np.random.default_rng(61 + case)
    rad_prev, rad_cur = (rng.uniform(0.0, 2.0, (h, w, 4)).astype(F) for _ in range(2))
    mom = np.stack([rng.uniform(0.05, 2.0, (h, w)), rng.uniform(0.05, 4.0, (h, w))], axis=-1).astype(np.float16)
    hlen = rng.integers(1, 256, (h, w)).astype(np.uint8)
    cam_prev, cam_cur = fr["cams"]
    out = VM.reproject(R.Camera(cam_cur, w, h), R.Camera(cam_prev, w, h), rad_cur, rad_prev, fr["gb"][1]["depth"], fr["gb"][0]["depth"],
                       fr["gb"][1]["normal"], fr["gb"][0]["normal"], mom, hlen, fr["ids"][1], fr["ids"][0], fr["plane"], table=None)
    hd, wd = h // 8 * 8, w // 8 * 8
    on = np.isin(fr["ids"][1], fr["deformed"])[:hd, :wd]
    took = out["n_prev"] > 0
    share = out["near"].sum() / (hd * wd)
    print(f"[{CASE_IDS[case]}] deformed submesh covers {int(on.sum())} px, per-vertex motion on {int(out['per_vertex'].sum())}; near share "
          f"{share:.2e} ({int(out['near'].sum())} px); history taken on {took[on].mean():.3f} of the submesh's pixels")
    assert on.sum() > 100 and np.array_equal(out["per_vertex"], on)
    assert share < NEAR_CAP, share
    assert took[on].mean() >= KEPT_FLOOR, took[on].mean()
