"""A brute-force ray caster over a scene's world-space triangles, and the scenes, updates and cameras of tests/test_update_views_gpu.py.
TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`cast` generalises motion_ref.primary_ids: Moller-Trumbore against every triangle, no acceleration structure, any rays, in chunks
of rays x triangles so that memory stays bounded, in the floating-point type asked for.  float64 is the reference.  The float32
run of the same code exists to show, on the CPU, how many pixels two correct casters disagree at for a given camera -- rays that
pass an edge or a corner within rounding: tests/test_views_ref_cpu.py holds every (scene state, camera) pair of the GPU tests to
TIE_CAP // 2 such pixels, which is what lets those tests cap the device's disagreement with float64 at TIE_CAP.

Importing the GPU test modules for their scene helpers touches no device: the CPU test runs without a GPU.
"""
import math

import numpy as np

import reproject_ref as R
from motion_ref import NO_SUBMESH, scene_triangles
from nebulae_amd import scene as S
from test_deform_gpu import sine_along_normal, with_arrays
from test_refit_gpu import TIE_CAP, cornell_camera, cornell_parts, moved_matrices, with_matrices, world_transform  # noqa: F401

F = np.float32
VW, VH = 64, 48        # the swept views
FAR = 1000.0           # far plane of the views that look at objects carried out of the room (the orbit camera's is 100)
N_CELLS = 24           # the floor patch


# ------------------------------------------------------------------------------------------------
# the caster
# ------------------------------------------------------------------------------------------------
def triangles(sc):
    """motion_ref.scene_triangles plus the primitive index of each triangle within its geometry -> (v0, e1, e2, geometry, primitive)"""
    v0, e1, e2, gi = scene_triangles(sc)
    prim = np.concatenate([np.arange(len(g["indices"]) // 3, dtype=np.uint32) for g in sc.geometries])
    return v0, e1, e2, gi, prim


def cast(tris, o, d, tmin=0.0, tmax=np.inf, dtype=np.float64, ray_chunk=256, tri_chunk=4096):
    """tris: triangles(sc); o [n, 3] or [3], d [n, 3]: rays.  The closest hit with tmin < t < tmax; among equal t the first triangle.
    -> dict(geometry uint32 [n] (NO_SUBMESH: none), primitive uint32 [n], t [n] (inf: none)), computed in `dtype` throughout."""
    v0, e1, e2 = (np.ascontiguousarray(a, dtype) for a in tris[:3])
    gi, prim = tris[3], tris[4]
    d = np.ascontiguousarray(d, dtype).reshape(-1, 3)
    n = d.shape[0]
    o = np.broadcast_to(np.asarray(o, dtype), (n, 3))
    lo = np.broadcast_to(np.asarray(tmin, dtype), (n,))
    eps = dtype(1e-14)
    best = np.full(n, np.inf, dtype)
    which = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for a in range(0, n, ray_chunk):
            oo, dd, ll = o[a:a + ray_chunk, None, :], d[a:a + ray_chunk, None, :], lo[a:a + ray_chunk, None]
            rows = np.arange(dd.shape[0])
            for b in range(0, len(gi), tri_chunk):
                V0, E1, E2 = v0[None, b:b + tri_chunk], e1[None, b:b + tri_chunk], e2[None, b:b + tri_chunk]
                p = np.cross(dd, E2)
                det = np.sum(p * E1, -1)
                tv = oo - V0
                u = np.sum(p * tv, -1) / det
                q = np.cross(tv, E1)
                v = np.sum(dd * q, -1) / det
                t = np.sum(q * E2, -1) / det
                hit = (np.abs(det) > eps) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > ll) & (t < dtype(tmax))
                t = np.where(hit, t, dtype(np.inf))
                k = np.argmin(t, axis=1)  # (the first of equal minima)
                tk = t[rows, k]
                better = tk < best[a:a + ray_chunk]
                best[a:a + ray_chunk] = np.where(better, tk, best[a:a + ray_chunk])
                which[a:a + ray_chunk] = np.where(better, b + k, which[a:a + ray_chunk])
    found = which >= 0
    w = np.where(found, which, 0)
    return dict(geometry=np.where(found, gi[w], NO_SUBMESH).astype(np.uint32), primitive=np.where(found, prim[w], NO_SUBMESH).astype(np.uint32), t=best)


def primary(sc, cam, W, H, dtype=np.float64, tris=None):
    """every pixel's primary ray (the camera basis of neb_gbuffer_raycast, reproject_ref.Camera) against the scene
    -> dict(geometry, primitive, t [H, W], covered bool [H, W]: the closest hit lies between the near and the far plane)"""
    c = R.Camera(cam, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ndc_x = ((xs + 0.5) / W * 2.0 - 1.0).astype(dtype)
    ndc_y = (1.0 - (ys + 0.5) / H * 2.0).astype(dtype)
    xa, ya, za = [np.asarray(v, dtype) for v in (c.x, c.y, c.z)]
    d = xa * (ndc_x * dtype(c.sx))[..., None] + ya * (ndc_y * dtype(c.sy))[..., None] - za
    d = (d / np.sqrt(np.sum(d * d, -1, keepdims=True))).astype(dtype)
    out = cast(tris if tris is not None else triangles(sc), np.asarray(c.eye, dtype), d.reshape(-1, 3), dtype=dtype)
    out = {k: v.reshape(H, W) for k, v in out.items()}
    with np.errstate(all="ignore"):
        zv = out["t"] * -(d @ za)  # distance along the view axis
        out["covered"] = (out["geometry"] != NO_SUBMESH) & (zv >= dtype(cam.znear)) & (zv <= dtype(cam.zfar))
    return out


def differing(a, b):
    """pixels at which two primary casts disagree in coverage or, where both are covered, in the submesh they see"""
    return (a["covered"] != b["covered"]) | (a["covered"] & b["covered"] & (a["geometry"] != b["geometry"]))


def bounce_rays(gb, c):
    """The first bounce ray of every pixel of a one-sample GI dispatch, rebuilt from a G-buffer (planes as the library stores them:
    albedo, rough_metal, world_pos, normal) and the dispatch's constants with the arithmetic of oracle/gi_np.py's trace (its first
    lines, up to the ray) -> (origins, directions float32 [H * W, 3]); the rays start at tmin = 0.01."""
    from oracle import gi_np as G
    U = np.uint32
    H, W = gb["albedo"].shape
    n = H * W
    yy, xx = np.meshgrid(np.arange(H, dtype=U), np.arange(W, dtype=U), indexing="ij")
    rng = G.jenkins_hash((xx.reshape(-1) + yy.reshape(-1) * U(W)) ^ G.jenkins_hash(np.array([c.frameIndex], U)))
    world_pos = gb["world_pos"].reshape(n, 4)[:, :3].astype(F)
    SN = G.oct16_fast_unpack(gb["normal"].reshape(n, 4)[:, 2:4])
    G.rand(rng)      # NrcCreatePathState
    G.rand(rng)      # the draw against the specular probability: it scales the throughput, not the ray
    u0, u1 = G.rand2(rng)
    return (world_pos + SN * F(1e-2)).astype(F), G.cosine_sample_hemisphere_surface_aligned(u0, u1, SN)


# ------------------------------------------------------------------------------------------------
# the beamed room
# ------------------------------------------------------------------------------------------------
RUG, BEAMS, POST = 5, 6, 7      # geometry indices after cornell_parts' five (0 shell, 1 short box, 2 tall box, 3 red wall, 4 green wall)


def _rotation(axis, deg, about):
    """4x4, row-vector convention: a rotation by deg about the axis (0 x, 1 y, 2 z) through the point `about`"""
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R3 = np.eye(3)
    R3[i, i], R3[i, j], R3[j, i], R3[j, j] = c, s, -s, c
    T = np.eye(4)
    T[:3, :3] = R3
    p = np.asarray(about, np.float64)
    T[3, :3] = p - p @ R3
    return T


def beamed_room():
    """cornell_parts() plus 5 a floor patch of 24 x 24 cells two
    centimetres above the floor, 6 four thin beams across the room as one submesh, 7 one post from floor to ceiling.  The beams and
    the post are axis-parallel boxes in their own space, tilted by their submesh's matrix: each of their long triangles has a world
    box that spans a good part of the room, as the shell's and the walls' quads do, while the patch brings the mean box area down --
    these are the triangles the builder's reference splitting takes (oversized())."""
    sc = cornell_parts()
    M = sc.geometries[0]["M"].astype(np.float64)
    Minv = np.linalg.inv(M)
    mat = sc.geometries[1]["material"]

    def add(part, world):
        """`part` in a space of its own, `world` (4x4) takes it to its place in the room"""
        P, N, UV, I = part
        sc.add_geometry(P, N, UV, I, material=mat, M=np.ascontiguousarray(world @ np.eye(4), F))

    def patch(u, v):
        pos = np.stack([-0.93 + 1.83 * u, np.full_like(u, -0.98), -1.91 + 1.79 * v], -1)
        nrm = np.zeros_like(pos)
        nrm[..., 1] = 1.0
        return pos, nrm
    P, N, UV, I = S._grid_surface(patch, N_CELLS, N_CELLS, uv_scale=(3.0, 3.0))
    I = I.reshape(-1, 3)[:, ::-1].reshape(-1)  # (counter-clockwise seen from above, as the normals say)
    sc.add_geometry((P @ Minv[:3, :3] + Minv[3, :3]).astype(F), (N @ Minv[:3, :3]).astype(F), UV, I, material=sc.geometries[0]["material"], M=M.astype(F))
    beams = [S._box((-0.93, y, z - 0.02), (0.93, y + 0.04, z + 0.02)) for y, z in ((0.40, -0.67), (0.47, -0.89), (0.55, -1.12), (0.62, -1.31))]
    tilt = _rotation(1, 35.0, (0.0, 0.5, -1.0)) @ _rotation(2, 20.0, (0.0, 0.5, -1.0))
    add(S._merge(beams), tilt)
    post = S._box((-0.02, -0.97, -0.02), (0.02, 0.93, 0.02))
    lean = _rotation(2, 27.0, (0.0, 0.0, 0.0)) @ _rotation(0, 19.0, (0.0, 0.0, 0.0))
    lean[3, :3] += (-0.45, 0.0, -0.5)
    add(post, lean)
    return sc


def oversized(sc):
    """gi_build.hip's split_references, its first step: the triangles whose world box has more than 16 times the mean half area
    -> (bool per triangle in scene order, the geometry index of each)"""
    v0, e1, e2, gi = scene_triangles(sc)
    v0, e1, e2 = (a.astype(F) for a in (v0, e1, e2))
    pts = np.stack([v0, v0 + e1, v0 + e2])
    ext = (pts.max(0) - pts.min(0)).astype(np.float64)
    area = ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0]
    return area > 16.0 * area.mean(), gi


# ------------------------------------------------------------------------------------------------
# updates (4x4 world-space motions, row-vector convention, and deformation parameters)
# ------------------------------------------------------------------------------------------------
def beams_shift():
    T = np.eye(4)
    T[3, :3] = (0.057, -0.171, 0.113)
    return T


def carried_out(what):
    """`box`: to three times the room's extent (2 units) outside it; `beams`: beyond +-218 units, where the sun table's certificate ends"""
    T = np.eye(4)
    T[3, :3] = {"box": (6.3, 0.4, 0.9), "beams": (-3.0, 1.0, -260.0)}[what]
    return T


def mirror_of_the_tall_box():
    """a reflection in the vertical plane x = 0.4 through the tall box's centre, turned by 31 degrees about the vertical through it:
    determinant -1"""
    T = np.eye(4)
    T[0, 0] = -1.0
    T[3, 0] = 0.8
    return T @ _rotation(1, 31.0, (0.4, 0.0, -1.6))


RUG_SINE = dict(amplitude=0.012, wavelength=0.57, phase=0.3)
POST_SINE = dict(amplitude=0.008, wavelength=0.9, phase=1.1)


# ------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------
def look(eye, target, up=(0.0, 1.0, 0.0), zfar=100.0):
    cam = S.CameraDesc()
    cam.eye[:], cam.target[:], cam.up[:] = [float(v) for v in eye], [float(v) for v in target], [float(v) for v in up]
    cam.vfov_deg, cam.znear, cam.zfar = 60.0, 0.1, zfar
    return cam


def swept_views(room_camera):
    """the views of every update inside the room.  None looks along an axis exactly or sits on a plane of symmetry: the patch's grid
    lines and the boxes' edges cross the pixel centres at an angle."""
    return {
        "room": room_camera,
        "+x": look((-0.83, -0.13, -0.91), (0.9, -0.41, -1.13)),
        "-x": look((0.87, 0.23, -1.07), (-0.9, -0.37, -0.81)),
        "+z": look((-0.43, 0.12, -1.87), (-0.11, -0.33, 0.0)),
        "-z": look((-0.17, 0.11, -0.13), (0.09, -0.29, -2.0)),
        "down": look((0.07, 0.93, -1.03), (0.03, -1.0, -0.97), up=(0.31, 0.0, -1.0)),
        "along a beam": look((-0.91, 0.41, -0.71), (0.9, 0.69, -0.17)),
        "where the tall box stood": look((0.66, -0.31, -1.34), (-0.6, -0.6, -0.3)),
    }


def outside_views():
    """for the moves out of the scene box (carried_out): from inside the room, from the carried box's side looking back, and from
    above the room's open front towards where the beams went, with the room in the lower half of the frame"""
    return {
        "from inside": look((-0.13, 0.07, -0.23), (0.37, -0.21, -1.7), zfar=FAR),
        "looking back": look((7.3, 0.3, 1.1), (0.0, -0.5, -1.0), zfar=FAR),
        "both": look((-3.2, 1.8, -262.1), (0.5, -0.2, -1.0), zfar=FAR),
    }


# ------------------------------------------------------------------------------------------------
# the scene states of the GPU tests, each with the views it is looked at from
# ------------------------------------------------------------------------------------------------
def room_updates():
    """the three updates of the sweep, cumulative -> (the room, [(name, kind, payload, the scene after it)]); payload: (indices,
    matrices) of update_transforms, or {geometry: arrays} of update_vertices"""
    sc0 = beamed_room()
    m1 = moved_matrices(sc0, [1, 2], world_transform("rotate"))
    s1 = with_matrices(sc0, [1, 2], m1)
    m2 = moved_matrices(s1, [BEAMS], beams_shift())
    s2 = with_matrices(s1, [BEAMS], m2)
    deform = {RUG: sine_along_normal(s2, RUG, **RUG_SINE), POST: sine_along_normal(s2, POST, **POST_SINE)}
    s3 = with_arrays(s2, deform)
    return sc0, [("rotate the boxes", "transforms", ([1, 2], m1), s1), ("shift the beams", "transforms", ([BEAMS], m2), s2),
                 ("sine on patch and post", "vertices", deform, s3)]


def carried_updates():
    """-> (the room, indices, matrices that carry the short box and the beams out, the scene then)"""
    sc0 = beamed_room()
    mats = np.concatenate([moved_matrices(sc0, [1], carried_out("box")), moved_matrices(sc0, [BEAMS], carried_out("beams"))])
    return sc0, [1, BEAMS], mats, with_matrices(sc0, [1, BEAMS], mats)


def view_cases():
    """every (scene state, camera) pair the GPU tests compare with the float64 caster: {name: (scene, camera, W, H)}"""
    out = {}
    sc0, updates = room_updates()
    for name, _, _, sc in updates:
        for vname, cam in swept_views(cornell_camera()).items():
            out[f"{name} / {vname}"] = (sc, cam, VW, VH)
    sc0, _, _, far = carried_updates()
    for state, sc in (("carried out", far), ("brought back", sc0)):
        for vname, cam in outside_views().items():
            if state == "carried out" or vname != "both":  # (from behind where the beams were, the room is a third of a pixel)
                out[f"{state} / {vname}"] = (sc, cam, VW, VH)
    return out
