"""The scenes of the sun-table audit (tests/test_sun_audit_gpu.py on the device, tests/test_sun_audit_cpu.py with the CPU prototype's
flags): each the smallest shape at which one mechanism of gi_sun_table.hip's build can still go wrong.  TEST INFRASTRUCTURE.

cases() -> {name: Case}.  Building a Case's scene touches no device."""
import math
from dataclasses import dataclass
from typing import Callable

import numpy as np

from nebulae_amd import scene as S

F = np.float32
SUN = (0.5, -1.0, -0.2)  # the default sun (scene.default_constants)
DISK = 0.58              # its diameter in degrees (renderer default)


@dataclass
class Case:
    make: Callable            # -> Scene
    sun: tuple = SUN
    disk: float = DISK
    table: bool = True        # False: the device builds no table for this scene
    shares: bool = False      # trace every sampled ray and assert `floor` on share (c)
    floor: float = 0.0


def _material(sc):
    return sc.add_material(albedo=(0.7, 0.6, 0.5, 1), rm=(0.8, 0.0))


def _small_tri(c, size=0.03):
    """a small triangle that faces +y, centred at c"""
    c = np.asarray(c, np.float64)
    P = np.array([c + (-size, 0, size), c + (size, 0, size), c + (0, 0, -size)], F)
    return P, np.tile(np.array([[0, 1, 0]], F), (3, 1)), np.zeros((3, 2), F), np.array([0, 1, 2], np.uint32)


def _over(base, h, sun=SUN):
    """the point h above `base` (a point of a floor) on the line towards the sun: what lies there shadows `base` under the disk's centre"""
    s = np.asarray(sun, np.float64)
    return np.asarray(base, np.float64) - s * (h / -s[1])


# ------------------------------------------------------------------------------------------------
# wave edges: flat grids of n triangles in all, a small roof (2 of them) over a part
# ------------------------------------------------------------------------------------------------
def grid_scene(n_tris):
    sc = S.Scene(f"grid-{n_tris}")
    m = _material(sc)
    n_floor = n_tris if n_tris <= 2 else n_tris - 2
    per_row, cell = 16, 0.25
    P, I = [], []
    for k in range(n_floor):
        row, i = divmod(k, per_row)
        c, upper = divmod(i, 2)
        x0, x1, z0, z1 = c * cell - 1.0, (c + 1) * cell - 1.0, -row * cell, -(row + 1) * cell
        q = [(x0, -1.0, z0), (x1, -1.0, z0), (x1, -1.0, z1), (x0, -1.0, z1)]
        tri = (q[0], q[2], q[3]) if upper else (q[0], q[1], q[2])
        I += [len(P), len(P) + 1, len(P) + 2]
        P += tri
    P = np.array(P, F)
    N = np.tile(np.array([[0, 1, 0]], F), (len(P), 1))
    parts = [(P, N, np.zeros((len(P), 2), F), np.array(I, np.uint32))]
    if n_tris > 2:
        rows = (n_floor + per_row - 1) // per_row
        cx, cz = _over((0.0, -1.0, -0.5 * rows * cell), 0.3)[[0, 2]]
        parts.append(S._quad((cx - 0.3, -0.7, cz + 0.3), (cx + 0.3, -0.7, cz + 0.3), (cx + 0.3, -0.7, cz - 0.3), (cx - 0.3, -0.7, cz - 0.3)))
    sc.add_geometry(*S._merge(parts), material=m)
    assert sc.num_triangles == n_tris
    return sc


# ------------------------------------------------------------------------------------------------
# one lane's queue overflowing; many lanes at once
# ------------------------------------------------------------------------------------------------
def queue_scene(k, inside):
    """One receiver quad [0, 1]^2 at y = 0 (geometry 0: triangle 0 = the half x > z', triangle 1 the other) and k small occluders
    (geometry 1) over triangle 0's footprint (inside) or over triangle 1's -- outside triangle 0's footprint, inside its box.  The first
    occluder stands over the centroid sample of the triangle it shadows."""
    sc = S.Scene(f"queue-{k}-{'in' if inside else 'out'}")
    m = _material(sc)
    sc.add_geometry(*S._quad((0, 0, 0), (1, 0, 0), (1, 0, -1), (0, 0, -1)), material=m)  # triangles (p0 p1 p2), (p0 p2 p3)
    rng = np.random.default_rng(100 + k)
    a, b, c = (np.array(p, np.float64) for p in (((0, 0, 0), (1, 0, 0), (1, 0, -1)) if inside else ((0, 0, 0), (1, 0, -1), (0, 0, -1))))
    occ = []
    for j in range(k):
        u, v = rng.random(2)
        if u + v > 1:
            u, v = 1 - u, 1 - v
        u, v = 0.08 + 0.76 * u, 0.08 + 0.76 * v  # (the whole occluder stays inside the column, the disk's spread included)
        base = (a + b + c) / 3 if j == 0 else a + u * (b - a) + v * (c - a)
        occ.append(_small_tri(_over(base, 0.2 + 1.3 * j / max(1, k - 1))))
    sc.add_geometry(*S._merge(occ), material=m)
    return sc


def stack_scene(k=2500):
    """One receiver quad and k small occluders stacked over a patch of 0.4 x 0.4 of its first triangle, up to 3 units high: all of them
    lie in the receiver's column and none covers it, so its hint walk visits every node over the patch -- more than the 320 a hint walk
    may visit -- while only the top of the stack is lit (few rays to trace)."""
    sc = S.Scene(f"stack-{k}")
    m = _material(sc)
    sc.add_geometry(*S._quad((0, 0, 0), (1, 0, 0), (1, 0, -1), (0, 0, -1)), material=m)
    rng = np.random.default_rng(2500)
    occ = [_small_tri(_over((0.45 + 0.4 * rng.random(), 0.0, -0.05 - 0.3 * rng.random()), 0.2 + 2.8 * j / (k - 1))) for j in range(k)]
    sc.add_geometry(*S._merge(occ), material=m)
    return sc


def strip_scene(n_receivers=64, per_receiver=17):
    """a strip of n_receivers triangles, per_receiver small occluders over each (the first over its centroid)"""
    sc = S.Scene(f"strip-{n_receivers}x{per_receiver}")
    m = _material(sc)
    quads = [S._quad((q * 0.5, 0, 0), (q * 0.5 + 0.5, 0, 0), (q * 0.5 + 0.5, 0, -0.5), (q * 0.5, 0, -0.5)) for q in range(n_receivers // 2)]
    sc.add_geometry(*S._merge(quads), material=m)
    P, _, _, I = sc.geometries[0]["positions"], None, None, sc.geometries[0]["indices"].reshape(-1, 3)
    rng = np.random.default_rng(17)
    occ = []
    for t in range(n_receivers):
        a, b, c = (P[i].astype(np.float64) for i in I[t])
        for j in range(per_receiver):
            u, v = rng.random(2)
            if u + v > 1:
                u, v = 1 - u, 1 - v
            u, v = 0.1 + 0.7 * u, 0.1 + 0.7 * v
            base = (a + b + c) / 3 if j == 0 else a + u * (b - a) + v * (c - a)
            occ.append(_small_tri(_over(base, 0.15 + 0.05 * j), size=0.012))
    sc.add_geometry(*S._merge(occ), material=m)
    return sc


# ------------------------------------------------------------------------------------------------
# the single occluder among decoys
# ------------------------------------------------------------------------------------------------
def _decoys(n, where, y):
    """n small triangles in the plane y, spread over the rectangle where = (x0, x1, z0, z1): coplanar, they shadow nothing"""
    x0, x1, z0, z1 = where
    side = int(math.ceil(math.sqrt(n)))
    out = []
    for j in range(n):
        r, c = divmod(j, side)
        out.append(_small_tri((x0 + (c + 0.5) * (x1 - x0) / side, y, z0 + (r + 0.5) * (z1 - z0) / side), size=0.02))
    return S._merge(out)


def sliver_scene(position):
    """Receiver quad [0, 1] x [0, -1] at y = 0 (geometry 0); geometry 1: ONE triangle whose shadow under the disk's centre is the corner
    {x - z' >= 1 - s} of receiver triangle 0, s^2 = 1e-3 of its area, at the corner p1 = (1, 0, 0) (z' = -z); geometry 2: 500 decoys in
    the receiver's plane.  position: where the occluder should come in leaf (Morton) order -- "first": low, before the decoys' corner;
    "middle": decoys on both sides; "last": at the top of the scene, the decoys all lower and nearer the origin."""
    sc = S.Scene(f"sliver-{position}")
    m = _material(sc)
    sc.add_geometry(*S._quad((0, 0, 0), (1, 0, 0), (1, 0, -1), (0, 0, -1)), material=m)
    s = math.sqrt(1e-3)
    h = {"first": 0.05, "middle": 0.05, "last": 3.0}[position]
    # in the floor plane (x, z'): the edge P Q on the line x - z' = 1 - s, the third vertex beyond the corner
    foot = [(1 - s - 0.2, 0.0, 0.2), (1 + 0.5, 0.0, 0.5), (1 + 0.2, 0.0, -(s + 0.2))]
    P = np.array([_over(p, h) for p in foot], F)
    sc.add_geometry(P, np.tile(np.array([[0, 1, 0]], F), (3, 1)), np.zeros((3, 2), F), np.array([0, 1, 2], np.uint32), material=m)
    where = {"first": (3.0, 6.0, -6.0, -3.0), "middle": (-3.0, 5.0, -4.0, 3.0), "last": (-6.0, -1.0, 1.0, 6.0)}[position]
    sc.add_geometry(*_decoys(500, where, 0.0), material=m)
    return sc


def full_occluder_scene():
    """Receiver quad (geometry 0) wholly under ONE triangle (geometry 1); 50 decoys in the receiver's plane (geometry 2) cover nothing."""
    sc = S.Scene("full-occluder")
    m = _material(sc)
    sc.add_geometry(*S._quad((0, 0, 0), (1, 0, 0), (1, 0, -1), (0, 0, -1)), material=m)
    foot = [(-1.0, 0.0, 1.0), (3.5, 0.0, 1.0), (-1.0, 0.0, -3.5)]
    P = np.array([_over(p, 0.6) for p in foot], F)
    sc.add_geometry(P, np.tile(np.array([[0, 1, 0]], F), (3, 1)), np.zeros((3, 2), F), np.array([0, 1, 2], np.uint32), material=m)
    sc.add_geometry(*_decoys(50, (4.0, 6.0, -2.0, 0.0), 0.0), material=m)
    return sc


# ------------------------------------------------------------------------------------------------
# sides and normals
# ------------------------------------------------------------------------------------------------
def grazed_scene(sun=SUN):
    """A floor, and over it two quads whose planes hold the sun direction (|N.L| at rounding level: the rays of a hit start on either
    side), one behind the other along the sun, and a roof over a part of the first."""
    sc = S.Scene("grazed")
    m = _material(sc)
    L = -np.asarray(sun, np.float64)
    L /= np.linalg.norm(L)
    a = np.cross(L, (0.0, 0.0, 1.0))
    a /= np.linalg.norm(a)
    b = np.cross(L, a)
    parts = [S._quad((-3, -1, 2), (3, -1, 2), (3, -1, -3), (-3, -1, -3))]
    for o, w in (((0.0, -0.2, 0.0), a), ((0.3, -0.2, -0.4), b)):
        o = np.asarray(o)
        p = [o - 0.5 * w - 0.4 * L, o + 0.5 * w - 0.4 * L, o + 0.5 * w + 0.4 * L, o - 0.5 * w + 0.4 * L]
        parts.append(S._quad(*p))
    c = _over((0.2, -0.2, 0.0), 0.9, sun)
    parts.append(S._quad((c[0] - 0.25, c[1], c[2] + 0.25), (c[0] + 0.25, c[1], c[2] + 0.25), (c[0] + 0.25, c[1], c[2] - 0.25), (c[0] - 0.25, c[1], c[2] - 0.25)))
    sc.add_geometry(*S._merge(parts), material=m)
    return sc


def sphere_scene():
    """a smooth-shaded sphere of 16 x 10 x 2 = 320 triangles (radial vertex normals: they disagree within every triangle, and the
    silhouette's triangles see the sun from both sides) over a ground of 128"""
    sc = S.Scene("sphere")
    m = _material(sc)

    def ball(u, v):
        a, b = u * 2 * np.pi, (v - 0.5) * np.pi
        d = np.stack([np.cos(b) * np.cos(a), np.sin(b), -np.cos(b) * np.sin(a)], -1)
        return np.array((0.1, 0.0, -0.2)) + 0.7 * d, d

    def ground(u, v):
        pos = np.stack([-2.5 + 5.0 * u, np.full_like(u, -1.0), 2.0 - 5.0 * v], -1)
        nrm = np.zeros_like(pos)
        nrm[..., 1] = 1.0
        return pos, nrm
    sc.add_geometry(*S._grid_surface(ball, 16, 10), material=m)
    sc.add_geometry(*S._grid_surface(ground, 8, 8), material=m)
    return sc


def mirrored_scene():
    """a box under a mirroring, non-uniformly scaled instance transform (determinant < 0) and a smooth blob under the same, over a ground"""
    sc = S.Scene("mirrored")
    m = _material(sc)
    M = np.eye(4, dtype=F)
    M[0, 0], M[1, 1], M[2, 2] = -1.3, 0.7, 1.1
    M[0, 1] = 0.2  # (a shear on top: the normals are transformed by M itself, as the shader does)
    M[3, :3] = (0.4, -0.3, -0.6)
    sc.add_geometry(*S._box((-0.4, -0.5, -0.4), (0.4, 0.5, 0.4)), material=m, M=M)

    def blob(u, v):
        a, b = u * 2 * np.pi, (v - 0.5) * np.pi
        d = np.stack([np.cos(b) * np.cos(a), np.sin(b), -np.cos(b) * np.sin(a)], -1)
        return np.array((1.2, 0.9, 0.3)) + 0.35 * d, d
    sc.add_geometry(*S._grid_surface(blob, 10, 6), material=m, M=M)

    def ground(u, v):
        pos = np.stack([-3.0 + 6.0 * u, np.full_like(u, -1.0), 2.5 - 5.0 * v], -1)
        nrm = np.zeros_like(pos)
        nrm[..., 1] = 1.0
        return pos, nrm
    sc.add_geometry(*S._grid_surface(ground, 6, 6), material=m)
    return sc


# ------------------------------------------------------------------------------------------------
# long walks, scale
# ------------------------------------------------------------------------------------------------
def longthin_scene():
    """The long-thin stand-in without what carries its triangle budget: the full-length strips of walls, gallery floors, undersides and
    roofs and the 40 beams across the court (scene.atrium_standin(long_thin=True), geometries 1-17) over a floor of 384 triangles.
    (Its longest hint walk is 144 nodes; denser floors do not lengthen it, the footprint test culls them: stack_scene is the one that reaches the cap.)"""
    full = S.atrium_standin(target_triangles=1, n_submeshes=18, tex_size=8, long_thin=True)
    sc = S.Scene("longthin-strips")
    sc.materials, sc.textures = full.materials, full.textures
    g0 = full.geometries[0]
    lo, hi = g0["positions"].min(0), g0["positions"].max(0)

    def floor(u, v):
        pos = np.stack([lo[0] + (hi[0] - lo[0]) * u, np.full_like(u, float(lo[1])), lo[2] + (hi[2] - lo[2]) * (1 - v)], -1)
        nrm = np.zeros_like(pos)
        nrm[..., 1] = 1.0
        return pos, nrm
    P, N, UV, I = S._grid_surface(floor, 16, 12)
    sc.add_geometry(P, N, UV, I.reshape(-1, 3)[:, ::-1].reshape(-1), material=g0["material"], M=g0["M"])
    sc.geometries += full.geometries[1:]
    return sc


def mini_atrium():
    """An atrium of about 600 triangles with the stand-in's extent and node scale: a floor, four galleries around an open court with
    their roofs, outer walls, twelve square columns and three smooth blobs on the court's floor."""
    sc = S.Scene("mini-atrium")
    m = _material(sc)
    s = 0.00800000037997961
    M = np.diag([s, s, s, 1.0]).astype(F)
    x0, x1, z0, z1, yf, y2, yc = -1920.0, 1800.0, -1180.0, 1105.0, 0.0, 560.0, 1429.0
    ix0, ix1, iz0, iz1 = x0 + 700, x1 - 700, z0 + 520, z1 - 520

    def plane(xa, xb, za, zb, y, nu, nv, up=True):
        def fn(u, v):
            pos = np.stack([xa + (xb - xa) * u, np.full_like(u, y), za + (zb - za) * (v if up else 1 - v)], -1)
            nrm = np.zeros_like(pos)
            nrm[..., 1] = 1.0 if up else -1.0
            return pos, nrm
        return S._grid_surface(fn, nu, nv)
    parts = [plane(x0, x1, z0, z1, yf, 10, 8)]
    for y, up in ((y2, True), (yc, True)):  # (gallery floors and the roofs' upper faces)
        parts += [plane(x0, ix0, z0, z1, y, 2, 6, up), plane(ix1, x1, z0, z1, y, 2, 6, up), plane(ix0, ix1, z0, iz0, y, 6, 2, up),
                  plane(ix0, ix1, iz1, z1, y, 6, 2, up)]
    for (xa, za), (xb, zb) in (((x0, z0), (x1, z0)), ((x1, z1), (x0, z1)), ((x0, z1), (x0, z0)), ((x1, z0), (x1, z1))):
        t = np.array([xb - xa, zb - za], float)
        n = -np.array([t[1], -t[0]]) / np.linalg.norm(t)

        def fn(u, v, xa=xa, za=za, t=t, n=n):
            pos = np.stack([xa + t[0] * (1 - u), yf + (yc - 5.0 - yf) * v, za + t[1] * (1 - u)], -1)  # (the walls end 4 cm under the roofs)
            nrm = np.zeros_like(pos)
            nrm[..., 0], nrm[..., 2] = n[0], n[1]
            return pos, nrm
        parts.append(S._grid_surface(fn, 4, 2))
    sc.add_geometry(*S._merge(parts), material=m, M=M)
    cols = [S._box((cx - 40, yf, cz - 40), (cx + 40, y2, cz + 40)) for cx in np.linspace(ix0, ix1, 5) for cz in (iz0, iz1)] + \
        [S._box((cx - 40, yf, -40.0), (cx + 40, y2, 40.0)) for cx in (ix0, ix1)]
    sc.add_geometry(*S._merge(cols), material=m, M=M)
    rng = np.random.default_rng(5)
    for k in range(3):
        c = np.array((rng.uniform(ix0 + 150, ix1 - 150), yf + 80.0, rng.uniform(iz0 + 100, iz1 - 100)))

        def blob(u, v, c=c):
            a, b = u * 2 * np.pi, (v - 0.5) * np.pi
            d = np.stack([np.cos(b) * np.cos(a), np.sin(b), -np.cos(b) * np.sin(a)], -1)
            return c + 70.0 * d, d
        sc.add_geometry(*S._grid_surface(blob, 6, 4), material=m, M=M)
    return sc


# ------------------------------------------------------------------------------------------------
# updates
# ------------------------------------------------------------------------------------------------
UPDATE_FLOOR, UPDATE_OCCLUDER, UPDATE_BARE = 0, 1, 2


def update_scene():
    """geometry 0: a floor of 8 x 8 cells under the open sky; 1: a slab beside it that shadows nothing of it (update_moved puts it over
    the floor); 2: a quad without a tangent stream -- a hit on it ends the path, no shadow ray starts there."""
    sc = S.Scene("update")
    m = _material(sc)

    def floor(u, v):
        pos = np.stack([-2.0 + 4.0 * u, np.full_like(u, -1.0), 2.0 - 4.0 * v], -1)
        nrm = np.zeros_like(pos)
        nrm[..., 1] = 1.0
        return pos, nrm
    sc.add_geometry(*S._grid_surface(floor, 8, 8), material=m)
    sc.add_geometry(*S._box((-0.8, -0.05, -0.8), (0.8, 0.05, 0.8)), material=m, M=update_matrix(False))
    sc.add_geometry(*S._quad((2.5, -1, 1), (3.5, -1, 1), (3.5, -1, 0), (2.5, -1, 0)), material=m, omit=("tangents",))
    return sc


def update_matrix(over_the_floor):
    M = np.eye(4, dtype=F)
    M[3, :3] = (0.3, -0.2, -0.1) if over_the_floor else (6.0, -0.9, 0.0)
    return M


def with_matrix(sc, index, M):
    out = S.Scene(sc.name)
    out.materials, out.textures = sc.materials, sc.textures
    out.geometries = [dict(g) for g in sc.geometries]
    out.geometries[index]["M"] = np.ascontiguousarray(M, F)
    return out


# ------------------------------------------------------------------------------------------------
def _beamed_room():
    import views_ref as V
    return V.beamed_room()


def cases():
    c = {}
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        c[f"grid_{n}"] = Case(lambda n=n: grid_scene(n))
    for k in (20, 40, 200):
        c[f"queue_{k}_inside"] = Case(lambda k=k: queue_scene(k, True))
        c[f"queue_{k}_outside"] = Case(lambda k=k: queue_scene(k, False))
    c["strip_64x17"] = Case(strip_scene)
    for p in ("first", "middle", "last"):
        c[f"sliver_{p}"] = Case(lambda p=p: sliver_scene(p))
    c["full_occluder"] = Case(full_occluder_scene, shares=True)
    c["sun_down_grid"] = Case(lambda: grid_scene(129), sun=(0.0, -1.0, 0.0))
    c["sun_down_cornell"] = Case(lambda: S.cornell_standin(), sun=(0.0, -1.0, 0.0))
    c["sun_plus_x_cornell"] = Case(lambda: S.cornell_standin(), sun=(1.0, 0.0, 0.0))
    c["grazed"] = Case(grazed_scene)
    c["grazed_3deg"] = Case(grazed_scene, disk=3.0)
    c["sphere"] = Case(sphere_scene, shares=True)
    c["sphere_3deg"] = Case(sphere_scene, disk=3.0, shares=True, floor=0.1)
    c["mirrored"] = Case(mirrored_scene, shares=True)
    c["grid_129_3deg"] = Case(lambda: grid_scene(129), disk=3.0)
    c["longthin"] = Case(longthin_scene)
    c["stack_2500"] = Case(stack_scene)
    c["split_room"] = Case(_beamed_room, sun=(0.23, -0.31, -0.92))
    c["atrium"] = Case(mini_atrium, shares=True, floor=0.6)
    c["atrium_3deg"] = Case(mini_atrium, sun=(-0.3, -1.0, 0.4), disk=3.0)  # (cells of 3 units under a 3-degree disk: next to nothing can be proven)
    c["atrium_shifted"] = Case(lambda: S.moved_scene(mini_atrium(), 1.0, (150.0, 40.0, -90.0)), shares=True, floor=0.1)
    c["atrium_x100"] = Case(lambda: S.moved_scene(mini_atrium(), 100.0, (2000.0, 500.0, -1000.0)), table=False)
    return c
