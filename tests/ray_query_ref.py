"""Ray sets for neb_gi_cast_rays and the judge of its answers against the float64 brute-force caster (tests/views_ref.py).
TEST INFRASTRUCTURE, NOT PRODUCT CODE.  tests/test_ray_query_cpu.py shows on the CPU that the judge is right and able to fail, and
measures what its tolerances are derived from; tests/test_ray_query_gpu.py judges the device with it.

A ray is a row of 8 float32 {origin xyz, tmin, direction xyz, tmax} (neb_ray); the reference is computed in float64 FROM THE FLOAT32
VALUES the device is handed.  An answer names a triangle (geometry, primitive) with t, u, v, or is a miss (geometry = NO_SUBMESH).

The judge.  views_ref.cast in float64 gives T* and the winning triangle.  A device answer is RIGHT if it names that triangle or a
COINCIDENT one -- float64 Moeller-Trumbore of the ray against the triangle it names gives |t - T*| <= 1e-9 max(1, T*), u, v >= -1e-5,
u + v <= 1 + 1e-5 (the test scenes hold exactly coincident surfaces, and which of two triangles at one distance a walk reports depends
on its order) -- and WRONG otherwise; a miss is right where float64 finds nothing in the interval.  Wrong answers are capped per set
at TIE_CAP (test_refit_gpu: rays that graze an edge within rounding).  Where the answer is right, t (relative to max(1, t)), u and v
(absolute) must lie within T_TOL, U_TOL, V_TOL of the float64 values on the triangle the answer names: no exception is allowed.

The tolerances are not picked by hand: they are FOUR TIMES the largest error of a float32 evaluation of the same rays (views_ref.cast
and the arithmetic below in float32), measured by test_ray_query_cpu.test_calibration over every set on every scene state the GPU
tests use -- four times, because the device orders its operations differently from the float32 caster.  Measured there (maxima over
the three states and five sets): t 1.35e-5, u 4.0e-5, v 6.2e-5 (rounded up from 1.343e-5, 3.997e-5, 6.178e-5); the test prints
them on every run and holds the constants to them."""
import numpy as np

import views_ref as V
from motion_ref import NO_SUBMESH
from test_refit_gpu import TIE_CAP  # noqa: F401

F = np.float32
N_RAYS = 4096
SETS = ("scattered", "outside", "axis", "second", "short")
T_MEASURED, U_MEASURED, V_MEASURED = 1.35e-5, 4.0e-5, 6.2e-5  # float32 against float64, test_ray_query_cpu.test_calibration
T_TOL, U_TOL, V_TOL = 4 * T_MEASURED, 4 * U_MEASURED, 4 * V_MEASURED
COINCIDENT_T, COINCIDENT_UV = 1e-9, 1e-5


# ------------------------------------------------------------------------------------------------
# triangles
# ------------------------------------------------------------------------------------------------
def triangles(sc, hidden=()):
    """views_ref.triangles without the submeshes in `hidden` (the others keep their numbers)"""
    tris = V.triangles(sc)
    if not len(hidden):
        return tris
    keep = ~np.isin(tris[3], np.asarray(list(hidden)))
    return tuple(a[keep] for a in tris)


def _lookup(tris):
    """-> (sorted keys geometry << 32 | primitive, the triangle of each)"""
    key = (tris[3].astype(np.uint64) << np.uint64(32)) | tris[4].astype(np.uint64)
    order = np.argsort(key)
    return key[order], order


def triangle_index(tris, geometry, primitive):
    """the index into `tris` of each (geometry, primitive), -1 where the scene has no such triangle"""
    keys, order = _lookup(tris)
    want = (np.asarray(geometry).astype(np.uint64) << np.uint64(32)) | np.asarray(primitive).astype(np.uint64)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return np.where(keys[pos] == want, order[pos], -1)


def moller_trumbore(tris, index, rays, dtype=np.float64):
    """ray k against triangle index[k], views_ref.cast's operations in `dtype` -> (t, u, v); u weighs v0 + e1, v weighs v0 + e2"""
    v0, e1, e2 = (np.asarray(a, dtype)[index] for a in tris[:3])
    o, d = np.asarray(rays[:, 0:3], dtype), np.asarray(rays[:, 4:7], dtype)
    with np.errstate(all="ignore"):
        p = np.cross(d, e2)
        det = np.sum(p * e1, -1)
        tv = o - v0
        u = np.sum(p * tv, -1) / det
        q = np.cross(tv, e1)
        v = np.sum(d * q, -1) / det
        t = np.sum(q * e2, -1) / det
    return t, u, v


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def reference(tris, rays, dtype=np.float64):
    """the closest hit of every ray with tmin < t < tmax -> dict(geometry, primitive (NO_SUBMESH: none), t (inf: none), u, v, hit bool).
    (views_ref.cast takes one tmax for all rays: it is run to infinity, and a closest hit at or beyond a ray's own tmax is no hit --
    the closest hit below tmax is the closest hit of all, or there is none.)"""
    rays = np.asarray(rays, F)
    out = V.cast(tris, rays[:, 0:3], rays[:, 4:7], tmin=rays[:, 3], dtype=dtype)
    hit = (out["geometry"] != NO_SUBMESH) & (out["t"] < rays[:, 7].astype(dtype))
    out["geometry"] = np.where(hit, out["geometry"], NO_SUBMESH).astype(np.uint32)
    out["primitive"] = np.where(hit, out["primitive"], NO_SUBMESH).astype(np.uint32)
    out["t"] = np.where(hit, out["t"], np.inf)
    idx = triangle_index(tris, out["geometry"], out["primitive"])
    _, u, v = moller_trumbore(tris, np.maximum(idx, 0), rays, dtype)
    out["u"], out["v"], out["hit"] = np.where(hit, u, 0.0), np.where(hit, v, 0.0), hit
    return out


def answers(ref):
    """a reference (or any dict with these keys) as the device would report it: what the judge takes"""
    return {k: np.array(ref[k]) for k in ("t", "u", "v", "geometry", "primitive")}


# ------------------------------------------------------------------------------------------------
# ray sets
# ------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _rays(o, d, tmin=0.0, tmax=np.inf):
    n = len(o)
    r = np.empty((n, 8), F)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3], r[:, 7] = tmin, tmax
    return r


def scattered_rays(lo, hi, n, rng):
    """origins uniform in the inner 96 % of the box [lo, hi], directions uniform on the sphere scaled by a length in [0.25, 4]"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + 0.96 * h * rng.uniform(-1.0, 1.0, (n, 3))
    return _rays(o, _unit(rng, n) * rng.uniform(0.25, 4.0, (n, 1)))


def ray_sets(lo, hi, tris, seed=7, n=N_RAYS):
    """the five sets for a scene box [lo, hi] -> {name: float32 [n, 8]}
    scattered: origins uniform in the inner 96 % of the box, directions uniform on the sphere scaled by a length in [0.25, 4]
    outside:   origins on a sphere of 2.5 box diagonals around the centre, aimed at uniform points of the inner 80 % (not normalised)
    axis:      the scattered origins, directions with one or two components exactly +-1 and the rest exactly 0 (1 / d infinite)
    second:    the scattered rays with tmin = t1 * 1.001 + 1e-4 behind their float64 first hit t1 (rays without one keep tmin = 0)
    short:     the scattered rays with tmax = 0.5 t1: float64 says miss for every ray that had a hit"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    scattered = scattered_rays(lo, hi, n, rng)
    diag = float(np.linalg.norm(hi - lo))
    oo = c + 2.5 * diag * _unit(rng, n)
    outside = _rays(oo, c + 0.8 * h * rng.uniform(-1.0, 1.0, (n, 3)) - oo)
    d = np.zeros((n, 3))
    first = rng.integers(0, 3, n)
    d[np.arange(n), first] = rng.choice([-1.0, 1.0], n)
    two = rng.random(n) < 0.5
    other = (first + rng.integers(1, 3, n)) % 3
    d[np.arange(n)[two], other[two]] = rng.choice([-1.0, 1.0], int(two.sum()))
    axis = _rays(scattered[:, 0:3], d)
    t1 = reference(tris, scattered)
    second, short = scattered.copy(), scattered.copy()
    second[:, 3] = np.where(t1["hit"], t1["t"] * 1.001 + 1e-4, 0.0)
    short[:, 7] = np.where(t1["hit"], 0.5 * t1["t"], np.inf)
    return dict(scattered=scattered, outside=outside, axis=axis, second=second, short=short)


def submeshes_seen(name, sets, ref, tris):
    """the submeshes a set's rays find.  `short` finds none by construction: for it, the submeshes its rays were cut short of."""
    if name == "short":
        ref = reference(tris, sets["scattered"])
    return sorted(set(ref["geometry"][ref["hit"]].tolist()))


# ------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------
def judge(tris, rays, ref, got):
    """ref: reference(tris, rays); got: dict(t, u, v, geometry, primitive) per ray
    -> dict(wrong bool [n], tie bool [n]: right by a coincident triangle, off bool [n]: right triangle but t, u or v out of tolerance,
            err_t, err_u, err_v: the largest errors on the right answers)"""
    rays = np.asarray(rays, F)
    g, p = np.asarray(got["geometry"]).astype(np.uint32), np.asarray(got["primitive"]).astype(np.uint32)
    got_hit = g != NO_SUBMESH
    idx = triangle_index(tris, g, p)
    t64, u64, v64 = moller_trumbore(tris, np.maximum(idx, 0), rays)
    same = ref["hit"] & got_hit & (g == ref["geometry"]) & (p == ref["primitive"])
    with np.errstate(all="ignore"):
        coincident = (ref["hit"] & got_hit & ~same & (idx >= 0) & (np.abs(t64 - ref["t"]) <= COINCIDENT_T * np.maximum(1.0, ref["t"]))
                      & (u64 >= -COINCIDENT_UV) & (v64 >= -COINCIDENT_UV) & (u64 + v64 <= 1.0 + COINCIDENT_UV))
        right_hit = same | coincident
        right = right_hit | (~ref["hit"] & ~got_hit)
        et = np.where(right_hit, np.abs(np.asarray(got["t"], np.float64) - t64) / np.maximum(1.0, np.abs(t64)), 0.0)
        eu = np.where(right_hit, np.abs(np.asarray(got["u"], np.float64) - u64), 0.0)
        ev = np.where(right_hit, np.abs(np.asarray(got["v"], np.float64) - v64), 0.0)
    et, eu, ev = (np.where(np.isnan(e), np.inf, e) for e in (et, eu, ev))
    off = right_hit & ((et > T_TOL) | (eu > U_TOL) | (ev > V_TOL))
    # a miss is reported as t = inf exactly
    bad_miss = ~got_hit & ~np.isposinf(np.asarray(got["t"], np.float64))
    return dict(wrong=~right | bad_miss, tie=coincident, off=off, err_t=float(et.max(initial=0.0)), err_u=float(eu.max(initial=0.0)),
                err_v=float(ev.max(initial=0.0)))


def check(verdict, what, cap=TIE_CAP):
    """raises unless at most `cap` answers are wrong and every right one is within the tolerances"""
    n_wrong, n_off = int(verdict["wrong"].sum()), int(verdict["off"].sum())
    print(f"[{what}] wrong {n_wrong}, right by a coincident triangle {int(verdict['tie'].sum())}, out of tolerance {n_off}; "
          f"largest errors t {verdict['err_t']:.2e} u {verdict['err_u']:.2e} v {verdict['err_v']:.2e}")
    assert n_wrong <= cap, f"{what}: {n_wrong} answers are neither float64's triangle nor a coincident one; first at ray {int(np.nonzero(verdict['wrong'])[0][0])}"
    assert n_off == 0, (f"{what}: {n_off} right answers are out of tolerance (t {verdict['err_t']:.2e} / {T_TOL:.1e}, u {verdict['err_u']:.2e} / {U_TOL:.1e}, "
                        f"v {verdict['err_v']:.2e} / {V_TOL:.1e}); first at ray {int(np.nonzero(verdict['off'])[0][0])}")
    return n_wrong


def check_any_hit(occluded, ref, what, cap=TIE_CAP):
    """the device's word per ray against "float64 finds a hit in the interval" """
    n = int((np.asarray(occluded).astype(bool) != ref["hit"]).sum())
    print(f"[{what}] any-hit words differ from float64 at {n} rays")
    assert n <= cap, f"{what}: any-hit differs from float64 at {n} rays"
    assert set(np.unique(occluded).tolist()) <= {0, 1}, f"{what}: an any-hit word that is neither 0 nor 1"
    return n


# ------------------------------------------------------------------------------------------------
# the scene states of the GPU tests
# ------------------------------------------------------------------------------------------------
HIDDEN = 2  # the tall box


def states():
    """-> {name: (scene, hidden submeshes)}: the beamed room, the room after its three updates, that state without submesh 2"""
    sc0, updates = V.room_updates()
    last = updates[-1][3]
    return {"room": (sc0, ()), "updated": (last, ()), "updated, 2 hidden": (last, (HIDDEN,))}


def scene_box(sc):
    lo, hi = sc.world_aabb()
    return np.asarray(lo, np.float64), np.asarray(hi, np.float64)
