"""Reference for the grid tail of neb_gi_trace_paths_tail / neb_gi_bake_probes_tail (include/nebulae_hip.h, "THE TAIL").

tail32 restates steps 1, 4, 5, 6 and 7 of the contract in numpy float32 with one rounding per operation, so that a device record can be
compared BIT FOR BIT; tail64 is the same in float64.  `judge` compares the records of a tail call with those of the plain call over
the same rays and constants: every check of the issue's general case.  Its queries are callables -- on the device the library's own
shade_rays("surface") and gather_probes, in tests/test_probe_tail_cpu.py fabricated ones -- so that the judge itself runs, and is
shown to fail, on the CPU."""
import numpy as np

import path_ref as P
from nebulae_amd import _lib

F, F64, U32 = np.float32, np.float64, np.uint32
PI_INV = F(1.0) / F(3.14159265)
TAIL = U32(_lib.PATH_TAIL)
PDIFF_TOL = 4.5e-5  # tests/path_ref.py: the path judge's measured pdiff error against float64
UNANSWERED = U32(_lib.GATHER_NOT_GATHERED | _lib.GATHER_NO_PROBE)


def turned_normal(SN, direction, T=F):
    """step 1: the shading normal, turned toward the ray; the dot's products and sums each rounded, in x, y, z order"""
    SN, d = np.asarray(SN, T), np.asarray(direction, T)
    with np.errstate(all="ignore"):
        sd = ((SN[:, 0] * d[:, 0]).astype(T) + (SN[:, 1] * d[:, 1]).astype(T)).astype(T) + (SN[:, 2] * d[:, 2]).astype(T)
    return np.where((sd.astype(T) <= 0)[:, None], SN, -SN).astype(T)


def points(surface, direction):
    """the gather's points of the hits in `surface` (shade_rays("surface") records of rays with `direction`): float32 [n, 8]"""
    out = np.zeros((len(surface), 8), F)
    out[:, 0:3] = surface["position"]
    out[:, 4:7] = turned_normal(surface["shading_normal"], direction)
    return out


def _tail(vertex, surface, E, pd, T):
    thr, added = vertex["throughput"].astype(T), vertex["added"].astype(T)
    albedo, metal = surface["albedo"].astype(T), surface["metalness"].astype(T)
    with np.errstate(all="ignore"):
        k = (thr * (albedo * (T(1) - metal).astype(T)[:, None]).astype(T)).astype(T)  # step 4
        if pd is not None:  # step 5
            pd = np.asarray(pd, T)
            factor = np.where(pd > 0, (T(2) - pd).astype(T), T(1)).astype(T)
            k = (k * factor[:, None]).astype(T)
        inv = PI_INV if T is F else 1.0 / float(F(3.14159265))
        tail = ((k * np.asarray(E, T)).astype(T) * T(inv)).astype(T)  # step 6
        return tail, (added + tail).astype(T)  # step 7


def tail32(vertex, surface, E, pd=None):
    """`vertex`: the terminal vertex records WITHOUT a tail (the plain call's: throughput on entering, the direct `added`); `surface`:
    the shade_rays("surface") records of those vertices' rays; E: the gathered irradiance [n, 3]; pd: the recorded pdiff under
    NEB_TAIL_FRAME_WEIGHT, None without it -> (tail [n, 3], the new added [n, 3]), float32, one rounding per operation"""
    return _tail(vertex, surface, E, pd, F)


def tail64(vertex, surface, E, pd=None):
    return _tail(vertex, surface, E, pd, F64)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1) if a.size else np.zeros((len(a), 0), np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def judge(plain, got, K, frame_weight, shade, gather, what, pd64=None):
    """plain, got: (neb_ray_path [n], neb_path_vertex [n, K - 1]) of the plain call and of the tail call over the same rays and constants.
    shade(rays) -> shade_rays("surface") records; gather(points) -> neb_probe_gather records; pd64(rays, surface) -> float64 pdiff or
    None.  Raises AssertionError naming the check; -> dict(flagged, candidates, pdiff error)."""
    (p_out, p_vert), (g_out, g_vert) = plain, got
    n, last = len(p_out), K - 1
    p_vert, g_vert = p_vert.reshape(n, last), g_vert.reshape(n, last)
    # every vertex before the terminal one: the plain call's bits
    if last > 1:
        assert _same(g_vert[:, :last - 1].reshape(-1), p_vert[:, :last - 1].reshape(-1)), f"{what}: a vertex record before the terminal vertex differs from the plain call's"
    tp, tg = p_vert[:, last - 1], g_vert[:, last - 1]
    live = p_out["segments"] == last
    candidate = live & ((tp["flags"] & _lib.HIT_MATERIAL) != 0)
    rays = np.column_stack([tp["origin"], tp["tmin"], tp["direction"], tp["tmax"]]).astype(F)
    surface = shade(rays)
    pts = points(surface, tp["direction"])
    g = gather(pts)
    answered = candidate & ((g["flags"] & UNANSWERED) == 0)
    # the flags follow the rule
    assert np.array_equal((g_out["flags"] & TAIL) != 0, answered), f"{what}: path flags: NEB_PATH_TAIL is not (k == last, MATERIAL, the gather answered)"
    assert np.array_equal((tg["flags"] & TAIL) != 0, answered), f"{what}: vertex flags: NEB_PATH_TAIL is not (k == last, MATERIAL, the gather answered)"
    assert _same(g_out["flags"] & ~TAIL, p_out["flags"]) and _same(tg["flags"] & ~TAIL, tp["flags"]), f"{what}: a flag other than NEB_PATH_TAIL changed"
    # a path without the flag: the plain call's bits
    assert _same(g_out[~answered], p_out[~answered]) and _same(tg[~answered], tp[~answered]), f"{what}: a path without NEB_PATH_TAIL differs from the plain call's"
    # a flagged vertex
    a = answered
    for f in ("origin", "tmin", "direction", "t", "throughput", "rng", "geometry", "primitive", "u", "v", "tmax", "reserved"):
        assert _same(tg[f][a], tp[f][a]), f"{what}: {f} of a flagged vertex differs from the plain call's"
    pd = tg["pdiff"][a] if frame_weight else None
    if not frame_weight:
        assert not tg["pdiff"][a].view(U32).any(), f"{what}: pdiff recorded without NEB_TAIL_FRAME_WEIGHT"
    want = tail32(tp[a], surface[a], g["irradiance"][a], pd)[1]
    if not _same(tg["added"][a], want):
        bad = np.flatnonzero((tg["added"][a].view(U32) != want.view(U32)).any(-1))
        raise AssertionError(f"{what}: added != tail32 at {len(bad)} of {int(a.sum())} flagged vertices; first: ray {np.flatnonzero(a)[bad[0]]}: "
                             f"{tg['added'][a][bad[0]]} != {want[bad[0]]} (direct {tp['added'][a][bad[0]]}, E {g['irradiance'][a][bad[0]]})")
    worst = 0.0
    if frame_weight and pd64 is not None and a.any():
        worst = float(np.abs(tg["pdiff"][a].astype(F64) - pd64(rays[a], surface[a])).max())
        assert worst <= PDIFF_TOL, f"{what}: pdiff is {worst:.3e} from float64 (tolerance {PDIFF_TOL:.1e})"
    # out.rgb is the float32 running sum of the added words; everything else of the path record is the plain call's
    assert _same(g_out["radiance"], P.running_sum(g_vert, g_out["segments"].astype(np.int64))), f"{what}: out.rgb is not the float32 running sum of `added`"
    for f in ("t", "geometry", "primitive", "segments"):
        assert _same(g_out[f], p_out[f]), f"{what}: {f} of a path record differs from the plain call's"
    return dict(flagged=int(a.sum()), candidates=int(candidate.sum()), pdiff=worst, answered=answered, surface=surface, gather=g)
