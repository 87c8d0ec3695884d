"""The float32 restatement of neb_gi_trace_paths and the judge of its records, vertex by vertex.
TEST INFRASTRUCTURE, NOT PRODUCT CODE.  tests/test_path_cpu.py shows on the CPU that the judge is right and able to fail and measures
what its tolerances are derived from; tests/test_path_gpu.py judges the device with it.

trace32 is the bounce loop of oracle/gi_np.trace (lines 343-397; pathtracer.hlsl:495-621) started from a ray, not from a G-buffer
pixel: float32 with gi_np's functions, every intersection decided by the float64 caster on the float32 rays (as every float32 ray of
these tests is).  It returns the records the device returns.

judge_vertices is LOCAL PER VERTEX.  A path forks at every discrete outcome -- which triangle, lit or not, divided or not -- so no
reference path can be followed beside the device's; instead every discrete fact is taken from the records themselves or from the
library's own existing queries (`cast`: cast_rays, `shade`: shade_rays("surface")), and what is continuous is compared with float64
(ray_shade_ref.reconstruct on the triangle the record names) from the record's own inputs: the recorded throughput, the recorded
pdiff, the recorded decision.  On the CPU the two callables are float64 / float32 stand-ins (cpu_cast, cpu_shade).

Error classes: `added`, `origin`, `throughput` relative to max(1, |x|); `direction`, `pdiff` absolute.  The tolerances are not picked by
hand: each is FOUR TIMES the largest error of trace32's records under the judge, measured by test_path_cpu.test_calibration over the
states, sets and K = 8 the GPU tests use (the rule ray_shade_ref documents).  The test prints the measured values on every run and
holds the constants to them."""
import numpy as np

import ray_query_ref as Q
import ray_shade_ref as R
from motion_ref import NO_SUBMESH
from nebulae_amd import _lib
from oracle import gi_np
from test_refit_gpu import TIE_CAP  # noqa: F401

F, U32 = np.float32, np.uint32
PATH = np.dtype([("radiance", F, (3,)), ("t", F), ("geometry", U32), ("primitive", U32), ("flags", U32), ("segments", U32)])
VERTEX = np.dtype([("origin", F, (3,)), ("tmin", F), ("direction", F, (3,)), ("t", F), ("throughput", F, (3,)), ("rng", U32), ("added", F, (3,)),
                   ("flags", U32), ("geometry", U32), ("primitive", U32), ("u", F), ("v", F), ("tmax", F), ("pdiff", F), ("reserved", U32, (2,))])
assert PATH.itemsize == 32 and VERTEX.itemsize == 96
CLASSES = ("added", "origin", "throughput", "direction", "pdiff")
# trace32 against float64 under the judge, test_path_cpu.test_calibration: the maxima over the four states, the sets scattered / outside /
# second, K = 8, rounded up from added 6.156e-05, origin 5.401e-05, throughput 1.055e-04, direction 1.834e-04, pdiff 4.420e-05
MEASURED = dict(added=6.2e-5, origin=5.5e-5, throughput=1.06e-4, direction=1.84e-4, pdiff=4.5e-5)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
JUDGED_SETS = ("scattered", "outside", "second")
HIT_BITS = U32(0x3F)
T_MIN, T_MAX = F(0.001), F(R.TRACE_MAX)


def constants(K, frame_index=3, tan_half=None):
    c = R.constants(frame_index=frame_index, tan_half=tan_half)
    c.maxPathVertices = K
    return c


def seeds(n, frame_index):
    return gi_np.jenkins_hash(np.arange(n, dtype=U32) ^ gi_np.jenkins_hash(np.array([frame_index], U32)))


def draws(rng, count):
    """`count` Rand() of each stream -> (the draws [count, n] float32, the streams after them); `rng` is not changed"""
    state = np.array(rng, U32)
    out = [gi_np.rand(state) for _ in range(count)]
    return (np.stack(out) if out else np.zeros((0, len(state)), F)), state


def shadow_rays(hitP, GN, c, dtype, a0, a1):
    """ray_shade_ref.shadow_rays with the two disk draws as an argument"""
    n = len(hitP)
    L, B, T = R.sun_frame(c, dtype)
    if dtype == F:
        angle, dist = a0 * F(2.0) * F(3.1415926535), np.sqrt(a1, dtype=F)
        inc = gi_np.normalize((L + (B * np.sin(angle, dtype=F)[:, None] + T * np.cos(angle, dtype=F)[:, None]) * F(c.sunTanHalfAngle) * dist[:, None]).astype(F))
        transition = gi_np.dot(GN, inc) <= 0
    else:
        angle, dist = a0.astype(dtype) * 2.0 * 3.1415926535, np.sqrt(a1.astype(dtype))
        inc = R._unit(L + (B * np.sin(angle)[:, None] + T * np.cos(angle)[:, None]) * float(F(c.sunTanHalfAngle)) * dist[:, None])
        transition = np.sum(GN * inc, -1) <= 0
    so = (hitP + np.where(transition[:, None], -GN, GN) * dtype(1e-2)).astype(dtype)
    rays = np.zeros((n, 8), dtype)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = so, 0.001, inc, R.TRACE_MAX
    return rays


# ------------------------------------------------------------------------------------------------
# the CPU stand-ins of the library's two queries
# ------------------------------------------------------------------------------------------------
def cpu_cast(tris):
    """cast_rays: the triangle by the float64 caster on the float32 rays, t / u / v by float32 Moeller-Trumbore on that triangle"""
    def cast(rays, any_hit=False):
        rays = np.asarray(rays, F)
        n = len(rays)
        ok = R._walkable(rays)
        geometry, primitive = np.full(n, NO_SUBMESH, U32), np.full(n, NO_SUBMESH, U32)
        if ok.any():
            ref = Q.reference(tris, rays[ok])
            geometry[ok], primitive[ok] = ref["geometry"], ref["primitive"]
        found = geometry != NO_SUBMESH
        if any_hit:
            return found.astype(U32)
        idx = Q.triangle_index(tris, geometry, primitive)
        t, u, v = Q.moller_trumbore(tris, np.maximum(idx, 0), rays, F)
        return dict(t=np.where(found, t, F(np.inf)).astype(F), u=np.where(found, u, 0).astype(F), v=np.where(found, v, 0).astype(F), geometry=geometry,
                    primitive=primitive)
    return cast


def _attributes(sc, geometry):
    has = np.array([all(g[k] is not None for k in ("positions", "normals", "uvs", "tangents")) for g in sc.geometries] + [False])
    return has[np.minimum(np.asarray(geometry).astype(np.int64), len(sc.geometries))]


def cpu_shade(sc, tris, flat=None):
    """shade_rays("surface"): ray_shade_ref.reading32 on cpu_cast's triangles, as neb_ray_surface records (position, normals, the
    material's fields, t / u / v / ids and flags; texcoord and material are left 0)."""
    cast = cpu_cast(tris)
    flat = flat or gi_np.FlatScene(sc)

    def shade(rays):
        rays = np.asarray(rays, F)
        hit = cast(rays)
        rd = R.reading32(sc, tris, rays, hit["geometry"], hit["primitive"], flat=flat)
        rec = np.zeros(len(rays), R.SURFACE)
        found, att = rd["found"], _attributes(sc, hit["geometry"])
        rec["position"], rec["t"], rec["u"], rec["v"] = rd["position"], hit["t"], hit["u"], hit["v"]
        rec["geometry"], rec["primitive"] = hit["geometry"], hit["primitive"]
        rec["geometric_normal"] = np.where(att[:, None], rd["GN"], F(0))
        rec["shading_normal"] = np.where(rd["shaded"][:, None], rd["SN"], rec["geometric_normal"])
        rec["albedo"], rec["roughness"], rec["metalness"] = rd["albedo"], rd["roughness"], rd["metalness"]
        with np.errstate(all="ignore"):
            back = att & (gi_np.dot(rec["geometric_normal"], rays[:, 4:7]) > 0)
        rec["flags"] = (found * _lib.HIT_FOUND | att * _lib.HIT_ATTRIBUTES | rd["shaded"] * _lib.HIT_MATERIAL | back * _lib.HIT_BACKFACE
                        | ~R._walkable(rays) * _lib.HIT_NOT_WALKED).astype(U32)
        return rec
    return shade


# ------------------------------------------------------------------------------------------------
# trace32
# ------------------------------------------------------------------------------------------------
def trace32(sc, tris, rays, c, flat=None):
    """the loop of gi_np.trace:343-397 along `rays` -> (neb_ray_path [n], neb_path_vertex [n, K - 1])"""
    rays = np.asarray(rays, F)
    n, K = len(rays), int(c.maxPathVertices)
    out, vert = np.zeros(n, PATH), np.zeros((n, K - 1), VERTEX)
    cast, shade = cpu_cast(tris), cpu_shade(sc, tris, flat)
    sky, sun_rad = np.array(list(c.skyColor), F), np.array(list(c.sunLightRadiance), F)
    L = R.sun_frame(c, F)[0]
    rng, throughput, total = seeds(n, int(c.frameIndex)), np.ones((n, 3), F), np.zeros((n, 3), F)
    cur = rays.copy()
    alive = R._walkable(rays)
    out["t"], out["geometry"], out["primitive"], out["flags"] = np.inf, NO_SUBMESH, NO_SUBMESH, np.where(alive, 0, _lib.HIT_NOT_WALKED)
    for k in range(1, K):
        ids = np.flatnonzero(alive)
        if not len(ids):
            break
        r = cur[ids]
        surf = shade(r)
        found, shaded = surf["geometry"] != NO_SUBMESH, (surf["flags"] & _lib.HIT_MATERIAL) != 0
        flags = surf["flags"].copy()
        v = np.zeros(len(ids), VERTEX)
        v["origin"], v["tmin"], v["direction"], v["tmax"] = r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7]
        v["t"], v["u"], v["v"], v["geometry"], v["primitive"] = surf["t"], surf["u"], surf["v"], surf["geometry"], surf["primitive"]
        v["throughput"], v["rng"] = throughput[ids], rng[ids]
        (a0, a1), after = draws(rng[ids], 2)
        sh = shadow_rays(surf["position"], surf["geometric_normal"], c, F, a0, a1)
        sh[~shaded, 4:7] = 0.0
        visible = shaded & (cast(sh, any_hit=True) == 0)
        V = gi_np.normalize(-r[:, 4:7])
        with np.errstate(all="ignore"):
            brdf = gi_np.evaluate_direct_brdf(surf["albedo"], surf["roughness"], surf["metalness"], surf["shading_normal"], V, np.broadcast_to(L, (len(ids), 3)))
            lit = (((brdf * sun_rad).astype(F)) * throughput[ids]).astype(F)
            added = np.where(visible[:, None], lit, F(0))
            added = np.where(found[:, None], added, (sky * throughput[ids]).astype(F)).astype(F)
        flags |= (visible * _lib.HIT_SUN_VISIBLE).astype(U32)
        rng[ids] = np.where(shaded, after, rng[ids])
        if k == 1:
            out["t"][ids], out["geometry"][ids], out["primitive"][ids] = surf["t"], surf["geometry"], surf["primitive"]
            out["flags"][ids] |= flags
            total[ids] = added
        else:
            total[ids] = (total[ids] + added).astype(F)
        out["flags"][ids[~found]] |= _lib.PATH_ESCAPED
        out["segments"][ids] += 1
        bounce = shaded & (k + 1 < K)
        if bounce.any():
            b = np.flatnonzero(bounce)
            with np.errstate(all="ignore"):
                SNn = gi_np.normalize(surf["shading_normal"][b])
                (e0, e1), _ = draws(rng[ids[b]], 2)
                Ld = gi_np.cosine_sample_hemisphere_surface_aligned(e0, e1, SNn)
                pdiff = F(1.0) - gi_np.specular_probability(gi_np.saturate(gi_np.dot(V[b], SNn)), gi_np.specular_f0(surf["albedo"][b], surf["metalness"][b]),
                                                            surf["albedo"][b])
                cur[ids[b], 0:3] = (surf["position"][b] + surf["geometric_normal"][b] * F(1e-2)).astype(F)
                cur[ids[b], 3], cur[ids[b], 4:7], cur[ids[b], 7] = T_MIN, Ld, T_MAX
                tp = (throughput[ids[b]] * gi_np.diffuse_reflectance(surf["albedo"][b], surf["metalness"][b])).astype(F)
                (third,), after3 = draws(rng[ids[b]], 1)
                take = third < pdiff
                tp[take] = (tp[take] / pdiff[take, None]).astype(F)
            rng[ids[b]], throughput[ids[b]] = after3, tp
            v["pdiff"][b] = pdiff
            flags[b] |= (take * _lib.PATH_DIVIDED).astype(U32)
        v["added"], v["flags"] = added, flags
        vert[ids, k - 1] = v
        alive[:] = False
        alive[ids[bounce]] = True
    out["radiance"] = total
    return out, vert


# ------------------------------------------------------------------------------------------------
# float64 pieces of the next bounce (brdf.hlsli:129-143, :166-185)
# ------------------------------------------------------------------------------------------------
def _specular_probability64(vdotn, f0, albedo):
    lum = lambda x: x[:, 0] * float(F(0.2126)) + x[:, 1] * float(F(0.7152)) + x[:, 2] * float(F(0.0722))  # noqa: E731
    k = 1.0 - np.clip(vdotn, 0.0, 1.0) ** 5
    fres = np.clip(lum(f0 + (1.0 - f0) * k[:, None]), 0.0, 1.0)
    diff = lum(albedo) * (1.0 - fres)
    return np.clip(diff / np.maximum(float(F(0.0001)), fres + diff), float(F(0.1)), float(F(0.9)))


def _hemisphere64(u0, u1, sn, up_is_z):
    a, b = np.sqrt(u0.astype(np.float64)), float(gi_np.PI_TWO) * u1.astype(np.float64)
    z = np.stack([a * np.cos(b), a * np.sin(b), np.sqrt(1.0 - u0.astype(np.float64))], -1)
    up = np.where(up_is_z[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    tx = R._unit(np.cross(up, sn))
    ty = np.cross(sn, tx)
    return R._unit(z[:, 0:1] * tx + z[:, 1:2] * ty + z[:, 2:3] * sn)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1) if a.size else np.zeros((len(a), 0), np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def running_sum(vert, segments):
    """the float32 sum of the `added` words: assigned at vertex 1, then added in order, over the path's own records"""
    total = np.zeros((len(vert), 3), F)
    with np.errstate(all="ignore"):
        for k in range(vert.shape[1]):
            m = segments > k
            total[m] = vert["added"][m, k] if k == 0 else (total[m] + vert["added"][m, k]).astype(F)
    return total


# ------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------
def judge_vertices(sc, tris, rays, c, out, vertices, cast, shade, what, cap=TIE_CAP):
    """neb_ray_path [n] and neb_path_vertex [n, K - 1] records of `rays` under constants `c` -> dict(the largest error of each class,
    differ: shadow outcomes that differ per level, live: records per level).  Raises AssertionError naming the check that failed."""
    rays = np.asarray(rays, F)
    n, S = len(rays), int(c.maxPathVertices) - 1
    vertices = np.asarray(vertices).reshape(n, S)
    seg = out["segments"].astype(np.int64)
    sky, sun = np.array(list(c.skyColor), F), np.array(list(c.sunLightRadiance), F).astype(np.float64)
    L64 = R.sun_frame(c, np.float64)[0]
    live = seg[:, None] > np.arange(S)[None, :]
    vflags = vertices["flags"]
    found, shaded = (vflags & _lib.HIT_FOUND) != 0, (vflags & _lib.HIT_MATERIAL) != 0
    miss = live & ~found
    # ---- 1: chain integrity, exact bits ----
    assert (seg <= S).all(), f"{what}: segments above maxPathVertices - 1"
    assert not _bits(vertices.reshape(-1))[~live.reshape(-1)].any(), f"{what}: chain: a record past the path's end is not zero"
    assert not vertices["reserved"].any() and not (vflags & ~(HIT_BITS | U32(_lib.PATH_DIVIDED))).any(), f"{what}: chain: reserved words or unknown vertex flags"
    walkable = R._walkable(rays)
    assert np.array_equal(seg == 0, ~walkable) and np.array_equal((out["flags"] & _lib.HIT_NOT_WALKED) != 0, ~walkable), f"{what}: chain: NOT_WALKED / segments 0"
    first = vertices[:, 0]
    w = walkable
    assert _same(np.column_stack([first["origin"], first["tmin"], first["direction"], first["tmax"]])[w], rays[w]), f"{what}: chain: record 1 is not the caller's ray"
    assert _same(first["rng"][w], seeds(n, int(c.frameIndex))[w]) and _same(first["throughput"][w], np.ones((int(w.sum()), 3), F)), f"{what}: chain: the path's seed or first throughput"
    later = live[:, 1:]
    assert (vertices["tmin"][:, 1:][later].view(U32) == T_MIN.view(U32)).all() and (vertices["tmax"][:, 1:][later].view(U32) == T_MAX.view(U32)).all(), \
        f"{what}: chain: a later segment's interval is not (0.001, 10000)"
    assert np.isposinf(vertices["t"][miss]).all() and (vertices["geometry"][miss] == NO_SUBMESH).all() and (vertices["primitive"][miss] == NO_SUBMESH).all(), \
        f"{what}: chain: a missed segment's t or ids"
    assert np.isfinite(vertices["t"][live & found]).all(), f"{what}: chain: a hit without a distance"
    goes_on = np.zeros_like(live)
    goes_on[:, :-1] = live[:, 1:]
    assert np.array_equal(goes_on, live & shaded & (np.arange(S)[None, :] + 1 < S)), f"{what}: chain: a path goes on exactly from a shaded vertex that is not the last"
    for k in range(S - 1):
        m = goes_on[:, k]
        (a0, a1, third), after = draws(vertices["rng"][m, k], 3)
        assert _same(vertices["rng"][m, k + 1], after), f"{what}: chain: rng of record {k + 2} is not rng of record {k + 1} advanced by three draws"
        pd = vertices["pdiff"][m, k]
        assert np.array_equal((vflags[m, k] & _lib.PATH_DIVIDED) != 0, third < pd), f"{what}: chain: NEB_PATH_DIVIDED is not (third draw < pdiff) at vertex {k + 1}"
    assert not vertices["pdiff"][~goes_on].view(U32).any() and not (vflags[~goes_on] & _lib.PATH_DIVIDED).any(), f"{what}: chain: pdiff or DIVIDED where no bounce is sampled"
    assert np.array_equal((out["flags"] & _lib.PATH_ESCAPED) != 0, miss.any(-1)), f"{what}: chain: NEB_PATH_ESCAPED"
    assert not (out["flags"] & ~(HIT_BITS | U32(_lib.PATH_ESCAPED))).any(), f"{what}: chain: unknown flags"
    assert _same(out["t"][w], first["t"][w]) and _same(out["geometry"][w], first["geometry"][w]) and _same(out["primitive"][w], first["primitive"][w]) \
        and _same((out["flags"] & HIT_BITS)[w], (first["flags"] & HIT_BITS)[w]), f"{what}: chain: the first hit of `out` is not record 1's"
    blank = out[~w]
    assert np.isposinf(blank["t"]).all() and (blank["geometry"] == NO_SUBMESH).all() and (blank["primitive"] == NO_SUBMESH).all() \
        and (blank["flags"] == _lib.HIT_NOT_WALKED).all() and not blank["radiance"].view(U32).any(), f"{what}: chain: the record of a ray that was not walked"
    # ---- 3: local arithmetic against float64, 2: hits, 4: shadow outcomes -- per level ----
    err = {k: 0.0 for k in CLASSES}
    differ = []

    def worst(name, e, mask=None):
        e = np.where(np.isnan(e), np.inf, e).reshape(len(e), -1).max(-1)
        if mask is not None:
            e = e[mask]
        err[name] = max(err[name], float(e.max(initial=0.0)))

    for k in range(S):
        ids = np.flatnonzero(live[:, k])
        if not len(ids):
            differ.append(0)
            continue
        v = vertices[ids, k]
        r = np.column_stack([v["origin"], v["tmin"], v["direction"], v["tmax"]]).astype(F)
        fl = v["flags"]
        f_, sh_ = found[ids, k], shaded[ids, k]
        visible = (fl & _lib.HIT_SUN_VISIBLE) != 0
        ref = R.reading64(sc, tris, r, np.where(f_, v["geometry"], NO_SUBMESH), v["primitive"])
        assert np.array_equal(sh_, ref["shaded"]) and np.array_equal((fl & _lib.HIT_ATTRIBUTES) != 0, ref["attributes"]), f"{what}: vertex {k + 1}: ATTRIBUTES / MATERIAL"
        assert not visible[~sh_].any(), f"{what}: vertex {k + 1}: SUN_VISIBLE without MATERIAL"
        surf = shade(r)
        thr = v["throughput"].astype(np.float64)
        d64 = r[:, 4:7].astype(np.float64)
        V64 = R._unit(-d64)
        with np.errstate(all="ignore"):
            brdf = R.direct_brdf(ref["albedo"], ref["roughness"], ref["metalness"], ref["SN"], V64, np.broadcast_to(L64, (len(ids), 3)))
            want = brdf * sun * thr
            lit = sh_ & visible
            worst("added", np.abs(v["added"].astype(np.float64) - want) / np.maximum(1.0, np.abs(want)), lit)
            assert _same(v["added"][~f_], (sky * v["throughput"][~f_]).astype(F)), f"{what}: vertex {k + 1}: added: a miss does not add sky * throughput"
        assert not v["added"][f_ & ~lit].view(U32).any(), f"{what}: vertex {k + 1}: added: light where nothing is lit"
        if k + 1 < S:
            m = goes_on[ids, k]
            nxt = vertices[ids[m], k + 1]
            (e0, e1), _ = draws(draws(v["rng"][m], 2)[1], 2)
            SN64 = R._unit(ref["SN"][m])
            up_is_z = np.abs(gi_np.normalize(surf["shading_normal"][m])[:, 2]) < F(0.999)  # (a discrete choice: the library's own normal makes it)
            with np.errstate(all="ignore"):
                want_o = ref["position"][m] + ref["GN"][m] * 1e-2
                worst("origin", np.abs(nxt["origin"].astype(np.float64) - want_o) / np.maximum(1.0, np.abs(want_o)))
                worst("direction", np.abs(nxt["direction"].astype(np.float64) - _hemisphere64(e0, e1, SN64, up_is_z)))
                f0 = 0.04 + ref["metalness"][m, None] * (ref["albedo"][m] - 0.04)
                worst("pdiff", np.abs(v["pdiff"][m].astype(np.float64) - (1.0 - _specular_probability64(np.sum(V64[m] * SN64, -1), f0, ref["albedo"][m]))))
                want_t = thr[m] * (ref["albedo"][m] * (1.0 - ref["metalness"][m, None]))
                divided = (fl[m] & _lib.PATH_DIVIDED) != 0
                want_t = np.where(divided[:, None], want_t / v["pdiff"][m].astype(np.float64)[:, None], want_t)
                worst("throughput", np.abs(nxt["throughput"].astype(np.float64) - want_t) / np.maximum(1.0, np.abs(want_t)))
        for name in CLASSES:
            assert err[name] <= TOL[name], f"{what}: vertex {k + 1}: {name} off by {err[name]:.3e}, tolerance {TOL[name]:.1e}"
        hits = cast(r)
        for key in ("t", "u", "v", "geometry", "primitive"):
            assert _same(v[key], np.asarray(hits[key])), f"{what}: vertex {k + 1}: hits: {key} is not what cast_rays answers for the record's ray"
        assert np.array_equal((surf["flags"] & _lib.HIT_MATERIAL) != 0, sh_), f"{what}: vertex {k + 1}: MATERIAL is not shade_rays'"
        (a0, a1), _ = draws(v["rng"], 2)
        sray = shadow_rays(surf["position"], surf["geometric_normal"], c, F, a0, a1)
        sray[~sh_, 4:7] = 0.0
        occluded = np.asarray(cast(sray, any_hit=True)) != 0
        differ.append(int((sh_ & (visible == occluded)).sum()))
        assert differ[-1] <= cap, f"{what}: vertex {k + 1}: shadow: {differ[-1]} outcomes differ from cast_rays(any_hit) on the rebuilt shadow rays"
    # ---- 5: the sum, exact ----
    assert _same(out["radiance"], running_sum(vertices, seg)), f"{what}: sum: out.rgb is not the float32 running sum of the added words"
    counts = live.sum(0).tolist()
    print(f"[{what}] " + ", ".join(f"{k} {err[k]:.2e} / {TOL[k]:.1e}" for k in CLASSES) + f"; records per level {counts}, shadow outcomes that differ {differ}, "
          f"{int(miss.any(-1).sum())} escaped, mean segments {float(seg.mean()):.2f}")
    return dict(err, differ=differ, live=counts)
