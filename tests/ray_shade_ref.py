"""The float64 reference of neb_gi_shade_rays and the judges of its two records.
TEST INFRASTRUCTURE, NOT PRODUCT CODE.  tests/test_ray_shade_cpu.py shows on the CPU that the judges are right and able to fail and
measures what their tolerances are derived from; tests/test_ray_shade_gpu.py judges the device with them.

The reference is a float64 restatement of oracle/gi_np.py's FlatScene.reconstruct and evaluate_direct_brdf (the same text of the
reference's shaders, pathtracer.hlsl:299-395 and :209-228) and of the sun-disk shadow ray of :546-557.  It is evaluated ON THE
TRIANGLE THE DEVICE NAMES, at the float64 barycentrics of the float32 ray on that triangle (ray_query_ref.moller_trumbore): an answer
on a coincident triangle is judged on its own triangle, and whether the triangle itself is right is ray_query_ref.judge's business.

Errors: absolute for normals, albedo, roughness, metalness and texcoord; relative to max(1, |x|) for position and for radiance.
Radiance is compared where the device's shadow outcome (NEB_HIT_SUN_VISIBLE) agrees with float64's; outcomes that disagree are
capped at TIE_CAP per set.

The tolerances are not picked by hand: each is FOUR TIMES the largest error of the float32 reading -- float32 Moeller-Trumbore on
the same triangle, gi_np.FlatScene.reconstruct and gi_np.evaluate_direct_brdf -- against the float64 restatement, measured by
test_ray_shade_cpu.test_calibration over every state and set the GPU tests use; four times, the margin ray_query_ref gives the
device for its different order of operations.  The test prints the measured values on every run and holds the constants to them."""
import numpy as np

import ray_query_ref as Q
import views_ref as V
from motion_ref import NO_SUBMESH
from nebulae_amd import _lib
from nebulae_amd import scene as S
from oracle import gi_np
from test_refit_gpu import TIE_CAP, clone  # noqa: F401

F, U32 = np.float32, np.uint32
SURFACE = np.dtype([("position", F, (3,)), ("t", F), ("geometric_normal", F, (3,)), ("geometry", U32), ("shading_normal", F, (3,)), ("primitive", U32),
                    ("albedo", F, (3,)), ("roughness", F), ("metalness", F), ("texcoord", F, (2,)), ("material", np.int32), ("u", F), ("v", F),
                    ("flags", U32), ("reserved", U32)])
RADIANCE = np.dtype([("radiance", F, (3,)), ("t", F), ("geometry", U32), ("primitive", U32), ("flags", U32), ("reserved", U32)])
assert SURFACE.itemsize == 96 and RADIANCE.itemsize == 32
FIELDS = ("position", "normal", "albedo", "rm", "texcoord", "radiance")
# float32 against float64, test_ray_shade_cpu.test_calibration: the maxima over the four states, the five sets and both suns, rounded up
# from position 5.401e-5, normal 4.625e-5, albedo 8.775e-5, roughness / metalness 2.061e-5, texcoord 6.164e-5, radiance 1.669e-4.  (They
# are errors of the barycentrics for the most part: ray_query_ref measures u and v off by 4.0e-5 and 6.2e-5 on these sets.)
MEASURED = dict(position=5.5e-5, normal=4.7e-5, albedo=8.8e-5, rm=2.1e-5, texcoord=6.2e-5, radiance=1.7e-4)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
BACKFACE_SKIP = 1e-4
TRACE_MAX = 10000.0
NO_MATERIAL, NO_TANGENTS = "no material", "no tangents"


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def room_with_extras():
    """the beamed room plus two boxes that float above the floor: one without a material, one without its tangent stream
    -> (scene, {NO_MATERIAL: geometry index, NO_TANGENTS: geometry index})"""
    sc = clone(V.beamed_room())
    first = len(sc.geometries)
    white = sc.geometries[0]["material"]
    sc.add_geometry(*S._box((-0.6, -0.9, -0.5), (-0.3, -0.6, -0.2)), material=-1)
    sc.add_geometry(*S._box((0.3, -0.9, -0.6), (0.6, -0.5, -0.3)), material=white, omit=("tangents",))
    return sc, {NO_MATERIAL: first, NO_TANGENTS: first + 1}


def states():
    """ray_query_ref.states() plus the room with the two extra geometries -> {name: (scene, hidden submeshes)}"""
    out = dict(Q.states())
    out["room, extras"] = (room_with_extras()[0], ())
    return out


def constants(frame_index=1, tan_half=None):
    c = S.default_constants(frame_index=frame_index)
    if tan_half is not None:
        c.sunTanHalfAngle = tan_half
    return c


# ------------------------------------------------------------------------------------------------
# float64: ReconstructSurfaceData, EvaluateDirectBRDF, the sun-disk shadow ray
# ------------------------------------------------------------------------------------------------
def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(np.sum(v * v, -1, keepdims=True))


def _sample(img, uv):
    """SampleLevel(linear, wrap, mip 0) of an R8G8B8A8_UNORM image (gi_np.FlatScene.sample), float64"""
    h, w = img.shape[:2]
    x, y = uv[:, 0] * w - 0.5, uv[:, 1] * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xi, yi = x0.astype(np.int64) % w, y0.astype(np.int64) % h
    x1, y1 = (xi + 1) % w, (yi + 1) % h
    tex = img.astype(np.float64) / 255.0
    top = tex[yi, xi] + fx * (tex[yi, x1] - tex[yi, xi])
    bot = tex[y1, xi] + fx * (tex[y1, x1] - tex[y1, xi])
    return top + fy * (bot - top)


def reconstruct(sc, geometry, primitive, bu, bv):
    """ReconstructSurfaceData for hits on (geometry[k], primitive[k]) at barycentrics (bu, bv), float64 -> dict(GN, SN, albedo,
    roughness, metalness, texcoord, material int, attributes bool, shaded bool); what a flag leaves undefined is 0 (material: -1)"""
    n = len(geometry)
    out = dict(GN=np.zeros((n, 3)), SN=np.zeros((n, 3)), albedo=np.zeros((n, 3)), roughness=np.zeros(n), metalness=np.zeros(n),
               texcoord=np.zeros((n, 2)), material=np.full(n, -1, np.int64), attributes=np.zeros(n, bool), shaded=np.zeros(n, bool))
    b1, b2 = np.asarray(bu, np.float64), np.asarray(bv, np.float64)
    b0 = 1.0 - (b1 + b2)
    for gi in np.unique(geometry):
        if gi == NO_SUBMESH:
            continue
        g = sc.geometries[int(gi)]
        m = geometry == gi
        if any(g[k] is None for k in ("positions", "normals", "uvs", "tangents")):
            continue  # :313-318
        idx = g["indices"].reshape(-1, 3).astype(np.int64)[primitive[m].astype(np.int64)]
        w0, w1, w2 = b0[m, None], b1[m, None], b2[m, None]
        nrm = g["normals"].astype(np.float64)
        gn = _unit(nrm[idx[:, 0]] * w0 + nrm[idx[:, 1]] * w1 + nrm[idx[:, 2]] * w2)
        gn = _unit(gn @ g["M"].astype(np.float64)[:3, :3])  # mul(float4(GN, 0), surfaceToWorld)
        uvs = g["uvs"].astype(np.float64)
        uv = uvs[idx[:, 0]] * w0 + uvs[idx[:, 1]] * w1 + uvs[idx[:, 2]] * w2
        out["GN"][m], out["SN"][m], out["texcoord"][m], out["attributes"][m] = gn, gn, uv, True
        if g["material"] < 0:
            continue  # :349
        mat = sc.materials[g["material"]]
        ta, tn, tr = mat["textures"]
        out["albedo"][m] = np.array(mat["albedo"][:3], F).astype(np.float64) if ta < 0 else _sample(sc.textures[ta], uv)[:, :3]
        if tn >= 0:
            tg = g["tangents"].astype(np.float64)
            t4 = tg[idx[:, 0]] * w0 + tg[idx[:, 1]] * w1 + tg[idx[:, 2]] * w2
            t4 = t4 / np.sqrt(np.sum(t4 * t4, -1, keepdims=True))  # normalize(float4)
            bt = _unit(np.cross(gn, t4[:, :3]) * t4[:, 3:4])
            N = _sample(sc.textures[tn], uv)[:, :3] * 2.0 - 1.0
            out["SN"][m] = _unit(N[:, 0:1] * t4[:, :3] + N[:, 1:2] * bt + N[:, 2:3] * gn)
        if tr < 0:
            out["roughness"][m], out["metalness"][m] = float(F(mat["rm"][0])), float(F(mat["rm"][1]))
        else:
            rm = _sample(sc.textures[tr], uv)
            out["roughness"][m], out["metalness"][m] = rm[:, 1], rm[:, 2]
        out["material"][m], out["shaded"][m] = g["material"], True
    return out


def direct_brdf(albedo, roughness, metalness, sn, v, l):
    """gi_np.evaluate_direct_brdf, float64 (the zero-denominator Cook-Torrance term is 0 there too)"""
    dot = lambda a, b: np.sum(a * b, -1)  # noqa: E731
    sat = lambda x: np.clip(x, 0.0, 1.0)  # noqa: E731
    pi = float(gi_np.PI)
    h = _unit(v + l)
    ldotn, vdoth, vdotn, ndoth = dot(l, sn), sat(dot(v, h)), dot(v, sn), dot(sn, h)
    f0 = 0.04 + metalness[:, None] * (albedo - 0.04)
    fr = f0 + (1.0 - f0) * (1.0 - vdoth ** 5)[:, None]
    vn, ln, nh = sat(vdotn), sat(ldotn), sat(ndoth)
    alpha = roughness * roughness
    a2 = alpha * alpha
    dist = (nh * nh) * (a2 - 1.0) + 1.0
    with np.errstate(all="ignore"):
        ndf = a2 / (pi * dist * dist)
        k = alpha * 0.5
        gsf = (vn / (vn * (1.0 - k) + k)) * (ln / (ln * (1.0 - k) + k))
        den = 4.0 * vn * ln
        spec = np.where((den > 0)[:, None], (ndf * gsf / den)[:, None] * fr, 0.0)
    return (1.0 - fr) * (albedo / pi) + spec


def disk_draws(n, frame_index):
    """a0, a1 of ray i: rng = JenkinsHash(i ^ JenkinsHash(frameIndex)), two Rand (float32, exact)"""
    rng = gi_np.jenkins_hash(np.arange(n, dtype=U32) ^ gi_np.jenkins_hash(np.array([frame_index], U32)))
    return gi_np.rand2(rng)


def sun_frame(c, dtype):
    sun_dir = np.array(list(c.sunLightDirection), F).astype(dtype)
    nrm = gi_np.normalize if dtype == F else _unit
    L = nrm(-sun_dir[None])[0]
    B = nrm(gi_np.perpendicular(L[None]).astype(dtype))[0]
    T = np.cross(B, L).astype(dtype)
    return L, B, T


def shadow_rays(hitP, GN, c, dtype):
    """the shadow ray of every hit (pathtracer.hlsl:546-557) in `dtype` -> rays [n, 8] of that dtype (tmin 0.001, tmax 10000)"""
    n = len(hitP)
    a0, a1 = disk_draws(n, int(c.frameIndex))
    L, B, T = sun_frame(c, dtype)
    if dtype == F:
        angle, dist = a0 * F(2.0) * F(3.1415926535), np.sqrt(a1, dtype=F)
        inc = gi_np.normalize((L + (B * np.sin(angle, dtype=F)[:, None] + T * np.cos(angle, dtype=F)[:, None]) * F(c.sunTanHalfAngle) * dist[:, None]).astype(F))
        transition = gi_np.dot(GN, inc) <= 0
    else:
        angle, dist = a0.astype(dtype) * 2.0 * 3.1415926535, np.sqrt(a1.astype(dtype))
        inc = _unit(L + (B * np.sin(angle)[:, None] + T * np.cos(angle)[:, None]) * float(F(c.sunTanHalfAngle)) * dist[:, None])
        transition = np.sum(GN * inc, -1) <= 0
    so = (hitP + np.where(transition[:, None], -GN, GN) * dtype(1e-2)).astype(dtype)
    rays = np.zeros((n, 8), dtype)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = so, 0.001, inc, TRACE_MAX
    return rays


def occluded(tris, rays, mask):
    """float64 any-hit of rays[mask] in (tmin, tmax) against `tris` -> bool [n], False outside the mask"""
    out = np.zeros(len(rays), bool)
    if mask.any():
        r = rays[mask]
        hit = V.cast(tris, r[:, 0:3], r[:, 4:7], tmin=r[:, 3], tmax=TRACE_MAX)
        out[mask] = hit["geometry"] != NO_SUBMESH
    return out


# ------------------------------------------------------------------------------------------------
# the two readings of a set of answers (geometry, primitive per ray)
# ------------------------------------------------------------------------------------------------
def _walkable(rays):
    r = np.asarray(rays, np.float64)
    with np.errstate(all="ignore"):
        dd, oo = np.sum(r[:, 4:7] ** 2, -1), np.sum(r[:, 0:3] ** 2, -1)
        f32 = np.asarray(rays, F)
        dd32, oo32 = np.sum(f32[:, 4:7] ** 2, -1, dtype=F), np.sum(f32[:, 0:3] ** 2, -1, dtype=F)
        return (dd > 0) & np.isfinite(dd32) & np.isfinite(oo32) & np.isfinite(oo) & (r[:, 3] >= 0) & (r[:, 7] > r[:, 3])


def reading64(sc, tris, rays, geometry, primitive, c=None):
    """float64 on the named triangles -> dict(found, t, u, v, position, GN, SN, albedo, roughness, metalness, texcoord, material,
    attributes, shaded, walkable, and with constants: visible bool (shadow ray unoccluded, where shaded), radiance [n, 3])"""
    rays = np.asarray(rays, F)
    geometry, primitive = np.asarray(geometry).astype(U32), np.asarray(primitive).astype(U32)
    found = geometry != NO_SUBMESH
    idx = Q.triangle_index(tris, geometry, primitive)
    assert (idx[found] >= 0).all(), "an answer names a triangle the scene does not have"
    t, u, v = Q.moller_trumbore(tris, np.maximum(idx, 0), rays)
    t, u, v = np.where(found, t, np.inf), np.where(found, u, 0.0), np.where(found, v, 0.0)
    out = reconstruct(sc, np.where(found, geometry, NO_SUBMESH), primitive, u, v)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    with np.errstate(all="ignore"):
        out["position"] = np.where(found[:, None], o + d * np.where(found, t, 0.0)[:, None], 0.0)
    out.update(found=found, t=t, u=u, v=v, walkable=_walkable(rays))
    if c is not None:
        sh = shadow_rays(out["position"], out["GN"], c, np.float64)
        out["visible"] = out["shaded"] & ~occluded(tris, sh, out["shaded"])
        L = sun_frame(c, np.float64)[0]
        brdf = direct_brdf(out["albedo"], out["roughness"], out["metalness"], out["SN"], _unit(-d), np.broadcast_to(L, (len(rays), 3)))
        sun, sky = np.array(list(c.sunLightRadiance), F).astype(np.float64), np.array(list(c.skyColor), F).astype(np.float64)
        with np.errstate(all="ignore"):
            out["lit"] = np.where(out["shaded"][:, None], brdf * sun, 0.0)  # what an unoccluded shadow ray adds
        out["radiance"] = np.where(out["visible"][:, None], out["lit"], 0.0)
        out["radiance"][out["walkable"] & ~found] = sky
    return out


def reading32(sc, tris, rays, geometry, primitive, c=None, flat=None):
    """the float32 reading of the same triangles: float32 Moeller-Trumbore, gi_np.FlatScene.reconstruct, gi_np.evaluate_direct_brdf, the
    float32 shadow ray of gi_np.trace decided by the float64 caster (as every float32 ray here is) -> the keys of reading64 it can give"""
    rays = np.asarray(rays, F)
    geometry, primitive = np.asarray(geometry).astype(U32), np.asarray(primitive).astype(U32)
    found = geometry != NO_SUBMESH
    idx = Q.triangle_index(tris, geometry, primitive)
    t, u, v = Q.moller_trumbore(tris, np.maximum(idx, 0), rays, F)
    t, u, v = np.where(found, t, F(np.inf)).astype(F), np.where(found, u, 0).astype(F), np.where(found, v, 0).astype(F)
    flat = flat or gi_np.FlatScene(sc)
    first = np.concatenate([[0], np.cumsum([len(g["indices"]) // 3 for g in sc.geometries])])
    soup = np.where(found, first[np.where(found, geometry, 0)] + np.where(found, primitive, 0), 0).astype(np.int64)
    surf, ok = flat.reconstruct(soup[found], u[found], v[found])
    n = len(rays)
    out = dict(found=found, t=t, u=u, v=v, shaded=np.zeros(n, bool))
    out["shaded"][found] = ok
    for k, key in (("GN", "GN"), ("SN", "SN"), ("albedo", "albedo"), ("roughness", "roughness"), ("metalness", "metalness")):
        a = np.zeros((n,) + surf[key].shape[1:], F)
        a[found] = surf[key]
        out[k] = a
    # the uv the maps are sampled at (FlatScene.reconstruct keeps it to itself): its expression, float32
    uv = np.zeros((n, 2), F)
    for gi in np.unique(geometry[found]):
        g = sc.geometries[int(gi)]
        if any(g[k] is None for k in ("positions", "normals", "uvs", "tangents")):
            continue
        m = found & (geometry == gi)
        ix = g["indices"].reshape(-1, 3).astype(np.int64)[primitive[m].astype(np.int64)]
        b1, b2 = u[m, None], v[m, None]
        b0 = F(1.0) - (b1 + b2)
        uvs = g["uvs"].astype(F)
        uv[m] = (uvs[ix[:, 0]] * b0 + uvs[ix[:, 1]] * b1 + uvs[ix[:, 2]] * b2).astype(F)
    out["texcoord"] = uv
    o, d = rays[:, 0:3], rays[:, 4:7]
    with np.errstate(all="ignore"):
        out["position"] = np.where(found[:, None], (o + d * np.where(found, t, F(0))[:, None]).astype(F), F(0))
    if c is not None:
        sh = shadow_rays(out["position"], out["GN"], c, F)
        out["visible"] = out["shaded"] & ~occluded(tris, sh, out["shaded"])
        L = sun_frame(c, F)[0]
        with np.errstate(all="ignore"):
            brdf = gi_np.evaluate_direct_brdf(out["albedo"], out["roughness"], out["metalness"], out["SN"], gi_np.normalize(-d), np.broadcast_to(L, (n, 3)))
            out["lit"] = np.where(out["shaded"][:, None], brdf * np.array(list(c.sunLightRadiance), F), F(0))
        out["radiance"] = np.where(out["visible"][:, None], out["lit"], F(0))
    return out


def errors(ref, got, radiance_key=None):
    """the largest error of each field class of `got` (a reading, or surface records by the names below) against the float64 reading:
    position relative to max(1, |x|), the others absolute; only where ref's flags define the field"""
    att, sh, found = ref["attributes"], ref["shaded"], ref["found"]

    def worst(e, mask):
        e = np.where(np.isnan(e), np.inf, e)
        e = e.reshape(len(e), -1).max(-1)
        return float(e[mask].max(initial=0.0))
    with np.errstate(all="ignore"):
        out = dict(position=worst(np.abs(got["position"] - ref["position"]) / np.maximum(1.0, np.abs(ref["position"])), found),
                   normal=max(worst(np.abs(got["GN"] - ref["GN"]), att), worst(np.abs(got["SN"] - ref["SN"]), sh)),  # (SN without a material: judge_surface)
                   albedo=worst(np.abs(got["albedo"] - ref["albedo"]), sh),
                   rm=max(worst(np.abs(got["roughness"] - ref["roughness"]), sh), worst(np.abs(got["metalness"] - ref["metalness"]), sh)),
                   texcoord=worst(np.abs(got["texcoord"] - ref["texcoord"]), att))
        if radiance_key is not None:
            out["radiance"] = worst(np.abs(got[radiance_key] - ref[radiance_key]) / np.maximum(1.0, np.abs(ref[radiance_key])), sh)
    return out


# ------------------------------------------------------------------------------------------------
# the judges
# ------------------------------------------------------------------------------------------------
def surface_records(reading):
    """a reading as the device would report it (neb_ray_surface): what judge_surface takes"""
    n = len(reading["found"])
    rec = np.zeros(n, SURFACE)
    f = reading["found"]
    att = reading.get("attributes", f)
    rec["position"], rec["t"] = reading["position"], reading["t"]
    rec["geometric_normal"], rec["shading_normal"], rec["texcoord"] = reading["GN"], reading["SN"], reading["texcoord"]
    rec["albedo"], rec["roughness"], rec["metalness"] = reading["albedo"], reading["roughness"], reading["metalness"]
    rec["geometry"], rec["primitive"] = reading["geometry"], reading["primitive"]
    rec["material"], rec["u"], rec["v"] = reading["material"], reading["u"], reading["v"]
    with np.errstate(all="ignore"):
        back = att & (np.sum(reading["GN"] * reading["direction"], -1) > 0)
    rec["flags"] = (f * _lib.HIT_FOUND | att * _lib.HIT_ATTRIBUTES | reading["shaded"] * _lib.HIT_MATERIAL | back * _lib.HIT_BACKFACE
                    | ~reading["walkable"] * _lib.HIT_NOT_WALKED).astype(U32)
    return rec


def radiance_records(reading):
    """a reading as neb_ray_radiance records: what judge_radiance takes"""
    rec = np.zeros(len(reading["found"]), RADIANCE)
    rec["radiance"], rec["t"], rec["geometry"], rec["primitive"] = reading["radiance"], reading["t"], reading["geometry"], reading["primitive"]
    flags = surface_records(reading)["flags"]
    rec["flags"] = flags | (reading["visible"] * _lib.HIT_SUN_VISIBLE).astype(U32)
    return rec


def as_answers(reading, rays, geometry, primitive):
    """completes a reading with what the record builders need"""
    out = dict(reading)
    out.update(geometry=np.asarray(geometry, U32), primitive=np.asarray(primitive, U32), direction=np.asarray(rays, F)[:, 4:7].astype(np.float64))
    return out


def judge_surface(sc, tris, rays, rec, what):
    """neb_ray_surface records against the float64 reading of the triangles they name: flags, the fields a flag leaves undefined, and
    every defined field within TOL.  -> the errors (printed)"""
    rays = np.asarray(rays, F)
    ref = reading64(sc, tris, rays, rec["geometry"], rec["primitive"])
    flags = rec["flags"]
    found, att, sh = ref["found"], ref["attributes"], ref["shaded"]
    assert not (flags & ~U32(0x1F)).any() and not rec["reserved"].any(), what
    assert np.array_equal((flags & _lib.HIT_FOUND) != 0, found), what
    assert np.array_equal((flags & _lib.HIT_NOT_WALKED) != 0, ~ref["walkable"]), f"{what}: NOT_WALKED"
    assert not (found & ~ref["walkable"]).any(), f"{what}: a ray that cannot be walked found something"
    assert np.array_equal((flags & _lib.HIT_ATTRIBUTES) != 0, att), f"{what}: ATTRIBUTES"
    assert np.array_equal((flags & _lib.HIT_MATERIAL) != 0, sh), f"{what}: MATERIAL"
    assert np.array_equal(rec["material"], ref["material"]), f"{what}: material"
    with np.errstate(all="ignore"):
        facing = np.sum(ref["GN"] * rays[:, 4:7].astype(np.float64), -1)
    sure = att & (np.abs(facing) >= BACKFACE_SKIP)
    assert np.array_equal(((flags & _lib.HIT_BACKFACE) != 0)[sure], facing[sure] > 0), f"{what}: BACKFACE"
    assert not (flags[~att] & _lib.HIT_BACKFACE).any(), f"{what}: BACKFACE without ATTRIBUTES"
    # what a clear flag leaves is 0: the whole record of a miss, normals and texcoord without attributes, the material's fields without one
    miss = np.zeros(1, SURFACE)
    miss["t"], miss["geometry"], miss["primitive"], miss["material"] = np.inf, NO_SUBMESH, NO_SUBMESH, -1
    blank = rec[~found].copy()
    blank["flags"] = 0
    assert (blank.view(np.uint8).reshape(len(blank), SURFACE.itemsize) == miss.view(np.uint8).reshape(1, SURFACE.itemsize)).all(), f"{what}: a miss record is not the miss record"
    for k in ("geometric_normal", "shading_normal", "texcoord"):
        assert not rec[k][~att].view(U32).any(), f"{what}: {k} without ATTRIBUTES"
    for k in ("albedo", "roughness", "metalness"):
        assert not rec[k][~sh].view(U32).any(), f"{what}: {k} without MATERIAL"
    only_att = att & ~sh
    assert np.array_equal(rec["shading_normal"][only_att].view(U32), rec["geometric_normal"][only_att].view(U32)), f"{what}: SN != GN without a material"
    got = dict(position=rec["position"].astype(np.float64), GN=rec["geometric_normal"].astype(np.float64), SN=rec["shading_normal"].astype(np.float64),
               albedo=rec["albedo"].astype(np.float64), roughness=rec["roughness"].astype(np.float64), metalness=rec["metalness"].astype(np.float64),
               texcoord=rec["texcoord"].astype(np.float64))
    err = errors(ref, got)
    print(f"[{what}] " + ", ".join(f"{k} {err[k]:.2e} / {TOL[k]:.1e}" for k in err) + f"; {int(found.sum())} hits, {int(sh.sum())} shaded, "
          f"{int((att & ~sh).sum())} without material, {int((found & ~att).sum())} without attributes")
    for k in err:
        assert err[k] <= TOL[k], f"{what}: {k} off by {err[k]:.3e}, tolerance {TOL[k]:.1e}"
    return err


def judge_radiance(sc, tris, rays, rec, c, what, cap=TIE_CAP):
    """neb_ray_radiance records against the float64 reading of the triangles they name -> (shadow outcomes that differ, largest error)"""
    rays = np.asarray(rays, F)
    ref = reading64(sc, tris, rays, rec["geometry"], rec["primitive"], c)
    flags, rgb = rec["flags"], rec["radiance"]
    found, sh = ref["found"], ref["shaded"]
    assert not (flags & ~U32(0x3F)).any() and not rec["reserved"].any(), what
    for bit, want, name in ((_lib.HIT_FOUND, found, "FOUND"), (_lib.HIT_NOT_WALKED, ~ref["walkable"], "NOT_WALKED"),
                            (_lib.HIT_ATTRIBUTES, ref["attributes"], "ATTRIBUTES"), (_lib.HIT_MATERIAL, sh, "MATERIAL")):
        assert np.array_equal((flags & bit) != 0, want), f"{what}: {name}"
    sky = np.array(list(c.skyColor), F)
    real_miss = ~found & ref["walkable"]
    assert (rgb[real_miss].view(U32) == sky.view(U32)).all(), f"{what}: a miss is not the sky's bits"
    assert not rgb[~ref["walkable"]].view(U32).any(), f"{what}: a ray that was not walked carries light"
    assert not rgb[found & ~sh].view(U32).any(), f"{what}: a hit without a material carries light"
    visible = (flags & _lib.HIT_SUN_VISIBLE) != 0
    assert not visible[~sh].any(), f"{what}: SUN_VISIBLE without MATERIAL"
    assert not rgb[sh & ~visible].view(U32).any(), f"{what}: an occluded hit carries light"
    differ = sh & (visible != ref["visible"])
    agree = sh & ~differ
    with np.errstate(all="ignore"):
        e = np.abs(rgb.astype(np.float64) - ref["radiance"]) / np.maximum(1.0, np.abs(ref["radiance"]))
    e = np.where(np.isnan(e), np.inf, e).max(-1)
    worst = float(e[agree].max(initial=0.0))
    print(f"[{what}] shadow outcomes differ from float64 at {int(differ.sum())} of {int(sh.sum())} shaded hits ({int(ref['visible'].sum())} see the sun); "
          f"radiance off by {worst:.2e} / {TOL['radiance']:.1e}, largest value {float(ref['radiance'][agree].max(initial=0.0)):.3f}")
    assert int(differ.sum()) <= cap, f"{what}: {int(differ.sum())} shadow outcomes differ from float64's"
    assert worst <= TOL["radiance"], f"{what}: radiance off by {worst:.3e}, tolerance {TOL['radiance']:.1e}; first at ray {int(np.argmax(np.where(agree, e, 0)))}"
    return int(differ.sum()), worst
