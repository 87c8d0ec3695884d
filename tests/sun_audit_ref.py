"""The sun table audited per triangle against float64 (TEST INFRASTRUCTURE, NOT PRODUCT CODE).

The table (nebulae_amd/csrc/gi_sun_table.hip) keeps, in every triangle slot's 128-byte shading record, one LIT BIT per side -- "no shadow
ray that starts on this side of this triangle can be occluded" -- and up to four occluder HINTS, slot indices the shade pass reads
`tris` with.  This file decodes the records as neb_gi_debug_shade_records returns them and holds them to what they claim, in plain
numpy float64.  It is written from the comments of gi_internal.h (the record's words, pack_hints' bit fields) and from the shader
reading in oracle/gi_np.py (trace, its sun next-event estimation): it calls neither the library nor lit_predicate.h.

  decode(records)       the words of a record: geometry, lit bits, primitive, the four hints, the side they are for
  AuditScene(scene)     the scene's world-space triangles (oracle.gi_np.FlatScene), without the hidden geometries
  shadow_rays(...)      the shader's shadow rays from 12 sample points per triangle towards 7 points of the sun disk
  occluded(...)         brute-force float64 any-hit against every visible triangle
  audit(...)            (a) occluded rays from sides called lit, (b) structural violations of the hints, (c) the share of all-clear
                        sides that carry a lit bit, (d) the share of occluded rays on hinted receivers that a hint occludes

No tolerance on (a) and (b): the certificate keeps a slack of at least 2e-4 (lit_predicate.h), so a float64 ray from a side proven
lit clears every triangle by far more than the rounding of this file.  tests/test_sun_audit_cpu.py shows that the audit passes the
CPU prototype's flags on every scene of the GPU test, and that it fails when a record is tampered with.
"""
import math

import numpy as np

from oracle import gi_np as G

F = np.float32
K_LIT_SHIFT = 30
K_GEOM_MASK = (1 << K_LIT_SHIFT) - 1
K_NO_HINT = 0x7FFFFF
K_HINTS = 4
RAY_OFFSET, RAY_TMIN = 1e-2, 0.001  # origin = P -+ GN * 1e-2, TMin of the sun RayQuery (gi_np.trace)
PULL_IN = 1e-3                      # corner and edge samples: this share of the edges inside the triangle
N_RANDOM, N_RIM = 5, 6


# ------------------------------------------------------------------------------------------------
# the records
# ------------------------------------------------------------------------------------------------
def decode(records):
    """records: uint32 [n_slots, 32] -> dict of per-slot arrays: geometry, lit (bit 0: the +GN side, bit 1: the -GN side), primitive,
    hints int64 [n_slots, 4] (K_NO_HINT: none), hint_side.  Word 27 (r6.w) = geometry | lit << 30; word 28 (r7.x) = primitive; words
    29-31 (r7.yzw) = 96 bits: hint k in bits 23 k .. 23 k + 22, the side in bit 95."""
    r = np.ascontiguousarray(records, np.uint32).reshape(-1, 32)
    w = r[:, 27]
    bits = r[:, 29].astype(object) | (r[:, 30].astype(object) << 32) | (r[:, 31].astype(object) << 64)  # exact 96-bit integers
    hints = np.array([[(int(b) >> (23 * k)) & K_NO_HINT for k in range(K_HINTS)] for b in bits], np.int64).reshape(-1, K_HINTS)
    return dict(geometry=(w & np.uint32(K_GEOM_MASK)).astype(np.int64), lit=(w >> np.uint32(K_LIT_SHIFT)).astype(np.int64),
                primitive=r[:, 28].astype(np.int64), hints=hints, hint_side=np.array([int(b) >> 95 for b in bits], np.int64))


def encode(geometry, lit, primitive, hints, hint_side):
    """the inverse of decode, for tests that make up records: -> uint32 [n, 32], every other word zero"""
    n = len(geometry)
    r = np.zeros((n, 32), np.uint32)
    r[:, 27] = (np.asarray(geometry, np.int64) | (np.asarray(lit, np.int64) << K_LIT_SHIFT)).astype(np.uint32)
    r[:, 28] = np.asarray(primitive, np.int64).astype(np.uint32)
    for i in range(n):
        b = int(hint_side[i]) << 95
        for k in range(K_HINTS):
            b |= (int(hints[i][k]) & K_NO_HINT) << (23 * k)
        r[i, 29], r[i, 30], r[i, 31] = b & 0xFFFFFFFF, (b >> 32) & 0xFFFFFFFF, (b >> 64) & 0xFFFFFFFF
    return r


# ------------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------------
class AuditScene:
    """The triangle soup of oracle.gi_np.FlatScene (float32 world-space vertices, held as float64) with a lookup from (geometry,
    primitive) to the soup.  visible: one bool per geometry (DeferredRenderer.visibility()); a hidden geometry occludes nothing."""

    def __init__(self, scene, visible=None):
        self.fs = G.FlatScene(scene)
        counts = [len(g["indices"]) // 3 for g in scene.geometries]
        self.first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.counts = np.array(counts, np.int64)
        vis = np.ones(len(counts), bool) if visible is None else np.asarray(visible, bool)
        self.tri_visible = vis[self.fs.geom]
        self.shaded = np.array([all(g[k] is not None for k in ("positions", "normals", "uvs", "tangents")) for g in scene.geometries], bool)
        self.n = len(self.fs.geom)

    def slot_triangle(self, dec):
        """per slot the index of its triangle in the soup, -1 where (geometry, primitive) names none"""
        g, p = dec["geometry"], dec["primitive"]
        ok = (g >= 0) & (g < len(self.counts))
        gg = np.where(ok, g, 0)
        ok &= p < self.counts[gg]
        return np.where(ok, self.first[gg] + p, -1)


def sample_points(n_tris, seed=7):
    """barycentrics (bu, bv) [n_tris, 12, 2] of the hit-point samples: the corners and the edge midpoints pulled in by PULL_IN of the
    edge lengths, the centroid, N_RANDOM random interior points (one seeded stream, another five per triangle)"""
    e = PULL_IN
    fixed = np.array([[e, e], [1 - 2 * e, e], [e, 1 - 2 * e],                                 # corners v0, v1, v2
                      [0.5 - 0.5 * e, e], [0.5 - 0.5 * e, 0.5 - 0.5 * e], [e, 0.5 - 0.5 * e],  # midpoints of v0v1, v1v2, v2v0
                      [1.0 / 3.0, 1.0 / 3.0]])
    rnd = np.random.default_rng(seed).random((n_tris, N_RANDOM, 2))
    fold = rnd.sum(-1) > 1.0
    rnd[fold] = 1.0 - rnd[fold]
    rnd = e + rnd * (1.0 - 3.0 * e)  # (kept PULL_IN inside every edge as well)
    return np.concatenate([np.broadcast_to(fixed, (n_tris,) + fixed.shape), rnd], 1)


def disk_dirs(sun, tan_half):
    """the shader's directions to the disk centre and to N_RIM points of its rim (dist = 1), float32 as gi_np.trace computes `inc`"""
    sun = np.array(sun, F)
    L = G.normalize(-sun[None])[0]
    B = G.normalize(G.perpendicular(L[None]))[0]
    T = G.cross(B[None], L[None])[0]
    out = [L]
    for k in range(N_RIM):
        a = F(k) * F(2.0) * F(3.1415926535) / F(N_RIM)
        out.append(G.normalize((L + (B * np.sin(a, dtype=F) + T * np.cos(a, dtype=F)) * F(tan_half) * F(1.0))[None].astype(F))[0])
    return np.stack(out).astype(F)


def shadow_rays(scene, tris, samples, dirs):
    """scene: AuditScene; tris: indices into its soup; samples: (bu, bv) [len(tris), s, 2]; dirs: disk_dirs -> dict of flat arrays over
    (triangle, sample, direction): tri, sample, origin float32 [m, 3], dir (index into dirs), side (0: the ray starts on the +GN side, 1: -GN).
    The shader's ray (gi_np.trace): P at the barycentrics in float32, GN interpolated and instance-transformed (FlatScene.reconstruct),
    side = dot(GN, inc) <= 0, origin = P -+ GN * 1e-2 in float32.  Triangles of a geometry without all attribute streams give no rays."""
    fs = scene.fs
    tris = np.asarray(tris, np.int64)
    s, nd = samples.shape[1], len(dirs)
    tt = np.repeat(tris, s)
    sample = np.tile(np.arange(s), len(tris))
    bu, bv = samples[..., 0].reshape(-1).astype(F), samples[..., 1].reshape(-1).astype(F)
    surf, _ = fs.reconstruct(tt, bu, bv)
    keep = scene.shaded[fs.geom[tt]]
    tt, bu, bv, GN, sample = tt[keep], bu[keep], bv[keep], surf["GN"][keep], sample[keep]
    b0 = (F(1.0) - (bu + bv)).astype(F)
    P = (fs.v0[tt].astype(F) * b0[:, None] + fs.v1[tt].astype(F) * bu[:, None] + fs.v2[tt].astype(F) * bv[:, None]).astype(F)
    tri = np.repeat(tt, nd)
    di = np.tile(np.arange(nd), len(tt))
    GNr, Pr = np.repeat(GN, nd, 0), np.repeat(P, nd, 0)
    transition = G.dot(GNr, dirs[di]) <= 0
    origin = (Pr + np.where(transition[:, None], -GNr, GNr) * F(RAY_OFFSET)).astype(F)
    return dict(tri=tri, sample=np.repeat(sample, nd), origin=origin, dir=di, side=transition.astype(np.int64))


def occluded(scene, rays, dirs, only=None, chunk=4_000_000):
    """Brute-force float64 any-hit of the rays against every visible triangle, the acceptance of FlatScene.intersect (Moeller-Trumbore,
    det != 0, 0 <= u <= 1, v >= 0, u + v <= 1, TMin < t < 10000).  The rays of a scene share len(dirs) directions, so per direction the
    three scalar triple products are matrix products: u = tv.(d x e2) / det, v = tv.(e1 x d) / det, t = tv.(e1 x e2) / det.
    -> (hit bool [m], first int64 [m]: the soup index of the first occluder in scene order, -1: none).
    only: int64 [m, k] soup indices (-1: none) -- then the rays are tested against those triangles alone, hidden ones excepted."""
    fs = scene.fs
    m = len(rays["tri"])
    hit, first = np.zeros(m, bool), np.full(m, -1, np.int64)
    vis = np.nonzero(scene.tri_visible)[0]
    if m == 0 or len(vis) == 0:
        return hit, first
    v0, e1, e2 = fs.v0[vis], fs.v1[vis] - fs.v0[vis], fs.v2[vis] - fs.v0[vis]
    nrm = np.cross(e1, e2)
    col = np.full(scene.n + 1, -1, np.int64)  # soup index -> column among the visible (the last entry: "none")
    col[vis] = np.arange(len(vis))
    step = max(1, chunk // len(vis))
    for k in range(len(dirs)):
        d = dirs[k].astype(np.float64)
        p, r = np.cross(d[None], e2), np.cross(e1, d[None])
        det = np.sum(e1 * p, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
        cp, cr, cn = np.sum(v0 * p, -1), np.sum(v0 * r, -1), np.sum(v0 * nrm, -1)
        ids = np.nonzero(rays["dir"] == k)[0]
        for a in range(0, len(ids), step):
            ii = ids[a:a + step]
            o = rays["origin"][ii].astype(np.float64)
            with np.errstate(invalid="ignore"):
                u = (o @ p.T - cp) * inv
                v = (o @ r.T - cr) * inv
                t = (o @ nrm.T - cn) * inv
                h = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > RAY_TMIN) & (t < G.TRACING_MAX_DISTANCE)
            if only is not None:
                c = col[only[ii]]
                h = (np.take_along_axis(h, np.maximum(c, 0), 1) & (c >= 0))
                hit[ii] = h.any(1)
            else:
                hit[ii] = h.any(1)
                first[ii] = np.where(hit[ii], vis[np.argmax(h, 1)], -1)
    return hit, first


# ------------------------------------------------------------------------------------------------
# the audit
# ------------------------------------------------------------------------------------------------
def hint_violations(dec, scene=None):
    """list (b): (slot, what) for every structural violation of a record's hints"""
    n = len(dec["geometry"])
    bad = []
    H, side, lit = dec["hints"], dec["hint_side"], dec["lit"]
    for s in range(n):
        h = [int(x) for x in H[s]]
        present = [x for x in h if x != K_NO_HINT]
        for x in present:
            if x >= n:
                bad.append((s, f"hint {x} is neither kNoHint nor below n_slots = {n}"))
            if x == s:
                bad.append((s, "a hint names its own slot"))
        seen_none = False
        for x in h:
            if x == K_NO_HINT:
                seen_none = True
            elif seen_none:
                bad.append((s, f"hint {x} stands behind a kNoHint entry"))
                break
        if len(set(present)) != len(present):
            bad.append((s, f"duplicate hints {h}"))
        if side[s] not in (0, 1):
            bad.append((s, f"hint_side {int(side[s])}"))
        elif present and (lit[s] >> side[s]) & 1:
            bad.append((s, f"hints {h} on a record whose hint_side {int(side[s])} is lit"))
        if scene is not None:
            g = int(dec["geometry"][s])
            if g < len(scene.shaded) and not scene.shaded[g] and (present or lit[s]):
                bad.append((s, f"a submesh without attribute streams carries lit bits {int(lit[s])} / hints {h}"))
    return bad


def audit(dec, scene, sun, tan_half, shares=False, seed=7):
    """dec: decode(records); scene: AuditScene of the scene the table was built for -> dict:
      occluded_lit   list (a): (slot, triangle, side, sample, direction, occluder) for rays occluded in float64 that start on a side
                     whose lit bit is set (first 50; "n_occluded_lit" counts all)
      violations     list (b): hint_violations, plus slots whose (geometry, primitive) names no triangle of the scene
      lit_sides      lit bits set, {side: count}; hinted: records with a hint
      lit_share      (c), with shares=True: of the (triangle, side) pairs that sampled rays start on and whose sampled rays are all
                     clear, the share whose lit bit is set in every slot of the triangle; "clear_sides" is their number
      hint_share     (d), with shares=True: of the occluded sampled rays that start on the hinted side of a hinted slot's triangle,
                     the share one of the slot's hints occludes; "hinted_rays" is their number
    Without `shares` only rays that can enter list (a) are traced: those of triangles with a lit bit in some slot."""
    n_slots = len(dec["geometry"])
    st = scene.slot_triangle(dec)
    violations = hint_violations(dec, scene)
    violations += [(int(s), f"(geometry {int(dec['geometry'][s])}, primitive {int(dec['primitive'][s])}) names no triangle") for s in np.nonzero(st < 0)[0]]
    lit = dec["lit"]
    # per triangle and side: lit in some slot / in every slot (a split triangle has several slots: all are audited as the one triangle)
    some, every = np.zeros((scene.n, 2), bool), np.ones((scene.n, 2), bool)
    has_slot = np.zeros(scene.n, bool)
    ok = (st >= 0) & scene.tri_visible[np.maximum(st, 0)]  # (no ray meets a hidden submesh: no shadow ray starts there, its bits say nothing)
    for side in (0, 1):
        b = ((lit >> side) & 1).astype(bool)
        np.logical_or.at(some[:, side], st[ok], b[ok])
        np.logical_and.at(every[:, side], st[ok], b[ok])
    has_slot[st[ok]] = True
    every &= has_slot[:, None]
    want = np.nonzero(has_slot if shares else some.any(1))[0]
    dirs = disk_dirs(sun, tan_half)
    samples = sample_points(scene.n, seed)[want]
    rays = shadow_rays(scene, want, samples, dirs)
    if not shares:  # only the rays that start on a side called lit
        keep = some[rays["tri"], rays["side"]]
        rays = {k: v[keep] for k, v in rays.items()}
    hit, first = occluded(scene, rays, dirs)
    wrong = np.nonzero(hit & some[rays["tri"], rays["side"]])[0]
    slot_of = {}
    for s in np.nonzero(ok)[0]:
        slot_of.setdefault(int(st[s]), []).append(int(s))
    occluded_lit = []
    for i in wrong[:50]:
        t, side = int(rays["tri"][i]), int(rays["side"][i])
        slot = next(s for s in slot_of[t] if (lit[s] >> side) & 1)
        occluded_lit.append(dict(slot=slot, triangle=t, geometry=int(scene.fs.geom[t]), primitive=int(scene.fs.prim[t]), side=side,
                                 sample=int(rays["sample"][i]), direction=int(rays["dir"][i]), origin=rays["origin"][i].tolist(),
                                 occluder=int(first[i])))
    out = dict(occluded_lit=occluded_lit, n_occluded_lit=int(len(wrong)), violations=violations, n_slots=n_slots, rays=int(len(hit)),
               lit_sides={0: int(((lit >> 0) & 1).sum()), 1: int(((lit >> 1) & 1).sum())},
               hinted=int((dec["hints"][:, 0] != K_NO_HINT).sum()), lit_share=None, clear_sides=0, hint_share=None, hinted_rays=0)
    if shares:
        started = np.zeros((scene.n, 2), bool)
        blocked = np.zeros((scene.n, 2), bool)
        started[rays["tri"], rays["side"]] = True
        np.logical_or.at(blocked, (rays["tri"], rays["side"]), hit)
        clear = started & ~blocked
        out["clear_sides"] = int(clear.sum())
        out["lit_share"] = float((clear & every).sum()) / max(1, int(clear.sum()))
        # (d): per hinted slot, the occluded rays of its triangle on the hinted side against the slot's hints alone
        order = np.argsort(rays["tri"], kind="stable")
        lo = np.searchsorted(rays["tri"][order], np.arange(scene.n), "left")
        hi = np.searchsorted(rays["tri"][order], np.arange(scene.n), "right")
        pick, only = [], []
        for s in np.nonzero(ok & (dec["hints"][:, 0] != K_NO_HINT) & (dec["hint_side"] <= 1))[0]:
            t = int(st[s])
            ii = order[lo[t]:hi[t]]
            ii = ii[hit[ii] & (rays["side"][ii] == dec["hint_side"][s])]
            if len(ii):
                h = dec["hints"][s]
                ht = np.where((h != K_NO_HINT) & (h < n_slots), st[np.minimum(h, n_slots - 1)], -1)
                pick.append(ii)
                only.append(np.broadcast_to(ht, (len(ii), K_HINTS)))
        if pick:
            pick, only = np.concatenate(pick), np.concatenate(only)
            sub = {k: v[pick] for k, v in rays.items()}
            by_hint, _ = occluded(scene, sub, dirs, only=only)
            out["hinted_rays"] = int(len(pick))
            out["hint_share"] = float(by_hint.sum()) / len(pick)
    return out


def sun_tan_half(diameter_deg):
    return math.tan(math.radians(diameter_deg * 0.5))
