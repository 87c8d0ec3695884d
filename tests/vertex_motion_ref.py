"""CPU reference of option svgf_vertex_motion: the previous-point plane neb_gbuffer_raycast writes for deformed
submeshes, in float64, and the third arm of the reprojecting temporal kernel.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`prev_point_plane` casts every pixel's primary ray in float64 (views_ref.primary), takes the hit triangle's barycentrics and carries
them to the triangle's PREVIOUS object-space vertices and normals under the history frame's matrices.  `reproject` is
motion_ref.reproject with the plane as one more input: a pixel whose .w is not the sentinel takes its point and geometric normal from
the plane (the normal decoded as the kernel decodes normal[hist]), every other pixel keeps motion_ref's rule.
"""
import os
import re

import numpy as np

import motion_ref as M
import reproject_ref as R
import views_ref as V
from reproject_ref import F


def _sentinel():
    text = open(os.path.join(R.ROOT, "nebulae_amd", "csrc", "svgf_reproject.h")).read()
    return np.uint32(int(re.search(r"kReprojNoPrevPoint\s*=\s*(0x[0-9A-Fa-f]+)", text).group(1), 16))


NO_PREV_POINT = _sentinel()


def deformed_geometries(sc_prev, sc_cur):
    """the geometries whose positions or normals differ between the two scenes"""
    return [k for k, (a, b) in enumerate(zip(sc_prev.geometries, sc_cur.geometries))
            if not (np.array_equal(a["positions"], b["positions"]) and np.array_equal(a["normals"], b["normals"]))]


def prev_point_plane(sc_prev, sc_cur, M_hist, cam, W, H, dirty=None):
    """sc_prev, sc_cur: the scene at the previous and at this raycast (same topology); M_hist [n, 4, 4]: the matrices of the previous
    raycast; cam: this frame's camera; dirty: the geometries a vertex update has named since the previous raycast (default: those whose
    vertices differ).  Everything in float64.
    -> dict(P [H, W, 3], N [H, W, 3] (unit), depth [H, W]: linear depth of the CURRENT hit in `cam`, flagged bool [H, W],
            geometry, primitive uint32 [H, W], covered bool [H, W])"""
    dirty = deformed_geometries(sc_prev, sc_cur) if dirty is None else list(dirty)
    hit = V.primary(sc_cur, cam, W, H)
    geom, prim = hit["geometry"], hit["primitive"]
    c = R.Camera(cam, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xa, ya, za, eye = [np.asarray(v, np.float64) for v in (c.x, c.y, c.z, c.eye)]
    d = xa * (((xs + 0.5) / W * 2.0 - 1.0) * float(c.sx))[..., None] + ya * ((1.0 - (ys + 0.5) / H * 2.0) * float(c.sy))[..., None] - za
    d /= np.sqrt(np.sum(d * d, -1, keepdims=True))
    P = np.full((H, W, 3), np.nan)
    N = np.full((H, W, 3), np.nan)
    flagged = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        depth = hit["t"] * -(d @ za)
    for gi in dirty:
        sel = hit["covered"] & (geom == gi)
        if not sel.any():
            continue
        gc, gp = sc_cur.geometries[gi], sc_prev.geometries[gi]
        tri = np.asarray(gc["indices"], np.int64).reshape(-1, 3)[prim[sel].astype(np.int64)]
        Mc = np.asarray(gc["M"], np.float64)
        Pw = np.asarray(gc["positions"], np.float64) @ Mc[:3, :3] + Mc[3, :3]
        v0, e1, e2 = Pw[tri[:, 0]], Pw[tri[:, 1]] - Pw[tri[:, 0]], Pw[tri[:, 2]] - Pw[tri[:, 0]]
        dd = d[sel]
        p = np.cross(dd, e2)
        det = np.sum(p * e1, -1)
        tv = eye - v0
        b1 = np.sum(p * tv, -1) / det
        b2 = np.sum(dd * np.cross(tv, e1), -1) / det
        b = np.stack([1.0 - (b1 + b2), b1, b2], -1)
        Mh = np.asarray(M_hist[gi], np.float64)
        q = np.einsum("nk,nkj->nj", b, np.asarray(gp["positions"], np.float64)[tri])
        P[sel] = q @ Mh[:3, :3] + Mh[3, :3]
        w = np.asarray(gp["normals"], np.float64)[tri] @ Mh[:3, :3]
        w /= np.linalg.norm(w, axis=-1, keepdims=True)
        n = np.einsum("nk,nkj->nj", b, w)
        N[sel] = n / np.linalg.norm(n, axis=-1, keepdims=True)
        flagged |= sel
    return dict(P=P, N=N, depth=depth, flagged=flagged, geometry=geom, primitive=prim, covered=hit["covered"])


def oct16_codes(n):
    """oct_pack of unit normals [..., 3] (float64) rounded to the two halfs of the normal plane's .xy -> float16 [..., 2]"""
    s = 1.0 / np.sum(np.abs(n), -1)
    px, py = n[..., 0] * s, n[..., 1] * s
    fold = n[..., 2] <= 0.0
    ex = np.where(fold, (1.0 - np.abs(py)) * np.where(px > 0, 1.0, -1.0), px)
    ey = np.where(fold, (1.0 - np.abs(px)) * np.where(py > 0, 1.0, -1.0), py)
    return np.stack([ex, ey], -1).astype(np.float16)


def half_order(h):
    """float16 -> int32 that counts codes along the real line (-0 and +0 coincide)"""
    u = np.ascontiguousarray(h, np.float16).view(np.uint16).astype(np.int32)
    return np.where(u & 0x8000, -(u & 0x7FFF), u)


def pack_plane(ref):
    """the plane the device would hold for prev_point_plane's result: float32 [H, W, 4], .w the oct16 pair or the sentinel"""
    H, W = ref["flagged"].shape
    out = np.zeros((H, W, 4), F)
    w = np.full((H, W), NO_PREV_POINT, np.uint32)
    f = ref["flagged"]
    out[f, :3] = ref["P"][f].astype(F)
    e = oct16_codes(ref["N"][f]).view(np.uint16).astype(np.uint32)
    w[f] = e[:, 0] | (e[:, 1] << 16)
    out[..., 3] = w.view(F)
    return out


def plane_fields(plane):
    """NEB_PLANE_PREV_POINT float32 [H, W, 4] -> (P float32 [H, W, 3], oct pair float16 [H, W, 2], has bool [H, W])"""
    w = np.ascontiguousarray(plane[..., 3]).view(np.uint32)
    e = np.stack([(w & 0xFFFF).astype(np.uint16), (w >> 16).astype(np.uint16)], -1).view(np.float16)
    return plane[..., :3], e, w != NO_PREV_POINT


def reproject(cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, hlen_hist, id_cur, id_hist,
              prev_plane, table=None, alpha=0.9, variance_eps=1e-4):
    """motion_ref.reproject with NEB_PLANE_PREV_POINT as one more input: where the plane's .w is not the sentinel, P and N_g are the
    plane's (N_g through the decode of normal[hist]'s .xy) and the delta entry is not looked at; elsewhere motion_ref's rule.  Such a
    pixel counts as `moved` in the result (its tap position has passed through another transform: `near` treats it so).
    The step is swapped in where motion_ref.reproject maps point and normal; everything behind it is that function's own code."""
    Hd, Wd = (depth_cur.shape[0] // 8) * 8, (depth_cur.shape[1] // 8) * 8
    Pp, e, has = plane_fields(np.ascontiguousarray(prev_plane, F)[:Hd, :Wd])
    Nv = R.geometric_normal(e)
    inner = M.map_point_normal

    def mapped(P, N, ids, tab):
        P_h, N_h, moved, frozen = inner(P, N, ids, tab)
        P_out = tuple(np.where(has, Pp[..., k], P_h[k]).astype(F) for k in range(3))
        return P_out, np.where(has[..., None], Nv, N_h).astype(F), moved | has, frozen & ~has

    M.map_point_normal = mapped
    try:
        out = M.reproject(cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, hlen_hist, id_cur, id_hist,
                          table=table, alpha=alpha, variance_eps=variance_eps)
    finally:
        M.map_point_normal = inner
    out["per_vertex"] = has
    return out
