"""CPU reference of the motion arm of the reprojecting temporal pass (option svgf_motion; nebulae_amd/csrc/svgf.hip,
reproj_delta_kernel and svgf_temporal_reproject_kernel<true>).  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

On top of tests/reproject_ref.py: the per-geometry delta table in float64 in the kernel's written-down operation order (it must
reach the kernel's fp32 bits), the mapping of a pixel's world point and geometric normal through its submesh's entry (float32, every
fmaf fused as in reproject_ref), and the id test.  `primary_ids` is a small float64 ray caster over a scene's triangles: the submesh
each pixel's primary ray hits, for G-buffers that come without ids (the CPU oracle's).
"""
import os
import re

import numpy as np

import reproject_ref as R
from reproject_ref import F, NORMAL_COS, PLANE_TOL, WEIGHT_MIN, fma, geometric_normal, surface, world_point

NO_SUBMESH = np.uint32(0xFFFFFFFF)


def _layout():
    text = open(os.path.join(R.ROOT, "nebulae_amd", "csrc", "svgf_reproject.h")).read()
    get = lambda name: int(re.search(rf"{name}\s*=\s*([0-9]+)", text).group(1))  # noqa: E731
    return get("kReprojDeltaFloat4"), get("kReprojDeltaSame"), get("kReprojDeltaMoved"), get("kReprojDeltaSingular")


ENTRY_FLOAT4, SAME, MOVED, SINGULAR = _layout()


# ---- the delta table: float64, the kernel's operation order, one rounding to float32 at the end ----

def _inverse(a):
    """cofactor inverse of [n, 3, 3] float64: nine 'product - product', det = (a00 c00 + a01 c01) + a02 c02, r = 1 / det,
    inv[i][j] = c[j][i] * r.  -> (inv, ok)"""
    c = np.empty_like(a)
    c[:, 0, 0] = a[:, 1, 1] * a[:, 2, 2] - a[:, 1, 2] * a[:, 2, 1]
    c[:, 0, 1] = a[:, 1, 2] * a[:, 2, 0] - a[:, 1, 0] * a[:, 2, 2]
    c[:, 0, 2] = a[:, 1, 0] * a[:, 2, 1] - a[:, 1, 1] * a[:, 2, 0]
    c[:, 1, 0] = a[:, 0, 2] * a[:, 2, 1] - a[:, 0, 1] * a[:, 2, 2]
    c[:, 1, 1] = a[:, 0, 0] * a[:, 2, 2] - a[:, 0, 2] * a[:, 2, 0]
    c[:, 1, 2] = a[:, 0, 1] * a[:, 2, 0] - a[:, 0, 0] * a[:, 2, 1]
    c[:, 2, 0] = a[:, 0, 1] * a[:, 1, 2] - a[:, 0, 2] * a[:, 1, 1]
    c[:, 2, 1] = a[:, 0, 2] * a[:, 1, 0] - a[:, 0, 0] * a[:, 1, 2]
    c[:, 2, 2] = a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]
    det = (a[:, 0, 0] * c[:, 0, 0] + a[:, 0, 1] * c[:, 0, 1]) + a[:, 0, 2] * c[:, 0, 2]
    r = 1.0 / det
    inv = np.transpose(c, (0, 2, 1)) * r[:, None, None]
    ok = (det != 0.0) & (np.abs(det) <= 1.7e308) & (np.abs(r) <= 1.7e308)
    return inv, ok


def _product(x, y):
    """(X Y)[i][j] = (x[i][0] y[0][j] + x[i][1] y[1][j]) + x[i][2] y[2][j]"""
    o = np.empty_like(x)
    for i in range(3):
        for j in range(3):
            o[:, i, j] = (x[:, i, 0] * y[:, 0, j] + x[:, i, 1] * y[:, 1, j]) + x[:, i, 2] * y[:, 2, j]
    return o


def delta_table(m_cur, m_hist):
    """m_cur, m_hist: [n, 4, 4] float32 surfaceToWorld (row-vector convention) of the two frames.
    -> dict(flag uint32 [n], D float32 [n, 4, 3], K float32 [n, 3, 3], entries float32 [n, 32] -- the device layout, bit for bit)"""
    mc = np.ascontiguousarray(m_cur, F).reshape(-1, 4, 4)
    mh = np.ascontiguousarray(m_hist, F).reshape(-1, 4, 4)
    n = mc.shape[0]
    same = (mc.view(np.uint32) == mh.view(np.uint32)).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        finite = (np.abs(mc) <= F(3.0e38)).all(axis=(1, 2)) & (np.abs(mh) <= F(3.0e38)).all(axis=(1, 2))
        ac, ah = mc[:, :3, :3].astype(np.float64), mh[:, :3, :3].astype(np.float64)
        tc, th = mc[:, 3, :3].astype(np.float64), mh[:, 3, :3].astype(np.float64)
        ic, ok_c = _inverse(ac)
        ih, ok_h = _inverse(ah)
        L, Q = _product(ic, ah), _product(ih, ac)
        t = np.empty((n, 3))
        for j in range(3):  # translation last
            t[:, j] = th[:, j] - ((tc[:, 0] * L[:, 0, j] + tc[:, 1] * L[:, 1, j]) + tc[:, 2] * L[:, 2, j])
        D = np.concatenate([L, t[:, None, :]], axis=1).astype(F)
        K = np.transpose(Q, (0, 2, 1)).astype(F)
        ok = finite & ok_c & ok_h & (np.abs(D) <= F(3.0e38)).all(axis=(1, 2)) & (np.abs(K) <= F(3.0e38)).all(axis=(1, 2))
    flag = np.where(same, SAME, np.where(ok, MOVED, SINGULAR)).astype(np.uint32)
    eyeD = np.concatenate([np.eye(3, dtype=F), np.zeros((1, 3), F)])
    D = np.where((flag == SAME)[:, None, None], eyeD, np.where((flag == MOVED)[:, None, None], D, F(0))).astype(F)
    K = np.where((flag == SAME)[:, None, None], np.eye(3, dtype=F), np.where((flag == MOVED)[:, None, None], K, F(0))).astype(F)
    entries = np.zeros((n, 4 * ENTRY_FLOAT4), F)
    entries.view(np.uint32)[:, 0] = flag
    entries[:, 4:16] = D.reshape(n, 12)
    entries[:, 16:25] = K.reshape(n, 9)
    return dict(flag=flag, D=D, K=K, entries=entries)


def map_point_normal(P, N, ids, table):
    """The kernel's mapping of every pixel: P = (Px, Py, Pz), N [..., 3] float32, ids uint32, table = delta_table(...) or None.
    -> (P_h, N_h, moved, frozen): moved pixels pass through D / K (explicit fmaf order, correctly rounded sqrt and divisions),
    the others keep P and N exactly; frozen pixels (flag 2) take no history."""
    shape = ids.shape
    moved = np.zeros(shape, bool)
    frozen = np.zeros(shape, bool)
    if table is None or len(table["flag"]) == 0:
        return P, N, moved, frozen
    n = len(table["flag"])
    has = ids < n
    g = np.where(has, ids, 0).astype(np.int64)
    flag = np.where(has, table["flag"][g], SAME)
    moved, frozen = flag == MOVED, flag == SINGULAR
    D, K = table["D"][g], table["K"][g]  # [..., 4, 3], [..., 3, 3]
    with np.errstate(all="ignore"):
        Ph = [fma(P[2], D[..., 2, j], fma(P[1], D[..., 1, j], fma(P[0], D[..., 0, j], D[..., 3, j]))) for j in range(3)]
        nr = [fma(N[..., 2], K[..., 2, j], fma(N[..., 1], K[..., 1, j], N[..., 0] * K[..., 0, j])) for j in range(3)]
        ln = np.sqrt(fma(nr[2], nr[2], fma(nr[1], nr[1], nr[0] * nr[0]))).astype(F)
        Nh = np.stack([(c / ln).astype(F) for c in nr], axis=-1)
    P_out = tuple(np.where(moved, Ph[k], P[k]).astype(F) for k in range(3))
    N_out = np.where(moved[..., None], Nh, N).astype(F)
    return P_out, N_out, moved, frozen


def reproject(cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, hlen_hist, id_cur, id_hist,
              table=None, alpha=0.9, variance_eps=1e-4):
    """One temporal pass of the motion arm: reproject_ref.reproject with P_h, N_h in place of P, N_g and the id test.
    table: delta_table(M_cur, M_hist), or None when nothing moved between the two frames (the library then launches no delta kernel).
    Returns what reproject_ref.reproject returns, plus moved / frozen masks; `near` also holds the moved pixels whose tap position
    lies within 1e-4 of an integer (P_h passes through one more rounded transform)."""
    H, W = depth_cur.shape
    Hd, Wd = (H // 8) * 8, (W // 8) * 8
    alpha, variance_eps = F(alpha), F(variance_eps)
    ys, xs = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
    s = (slice(0, Hd), slice(0, Wd))
    Cc = rad_cur[s].astype(F)
    dc = depth_cur[s]
    g = id_cur[s].astype(np.uint32)
    has = surface(dc) & (cam_hist is not None)
    near = np.zeros((Hd, Wd), bool)
    valid = np.zeros((4, Hd, Wd), bool)
    tap_ids_equal = np.ones((Hd, Wd), bool)  # every in-region tap carries the pixel's own id
    weights = np.zeros((4, Hd, Wd), F)
    sw = np.zeros((Hd, Wd), F)
    acc = np.zeros((Hd, Wd, 3), F)
    m0 = np.zeros((Hd, Wd), F)
    m1 = np.zeros((Hd, Wd), F)
    n = np.zeros((Hd, Wd), np.uint32)
    fx = np.full((Hd, Wd), np.nan, F)
    fy = np.full((Hd, Wd), np.nan, F)
    moved = np.zeros((Hd, Wd), bool)
    frozen = np.zeros((Hd, Wd), bool)
    if cam_hist is not None:
        ch = cam_hist
        P0 = world_point(cam_cur, xs, ys, dc)
        P, Ng, moved, frozen = map_point_normal(P0, geometric_normal(normal_cur[s]), g, table)
        r = [P[k] - ch.eye[k] for k in range(3)]
        zl = -fma(r[2], ch.z[2], fma(r[1], ch.z[1], r[0] * ch.z[0]))
        cx = fma(r[2], ch.x[2], fma(r[1], ch.x[1], r[0] * ch.x[0]))
        cy = fma(r[2], ch.y[2], fma(r[1], ch.y[1], r[0] * ch.y[0]))
        with np.errstate(all="ignore"):
            ndc_x, ndc_y = cx / (zl * ch.sx), cy / (zl * ch.sy)
            half_W, half_H = F(0.5) * F(W), F(0.5) * F(H)
            fx = fma(ndc_x, half_W, half_W) - F(0.5)
            fy = fma(-ndc_y, half_H, half_H) - F(0.5)
            inside = has & ~frozen & (zl > 0) & (fx > -1) & (fx < Wd) & (fy > -1) & (fy < Hd)
            x0f, y0f = np.floor(np.where(inside, fx, 0)), np.floor(np.where(inside, fy, 0))
        wx, wy = np.where(inside, fx, 0) - x0f, np.where(inside, fy, 0) - y0f
        near |= inside & moved & ((np.abs(fx - np.round(fx)) <= 1e-4) | (np.abs(fy - np.round(fy)) <= 1e-4))
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = PLANE_TOL * zl
        for t in range(4):
            px, py = x0 + (t & 1), y0 + (t >> 1)
            inb = inside & (px >= 0) & (px < Wd) & (py >= 0) & (py < Hd)
            pxc, pyc = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
            dt = depth_hist[pyc, pxc]
            same_id = id_hist[pyc, pxc].astype(np.uint32) == g
            tap_ids_equal &= same_id | ~inb
            ok = inb & surface(dt) & same_id
            Nt = geometric_normal(normal_hist[pyc, pxc])
            with np.errstate(all="ignore"):
                dot = fma(Ng[..., 2], Nt[..., 2], fma(Ng[..., 1], Nt[..., 1], Ng[..., 0] * Nt[..., 0]))
                near |= ok & (np.abs(dot - NORMAL_COS) <= 1e-4)
                ok &= dot >= NORMAL_COS
                Pt = world_point(ch, pxc, pyc, dt)
                dist = fma(Pt[2] - P[2], Ng[..., 2], fma(Pt[1] - P[1], Ng[..., 1], (Pt[0] - P[0]) * Ng[..., 0]))
                near |= ok & (np.abs(np.abs(dist) - tol) <= 1e-4 * np.abs(tol))
                ok &= np.abs(dist) <= tol
            w = (wx if t & 1 else F(1.0) - wx) * (wy if t >> 1 else F(1.0) - wy)
            r_t = rad_hist[pyc, pxc].astype(F)
            mh = mom_hist[pyc, pxc].astype(F)
            wv = np.where(ok, w, F(0))
            sw = np.where(ok, sw + w, sw).astype(F)
            for k in range(3):
                acc[..., k] = np.where(ok, fma(wv, r_t[..., k], acc[..., k]), acc[..., k])
            m0 = np.where(ok, fma(wv, mh[..., 0], m0), m0)
            m1 = np.where(ok, fma(wv, mh[..., 1], m1), m1)
            n = np.where(ok, np.maximum(n, hlen_hist[pyc, pxc].astype(np.uint32)), n)
            valid[t], weights[t] = ok, np.where(ok, w, F(0))
        near |= valid.any(axis=0) & (np.abs(sw - WEIGHT_MIN) <= 1e-4 * WEIGHT_MIN)
    take = sw > WEIGHT_MIN
    n = np.where(take, n, 0).astype(np.uint32)
    with np.errstate(all="ignore"):
        inv = np.where(take, F(1.0) / np.where(take, sw, F(1)), F(0)).astype(F)
    Ch = np.where(take[..., None], acc * inv[..., None], Cc[..., :3]).astype(F)
    Mh0, Mh1 = np.where(take, m0 * inv, F(0)).astype(F), np.where(take, m1 * inv, F(0)).astype(F)
    with np.errstate(divide="ignore"):
        a = np.where(n == 0, F(0), np.minimum(alpha, F(1.0) - F(1.0) / (n + 1).astype(F))).astype(F)
    out = rad_cur.astype(F).copy()
    for k in range(3):
        out[:Hd, :Wd, k] = fma(a, Ch[..., k] - Cc[..., k], Cc[..., k])
    Y = fma(Cc[..., 2], F(0.0722), fma(Cc[..., 1], F(0.7152), Cc[..., 0] * F(0.2126)))
    M1 = fma(a, Mh0 - Y, Y)
    Y2 = Y * Y
    M2 = fma(a, Mh1 - Y2, Y2)
    var = np.maximum(fma(-M1, M1, M2), variance_eps)
    moments = np.zeros((H, W, 2), np.float16)
    variance = np.zeros((H, W), np.float16)
    hlen = np.zeros((H, W), np.uint8)
    with np.errstate(over="ignore"):
        moments[:Hd, :Wd] = np.stack([M1, M2], axis=-1).astype(np.float16)
        variance[:Hd, :Wd] = var.astype(np.float16)
    hlen[:Hd, :Wd] = np.minimum(n + 1, 255).astype(np.uint8)
    return dict(radiance=out, moments=moments, variance=variance, hlen=hlen, q=(fx, fy), valid=valid, weights=weights, n_prev=n, near=near,
                alpha=a, moved=moved, frozen=frozen, tap_ids_equal=tap_ids_equal)


# ---- ids for G-buffers that come without them, object-space paint ----

def scene_triangles(sc):
    """world-space triangles of a scene in float64 -> (v0, e1, e2 [n, 3], geometry index [n])"""
    v0, e1, e2, gi = [], [], [], []
    for k, geo in enumerate(sc.geometries):
        M = np.asarray(geo["M"], np.float64)
        P = np.asarray(geo["positions"], np.float64) @ M[:3, :3] + M[3, :3]
        I = np.asarray(geo["indices"], np.int64).reshape(-1, 3)
        v0.append(P[I[:, 0]]), e1.append(P[I[:, 1]] - P[I[:, 0]]), e2.append(P[I[:, 2]] - P[I[:, 0]])
        gi.append(np.full(len(I), k, np.uint32))
    return np.concatenate(v0), np.concatenate(e1), np.concatenate(e2), np.concatenate(gi)


def primary_ids(sc, cam, W, H):
    """the geometry index of every pixel's primary hit (float64 Moller-Trumbore over all triangles; small scenes only) and its
    distance -> (ids uint32 [H, W] with NO_SUBMESH where nothing is hit, t float64)"""
    c = R.Camera(cam, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ndc_x = (xs + 0.5) / W * 2.0 - 1.0
    ndc_y = 1.0 - (ys + 0.5) / H * 2.0
    xa, ya, za = [np.asarray(v, np.float64) for v in (c.x, c.y, c.z)]
    d = xa * (ndc_x * float(c.sx))[..., None] + ya * (ndc_y * float(c.sy))[..., None] - za
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.asarray(c.eye, np.float64)
    v0, e1, e2, gi = scene_triangles(sc)
    best = np.full((H, W), np.inf)
    ids = np.full((H, W), NO_SUBMESH, np.uint32)
    with np.errstate(all="ignore"):
        for k in range(len(gi)):
            p = np.cross(d, e2[k])
            det = p @ e1[k]
            tv = o - v0[k]
            u = (p @ tv) / det
            q = np.cross(tv, e1[k])
            v = (d @ q) / det
            t = (q @ e2[k]) / det
            hit = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < best)
            best = np.where(hit, t, best)
            ids = np.where(hit, gi[k], ids)
    return ids, best


def object_points64(P_world, ids, geom, M):
    """object-space points (float64) of the pixels showing geometry `geom` under surfaceToWorld M (NaN elsewhere)"""
    Minv = np.linalg.inv(np.asarray(M, np.float64))
    out = P_world @ Minv[:3, :3] + Minv[3, :3]
    out[ids != geom] = np.nan
    return out
