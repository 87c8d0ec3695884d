"""CPU reference of the reprojecting temporal pass (option svgf_reproject; nebulae_amd/csrc/svgf.hip,
svgf_temporal_reproject_kernel).  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

numpy, float32, in the kernel's order of operations: every fmaf of the kernel is a fused multiply-add here too (the product
of two float32 values is exact in float64, so one float64 add and a rounding to float32 give the fused result but for a
double-rounding tie), divisions are IEEE ones on both sides, and the camera basis is built as the library's host code builds
it (camera_basis in neb_internal.h: float32 arithmetic, the C library's tanf).  The tap positions therefore come out bit for
bit as the kernel's; what can still differ is the decoded normals (the kernel's reciprocal square root), which only matter
at the validity thresholds -- `reproject` reports every pixel whose decision lies that close to one.

The two validity constants are read from nebulae_amd/csrc/svgf_reproject.h, their only definition.
"""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np

from oracle import svgf_np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    text = open(os.path.join(ROOT, "nebulae_amd", "csrc", "svgf_reproject.h")).read()
    get = lambda name: F(float(re.search(rf"{name}\s*=\s*([0-9.eE+-]+)f", text).group(1)))  # noqa: E731
    return get("kReprojNormalCos"), get("kReprojPlaneTol")


NORMAL_COS, PLANE_TOL = _constants()
WEIGHT_MIN = F(1e-4)

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]


def fma(a, b, c):
    """float32 fused multiply-add (a * b is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


class Camera:
    """camera_basis() of neb_internal.h in float32 (what neb_gbuffer_raycast and the reprojecting pass see)."""

    def __init__(self, cam, W, H):
        eye, tgt, up = [np.array(list(v), F) for v in (cam.eye, cam.target, cam.up)]

        def norm(v):
            ln = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            return np.array([v[0] / ln, v[1] / ln, v[2] / ln], F)

        z = norm(eye - tgt)
        x = norm(np.array([up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]], F))
        y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]], F)
        self.eye, self.x, self.y, self.z = eye, x, y, z
        tan_half = F(_libm.tanf(float(F(cam.vfov_deg) * (F(3.14159265) / F(180.0)) * F(0.5))))
        aspect = F(W) / F(H)
        self.sx, self.sy = aspect * tan_half, tan_half
        zn, zf = F(cam.znear), F(cam.zfar)
        self.m22 = zf / (zn - zf)
        self.m32 = zn * zf / (zn - zf)
        self.W, self.H = W, H


def world_point(c, x, y, d):
    """reproj_world_point: pixel (x, y) (int arrays) at D24 value d (uint32) seen by camera c -> (Px, Py, Pz) float32."""
    inv_W, inv_H = F(1.0) / F(c.W), F(1.0) / F(c.H)
    ndc_x = fma((x.astype(F) + F(0.5)) * inv_W, F(2.0), F(-1.0))
    ndc_y = fma((y.astype(F) + F(0.5)) * inv_H, F(-2.0), F(1.0))
    a, b = ndc_x * c.sx, ndc_y * c.sy
    z = c.m32 / (svgf_np.depth_unorm24(d) + c.m22)
    return tuple(fma(fma(c.x[k], a, fma(c.y[k], b, -c.z[k])), z, c.eye[k]) for k in range(3))


def geometric_normal(normal_f16):
    return svgf_np.oct16_fast_unpack(normal_f16[..., 0:2].astype(F))


def surface(d):
    return (d & np.uint32(0xFFFFFF)) != np.uint32(0xFFFFFF)


def reproject(cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, hlen_hist,
              alpha=0.9, variance_eps=1e-4):
    """One reprojecting temporal pass.  cam_cur / cam_hist: Camera (cam_hist None: no history anywhere).
    Returns dict(radiance, moments, variance, hlen) over the whole plane (the floored remainder keeps radiance[cur], zeros elsewhere)
    and diagnostics over the dispatch region: q = (fx, fy) (tap position - 0.5), valid [4, Hd, Wd], weights [4, Hd, Wd],
    n_prev, near (pixels whose decision lies within 1e-4 of a threshold)."""
    H, W = depth_cur.shape
    Hd, Wd = (H // 8) * 8, (W // 8) * 8
    alpha, variance_eps = F(alpha), F(variance_eps)
    ys, xs = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
    s = (slice(0, Hd), slice(0, Wd))
    Cc = rad_cur[s].astype(F)
    dc = depth_cur[s]
    has = surface(dc) & (cam_hist is not None)
    Ng = geometric_normal(normal_cur[s])
    near = np.zeros((Hd, Wd), bool)
    valid = np.zeros((4, Hd, Wd), bool)
    weights = np.zeros((4, Hd, Wd), F)
    sw = np.zeros((Hd, Wd), F)
    acc = np.zeros((Hd, Wd, 3), F)
    m0 = np.zeros((Hd, Wd), F)
    m1 = np.zeros((Hd, Wd), F)
    n = np.zeros((Hd, Wd), np.uint32)
    fx = np.full((Hd, Wd), np.nan, F)
    fy = np.full((Hd, Wd), np.nan, F)
    if cam_hist is not None:
        ch = cam_hist
        P = world_point(cam_cur, xs, ys, dc)
        r = [P[k] - ch.eye[k] for k in range(3)]
        zl = -fma(r[2], ch.z[2], fma(r[1], ch.z[1], r[0] * ch.z[0]))
        cx = fma(r[2], ch.x[2], fma(r[1], ch.x[1], r[0] * ch.x[0]))
        cy = fma(r[2], ch.y[2], fma(r[1], ch.y[1], r[0] * ch.y[0]))
        with np.errstate(all="ignore"):
            ndc_x, ndc_y = cx / (zl * ch.sx), cy / (zl * ch.sy)
            half_W, half_H = F(0.5) * F(W), F(0.5) * F(H)
            fx = fma(ndc_x, half_W, half_W) - F(0.5)
            fy = fma(-ndc_y, half_H, half_H) - F(0.5)
            inside = has & (zl > 0) & (fx > -1) & (fx < Wd) & (fy > -1) & (fy < Hd)
            x0f, y0f = np.floor(np.where(inside, fx, 0)), np.floor(np.where(inside, fy, 0))
        wx, wy = np.where(inside, fx, 0) - x0f, np.where(inside, fy, 0) - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = PLANE_TOL * zl
        for t in range(4):
            px, py = x0 + (t & 1), y0 + (t >> 1)
            inb = inside & (px >= 0) & (px < Wd) & (py >= 0) & (py < Hd)
            pxc, pyc = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
            dt = depth_hist[pyc, pxc]
            ok = inb & surface(dt)
            Nt = geometric_normal(normal_hist[pyc, pxc])
            dot = fma(Ng[..., 2], Nt[..., 2], fma(Ng[..., 1], Nt[..., 1], Ng[..., 0] * Nt[..., 0]))
            near |= ok & (np.abs(dot - NORMAL_COS) <= 1e-4)
            ok &= dot >= NORMAL_COS
            Pt = world_point(ch, pxc, pyc, dt)
            with np.errstate(all="ignore"):
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
    # temporal_accumulate / temporal_moments_f (svgf.hip)
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
    return dict(radiance=out, moments=moments, variance=variance, hlen=hlen, q=(fx, fy), valid=valid, weights=weights,
                n_prev=n, near=near, alpha=a)


# ---- float64 helpers for tests: world points of a G-buffer, a smooth function painted on the world ----

def world_points64(cam, depth):
    """float64 world point of every pixel of a G-buffer (NaN where there is no surface)."""
    H, W = depth.shape
    c = Camera(cam, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ex, xa, ya, za = [np.asarray(v, np.float64) for v in (c.eye, c.x, c.y, c.z)]
    ndc_x = (xs + 0.5) / W * 2.0 - 1.0
    ndc_y = 1.0 - (ys + 0.5) / H * 2.0
    d = (depth & 0xFFFFFF).astype(np.float64) / 16777215.0
    z = float(c.m32) / (d + float(c.m22))
    v = xa * (ndc_x * float(c.sx))[..., None] + ya * (ndc_y * float(c.sy))[..., None] - za
    P = ex + v * z[..., None]
    P[~surface(depth)] = np.nan
    return P


def paint(P):
    """a smooth, strictly positive RGB function of the world point (slow enough that bilinear resampling across the ~0.3 world units
    between neighbouring pixels of a grazing cornell-box wall at 96 x 64 stays within 1e-3)"""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    r = 1.0 + 0.5 * np.sin(0.25 * x + 0.1 * y) * np.cos(0.2 * z)
    g = 1.2 + 0.4 * np.cos(0.15 * x - 0.25 * z + 0.05 * y)
    b = 0.8 + 0.3 * np.sin(0.2 * y + 0.1 * z)
    out = np.zeros(P.shape[:-1] + (4,), np.float32)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = r, g, b, 1.0
    return np.nan_to_num(out)
