"""CPU reference of albedo demodulation (option svgf_demodulate; nebulae_amd/csrc/svgf_demod.h).  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

It adds nothing to the references it composes -- the C oracle's temporal + a-trous passes (oracle_lib.OracleSVGF) and the reprojecting
passes of reproject_ref / motion_ref / vertex_motion_ref, all unchanged: they are fed float32(radiance / d) as the current radiance and
the demodulated history as their history, and what they return is {demod, float32(demod * d)}.  d = max(albedo, floor) per channel from
this file's own R11G11B10_FLOAT decode; the floor is read from svgf_demod.h, its only definition.  Division and product are IEEE float32
ones (numpy's are correctly rounded), as the kernels' are.
"""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _floor():
    text = open(os.path.join(ROOT, "nebulae_amd", "csrc", "svgf_demod.h")).read()
    return F(float(re.search(r"kDemodFloor\s*=\s*([0-9.eE+-]+)f", text).group(1)))


FLOOR = _floor()


def small_float(bits, mbits):
    """an unsigned small float, 5-bit exponent (bias 15), `mbits` of mantissa -> float32"""
    bits = np.asarray(bits, np.uint32)
    e, m = (bits >> np.uint32(mbits)).astype(np.int64), (bits & np.uint32((1 << mbits) - 1)).astype(np.float64)
    frac = m / float(1 << mbits)
    with np.errstate(over="ignore"):
        val = np.where(e == 0, np.ldexp(frac, -14), np.ldexp(1.0 + frac, np.clip(e, 1, 30) - 15))
        val = np.where(e == 31, np.where(m == 0, np.inf, np.nan), val)
    return val.astype(F)


def decode_r11g11b10(words):
    """R11G11B10_FLOAT words [...] -> float32 [..., 3]"""
    w = np.asarray(words, np.uint32)
    return np.stack([small_float(w & np.uint32(0x7FF), 6), small_float((w >> np.uint32(11)) & np.uint32(0x7FF), 6),
                     small_float((w >> np.uint32(22)) & np.uint32(0x3FF), 5)], axis=-1)


def divisor(albedo_words):
    """d = fmaxf(albedo, floor) per channel (a NaN field takes the floor, as fmaxf does)"""
    return np.fmax(decode_r11g11b10(albedo_words), FLOOR).astype(F)


def demodulate(rad, d):
    out = np.array(rad, F, copy=True)
    with np.errstate(all="ignore"):
        out[..., :3] = out[..., :3] / d
    return out


def remodulate(demod, d):
    out = np.array(demod, F, copy=True)
    out[..., :3] = out[..., :3] * d
    return out


def random_albedo(rng, H, W):
    """random R11G11B10_FLOAT words: exponents 2^-8 .. 2^1 with random mantissas (so below the floor, between, and above 1), and one pixel
    in eight with a field that is exactly zero"""
    def field(mbits):
        e = rng.integers(7, 17, (H, W)).astype(np.uint32)
        m = rng.integers(0, 1 << mbits, (H, W)).astype(np.uint32)
        f = (e << np.uint32(mbits)) | m
        return np.where(rng.integers(0, 8, (H, W)) == 0, np.uint32(0), f).astype(np.uint32)
    return (field(6) | (field(6) << np.uint32(11)) | (field(5) << np.uint32(22))).astype(np.uint32)


class DemodSVGF:
    """The same-pixel chain: the C oracle run on demodulated planes.  Its radiance[hist] IS the demod plane (the oracle's own denoised
    output of the frame before is the demodulated colour), unless `history` replaces it (the seed: demodulate(radiance[hist], d))."""

    def __init__(self, W, H, levels, **kw):
        from oracle_lib import OracleSVGF
        self.o = OracleSVGF(W, H, levels, **kw)
        self.d = None

    def begin_frame(self, f, depth, normal, rad, albedo, history=None):
        o = self.o
        o.begin_frame(f)
        self.d = divisor(albedo)
        o.depth[o.cur][...] = depth
        o.normal[o.cur][...] = normal
        o.radiance[o.cur][...] = demodulate(rad, self.d)
        if history is not None:
            o.radiance[o.hist][...] = history

    def temporal(self):
        """-> the accumulated demodulated colour (what radiance[cur] holds after the temporal call), moments, variance"""
        o = self.o
        o.temporal_pass()
        return dict(radiance=o.radiance[o.cur].copy(), moments=o.moments[o.cur].copy(), variance=o.variance.copy())

    def atrous(self):
        o = self.o
        o.atrous_pass()
        demod = o.radiance[o.cur].copy()
        return dict(demod=demod, radiance=remodulate(demod, self.d))

    def close(self):
        self.o.close()


def reproject(ref_fn, cam_cur, cam_hist, rad_cur, demod_hist, albedo, *rest, **kw):
    """a reprojecting temporal pass (reproject_ref.reproject, motion_ref.reproject or vertex_motion_ref.reproject as `ref_fn`, `rest` =
    its arguments behind rad_hist) on the demodulated current radiance and the demod plane as history"""
    return ref_fn(cam_cur, cam_hist, demodulate(rad_cur, divisor(albedo)), np.asarray(demod_hist, F), *rest, **kw)
