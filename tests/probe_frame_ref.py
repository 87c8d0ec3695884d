"""The reference of neb_gbuffer_points / neb_gi_probe_indirect.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
tests/test_probe_frame_cpu.py shows on the CPU that it is right and able to fail; tests/test_probe_frame_gpu.py judges the device with it.

What lives here.
* The decode of the G-buffer planes into the gather's points in numpy float32: fp16 -> float32 is exact, the shading normal is
  oracle/gi_np.py's oct16_fast_unpack (the restatement the oracle already has; oct_unpack32 below writes the sum's order out and the CPU
  test holds the two to the same bits), the sky rule is the stencil byte.
* The indirect term  r + ((k * E) * (1 / pi))  in numpy float32, one IEEE operation per step: what the device must give bit for bit
  once E is the device's own gather of those points (judge_identity).  On the CPU E comes from probe_volume_ref.gather32.
* NEB_INDIRECT_FRAME_WEIGHT: the factor 2 - pd written once and run in float32 and float64.  The device is judged against float64
  under probe_volume_ref's rule: the tolerance is FOUR TIMES the largest error the float32 restatement shows against float64 on the
  GPU test's own planes (MEASURED, held to the measurement by test_probe_frame_cpu.test_calibration), in units of max(1, |word|).
* The synthetic G-buffers of the GPU test, on probe_volume_ref's grids (origin and spacing powers of two and small: a position inside
  a cell survives the rounding to fp16 inside that cell)."""
import numpy as np

import probe_volume_ref as PV
from nebulae_amd import _lib
from oracle import gi_np

F, F64, U32 = np.float32, np.float64, np.uint32
PI32 = F(3.14159265)
INV_PI32 = F(1.0) / PI32  # the library's kPiInv: one float32 division
TMIN = F(0.01)
# frame_weighted(float32) against frame_weighted(float64) under judge_weighted, test_probe_frame_cpu.test_calibration: the largest error
# of a radiance word in units of max(1, |word|) over KINDS x the two grids at 70 x 45, rounded up from 5.916e-07.  That is some five ulp
# of 1: the factor's chain (a normalisation, x^5, two luminances, a division) on top of three products and a sum, of words of size 1..4.
MEASURED = dict(frame_weight=6.0e-7)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
KINDS = ("uniform", "permuted", "stray", "special")
SIZES = ((70, 45), (8, 8), (1, 1))  # (width, height): neither a multiple of 8; one tile exactly; one pixel
GRIDS = ((1, 1, 1), (5, 4, 3))
CAMERA = (0.4, 1.9, 2.6)
CORRUPTIONS = ("1 / pi dropped", "metalness ignored", "sky pixels lit", "alpha written", "x and y transposed", "a NO_PROBE pixel stored to",
               "geometric normal used")


# ------------------------------------------------------------------------------------------------
# the planes -> points
# ------------------------------------------------------------------------------------------------
def oct_unpack32(e):
    """gi_device.h's oct_unpack (FAST = false) on float32 pairs [..., 2], the order of every sum written out"""
    e = np.asarray(e, F)
    with np.errstate(all="ignore"):
        x, y = e[..., 0], e[..., 1]
        z = ((F(1.0) - np.abs(x)).astype(F) - np.abs(y)).astype(F)
        sx, sy = np.where(x > 0, F(1.0), F(-1.0)), np.where(y > 0, F(1.0), F(-1.0))
        nx, ny = ((F(1.0) - np.abs(y)) * sx).astype(F), ((F(1.0) - np.abs(x)) * sy).astype(F)
        x, y = np.where(z < 0, nx, x), np.where(z < 0, ny, y)
        length = np.sqrt(((x * x + y * y).astype(F) + z * z).astype(F))
        return np.stack([x / length, y / length, z / length], -1).astype(F)


def sky(planes):
    return (planes["depth"] >> U32(24)) == 0


def points32(planes, geometric_normal=False):
    """what neb_gbuffer_points writes for the whole frame: float32 [h * w, 8]"""
    h, w = planes["depth"].shape
    out = np.zeros((h, w, 8), F)
    lit = ~sky(planes)
    with np.errstate(all="ignore"):
        out[..., 0:3] = np.where(lit[..., None], planes["world_pos"][..., 0:3].astype(F), F(0))
        pair = planes["normal"][..., 0:2] if geometric_normal else planes["normal"][..., 2:4]
        out[..., 4:7] = np.where(lit[..., None], gi_np.oct16_fast_unpack(pair.astype(F)), F(0))
    out[..., 3], out[..., 7] = TMIN, np.inf
    return out.reshape(h * w, 8)


def diffuse_k(planes, T=F):
    """albedo * (1 - metalness), [h, w, 3] of type T (the decodes are exact in either)"""
    with np.errstate(all="ignore"):
        albedo = gi_np.unpack_r11g11b10(planes["albedo"]).astype(T)
        return albedo * (T(1.0) - planes["rough_metal"][..., 1].astype(T))[..., None]


# ------------------------------------------------------------------------------------------------
# the indirect term
# ------------------------------------------------------------------------------------------------
def stored(gathered):
    """the pixels the call stores to: gathered, and some probe counted"""
    return (np.asarray(gathered["flags"]) & U32(_lib.GATHER_NOT_GATHERED | _lib.GATHER_NO_PROBE)) == 0


def indirect32(radiance, planes, gathered, corrupt=None):
    """radiance [h, w, 4] float32 after neb_gi_probe_indirect without flags, E = gathered["irradiance"] [h * w, 3] float32 taken as
    given; `corrupt`: one of CORRUPTIONS (but the normal's, which acts on the points), for the tests of the judge"""
    assert corrupt is None or corrupt in CORRUPTIONS
    h, w = planes["depth"].shape
    E = np.asarray(gathered["irradiance"], F).reshape(h, w, 3)
    mask = stored(gathered).reshape(h, w)
    if corrupt == "x and y transposed":
        E, mask = np.ascontiguousarray(E.reshape(w, h, 3).transpose(1, 0, 2)), np.ascontiguousarray(mask.reshape(w, h).T)
    if corrupt == "sky pixels lit":
        mask = mask | sky(planes)
        E = np.where(sky(planes)[..., None], F(1.0), E)
    if corrupt == "a NO_PROBE pixel stored to":
        mask = mask | ((np.asarray(gathered["flags"]) & U32(_lib.GATHER_NO_PROBE)) != 0).reshape(h, w)
    with np.errstate(all="ignore"):
        k = diffuse_k(planes)
        if corrupt == "metalness ignored":
            k = gi_np.unpack_r11g11b10(planes["albedo"])
        add = (k * E).astype(F)
        if corrupt != "1 / pi dropped":
            add = (add * INV_PI32).astype(F)
        out = radiance.copy()
        lit = (radiance[..., 0:3] + add).astype(F)
        out[..., 0:3] = np.where(mask[..., None], lit, radiance[..., 0:3])
        if corrupt == "alpha written":
            out[..., 3] = np.where(mask, F(1.0), radiance[..., 3])
    return out


def judge_identity(got, radiance, planes, gathered, name):
    """the plane after the call against indirect32 of the plane before it: every bit, the alpha and the pixels not stored to included"""
    want = indirect32(radiance, planes, gathered)
    a, b = np.ascontiguousarray(got, F).view(U32), want.view(U32)
    bad = np.argwhere((a != b).any(-1))
    assert bad.size == 0, f"{name}: {len(bad)} pixels differ; first (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    keep = ~stored(gathered).reshape(planes["depth"].shape)
    assert np.array_equal(a[keep], np.ascontiguousarray(radiance, F).view(U32)[keep]), f"{name}: a pixel that is not stored to changed"
    assert np.array_equal(a[..., 3], np.ascontiguousarray(radiance, F).view(U32)[..., 3]), f"{name}: alpha changed"
    return int(stored(gathered).sum())


def frame_factor(planes, camera, T):
    """2 - pd per pixel [h, w] in type T: gi_raygen's pd = 1 - Brdf_GetSpecularProbability(saturate(dot(normalize(V), SN)), F0, albedo)"""
    with np.errstate(all="ignore"):
        pts = points32(planes).reshape(planes["depth"].shape + (8,))
        P, SN = pts[..., 0:3].astype(T), pts[..., 4:7].astype(T)
        albedo = gi_np.unpack_r11g11b10(planes["albedo"]).astype(T)
        metal = planes["rough_metal"][..., 1].astype(T)[..., None]
        V = np.asarray(camera, F).astype(T) - P
        Vn = V / np.sqrt((V[..., 0] * V[..., 0] + V[..., 1] * V[..., 1]) + V[..., 2] * V[..., 2])[..., None]
        vdotn = np.clip((Vn[..., 0] * SN[..., 0] + Vn[..., 1] * SN[..., 1]) + Vn[..., 2] * SN[..., 2], T(0), T(1))
        f0 = T(0.04) + metal * (albedo - T(0.04))

        def lum(c):
            return (c[..., 0] * T(F(0.2126)) + c[..., 1] * T(F(0.7152))) + c[..., 2] * T(F(0.0722))
        x2 = vdotn * vdotn
        k = (T(1) - (x2 * x2) * vdotn)[..., None]
        fres = np.clip(lum(f0 + (T(1) - f0) * k), T(0), T(1))
        diff = lum(albedo) * (T(1) - fres)
        p = np.clip(diff / np.maximum(T(F(0.0001)), fres + diff), T(F(0.1)), T(F(0.9)))
        pd = T(1) - p
        out = np.where(pd > 0, T(2) - pd, T(1))
    assert out.dtype == T
    return out


def frame_weighted(radiance, planes, gathered, camera, T):
    """the plane after the call with NEB_INDIRECT_FRAME_WEIGHT, every number of type T; the pixels not stored to keep radiance's value"""
    h, w = planes["depth"].shape
    E = np.asarray(gathered["irradiance"], F).reshape(h, w, 3).astype(T)
    mask = stored(gathered).reshape(h, w)
    with np.errstate(all="ignore"):
        k = diffuse_k(planes, T) * frame_factor(planes, camera, T)[..., None]
        inv_pi = INV_PI32 if T is F else T(1.0) / T(F(3.14159265))
        out = radiance.astype(T)
        out[..., 0:3] = np.where(mask[..., None], out[..., 0:3] + (k * E) * inv_pi, out[..., 0:3])
    assert out.dtype == T
    return out


def judge_weighted(got, radiance, planes, gathered, camera, name, tol=None):
    """`got` against the float64 statement within tol (default TOL) in units of max(1, |word|) -> the largest such error; the pixels
    not stored to and the alpha keep their bits"""
    tol = TOL["frame_weight"] if tol is None else tol
    want = frame_weighted(radiance, planes, gathered, camera, F64)
    mask = stored(gathered).reshape(planes["depth"].shape)
    a = np.asarray(got)
    if a.dtype == F:
        before = np.ascontiguousarray(radiance, F).view(U32)
        assert np.array_equal(a.view(U32)[~mask], before[~mask]), f"{name}: a pixel that is not stored to changed"
        assert np.array_equal(a.view(U32)[..., 3], before[..., 3]), f"{name}: alpha changed"
    if not mask.any():
        return 0.0
    x, y = a[mask][:, 0:3].astype(F64), want[mask][:, 0:3]
    assert np.isfinite(x).all(), f"{name}: a stored word is not finite"
    err = float((np.abs(x - y) / np.maximum(1.0, np.abs(y))).max())
    assert err <= tol, f"{name}: radiance is off by {err:.3e}, tolerance {tol:.1e}"
    return err


# ------------------------------------------------------------------------------------------------
# the synthetic G-buffers of the GPU test (and of the calibration)
# ------------------------------------------------------------------------------------------------
def _r11g11b10(rng, shape):
    """random finite colours 2^-4 .. 2: exponent fields 11..15, any mantissa"""
    e = rng.integers(11, 16, shape + (3,)).astype(U32)
    m = rng.integers(0, 64, shape + (3,)).astype(U32)
    return (e[..., 0] << U32(6) | m[..., 0]) | ((e[..., 1] << U32(6) | m[..., 1]) << U32(11)) | ((e[..., 2] << U32(5) | (m[..., 2] >> U32(1))) << U32(22))


def synthetic_gbuffer(g, kind, w, h, seed=3):
    """planes {depth uint32 [h, w], world_pos fp16 [h, w, 4], normal fp16 [h, w, 4], albedo uint32 [h, w], rough_metal fp16 [h, w, 2]}
    on grid g.  uniform: the pixels of an 8 x 8 tile share a cell (the kernel's scalar-load arm); permuted: a cell of its own per pixel
    (the per-lane arm); stray: uniform but for pixel (1, 2) of every tile; special: by turns stencil 0, an fp16 infinity and a NaN in
    the position, a zero oct normal, positions below and above the grid, the cell without a valid probe, and plain pixels between."""
    assert kind in KINDS
    rng = np.random.default_rng(seed + 11 * KINDS.index(kind) + w + 131 * h)
    dims = np.array([int(d) for d in g["dims"]])
    cells = np.maximum(dims - 1, 1)
    ys, xs = np.mgrid[0:h, 0:w]
    tile = (ys // 8) * ((w + 7) // 8) + xs // 8
    per_tile = np.floor(rng.uniform(0, 1, (int(tile.max()) + 1, 3)) * cells)
    per_pixel = np.floor(rng.uniform(0, 1, (h, w, 3)) * cells)
    base = per_pixel if kind in ("permuted", "special") else per_tile[tile]
    if kind == "stray":
        lone = (xs % 8 == 1) & (ys % 8 == 2)
        base[lone] = (base[lone] + 1) % cells
    inside = np.where(dims > 1, rng.uniform(0.1, 0.9, (h, w, 3)), rng.uniform(-0.5, 0.5, (h, w, 3)))
    t = base + inside
    turn = (xs + 3 * ys) % 16 if kind == "special" else np.full((h, w), -1)
    t[turn == 4] = -0.75
    t[turn == 5] = (dims - 1 + 0.625)
    if tuple(dims) == (5, 4, 3):
        t[turn == 6] = np.array(PV.DEAD_CELL) + inside[turn == 6]
    p = np.zeros((h, w, 4), np.float16)
    p[..., 0:3] = (g["origin"].astype(F64) + t * g["spacing"].astype(F64)).astype(np.float16)
    p[..., 3] = 1.0
    p[..., 0][turn == 1] = np.inf
    p[..., 2][turn == 2] = np.nan
    n = rng.uniform(-1.0, 1.0, (h, w, 4)).astype(np.float16)  # (any pair of fp16 in -1..1 is an oct normal; .xy and .zw are independent)
    n[..., 2:4][turn == 3] = 0.0
    depth = (rng.integers(1, 1 << 24, (h, w)).astype(U32)) | U32(1 << 24)
    depth[turn == 0] &= U32(0x00FFFFFF)
    rm = rng.uniform(0.0, 1.0, (h, w, 2)).astype(np.float16)
    rm[..., 1][(xs + ys) % 5 == 0] = 1.0  # metals: nothing is added
    rm[..., 1][(xs + ys) % 5 == 1] = 0.0
    return dict(depth=depth, world_pos=p, normal=n, albedo=_r11g11b10(rng, (h, w)), rough_metal=rm)


def random_radiance(w, h, seed=9):
    """the plane the calls add to: words of both signs, a third of the green words -0"""
    rng = np.random.default_rng(seed + w + 131 * h)
    out = (rng.standard_normal((h, w, 4)) * 2.0).astype(F)
    ys, xs = np.mgrid[0:h, 0:w]
    out[..., 1][(xs + ys) % 3 == 0] = -0.0  # (-0 + 0 is +0: a store of "radiance + 0" to a pixel that is to be left alone shows)
    return out
