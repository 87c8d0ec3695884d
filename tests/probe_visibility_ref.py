"""The reference of neb_gi_bake_visibility / neb_gi_accumulate_visibility / neb_gi_gather_probes_visible.  TEST
INFRASTRUCTURE, NOT PRODUCT CODE.  tests/test_probe_visibility_cpu.py shows on the CPU that it is right and able to fail;
tests/test_probe_visibility_gpu.py judges the device with it.

What lives here, each written ONCE in the order include/nebulae_hip.h gives and run in float64 (the judge's reference) and in numpy float32
(the restatement: numpy's float32 `+ - * /`, sqrt and floor are IEEE operations, so it follows the header step by step and must give
the device's BITS).
* The bake as a reduction over given (direction, t, hit) arrays -- what neb_gi_cast_rays answers for the rays of neb_gi_probe_rays.
* The accumulation, with the bound the device's float32 running mean must stay inside (Accumulator64, derived at accumulate64).
* The visible gather: probe_volume_ref's gather with the Chebyshev factor per corner.  With maps that see everything it is
  probe_volume_ref.gather32 bit for bit (the CPU test asserts it), so the two texts cannot drift apart unnoticed.
* The tolerances: FOUR TIMES the largest error the float32 restatement shows against the float64 one on the GPU test's own inputs
  (MEASURED, held to the measurement by test_probe_visibility_cpu.test_calibration: the rule of probe_volume_ref.MEASURED).
* The inputs of the GPU test: probe_volume_ref's grids, records and point sets, random maps, and the leak fixture."""
import numpy as np

import probe_volume_ref as PV
from nebulae_amd import _lib
from probe_ref import K00, K1, K2A, K20, K22, RECORD

F, F64, U32 = np.float32, np.float64, np.uint32
VISIBILITY = np.dtype([("moments", F, (64, 2)), ("weight", F, (64,))])
assert VISIBILITY.itemsize == 768
# float32 against float64 of this file, test_probe_visibility_cpu.test_calibration:
#   gather: the largest error of an irradiance or weight word in units of max(1, |word|) (probe_volume_ref.judge_gather) over the four
#     grids, the five point counts and the three point kinds with random_maps, rounded up from 1.2145e-05.  Above the plain gather's
#     2.4e-6: var = m2 - m1 m1 cancels, and the factor is cubed.
#   bake: the largest error of a moment in units of max(1, |moment|), and of a weight in units of max(1, weight), over synthetic_samples,
#     rounded up from 2.947e-06 (S = 256 sequential float32 additions).
MEASURED = dict(gather=1.22e-5, bake=2.95e-6)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
CORRUPTIONS = ("fold sign dropped", "wrap replaced by clamp", "moments swapped", "r taken to the unbiased point", "floor 0.05 dropped", "cube dropped",
               "sample order reversed")
GATHER_CORRUPTIONS = CORRUPTIONS[:6]  # (the last one is the bake's)


# ------------------------------------------------------------------------------------------------
# the map
# ------------------------------------------------------------------------------------------------
def _sgn(x, T):
    return np.where(x >= 0, T(1), T(-1))  # sgn(0) = +1


def texel_directions(T=F64):
    """[64, 3] in T: n_k of texel k = i + 8 j, by the header's operations"""
    k = np.arange(64)
    ex = ((k % 8).astype(T) + T(0.5)) / T(8) * T(2) - T(1)
    ey = ((k // 8).astype(T) + T(0.5)) / T(8) * T(2) - T(1)
    vz = (T(1) - np.abs(ex)) - np.abs(ey)
    fold = vz < 0
    vx = np.where(fold, (T(1) - np.abs(ey)) * _sgn(ex, T), ex)
    vy = np.where(fold, (T(1) - np.abs(ex)) * _sgn(ey, T), ey)
    length = np.sqrt((vx * vx + vy * vy) + vz * vz)
    out = np.stack([vx / length, vy / length, vz / length], -1)
    assert out.dtype == T
    return out


def wrap(a, b, corrupt=None):
    """integer tap indices, each in -1 .. 8 -> the texel index a + 8 b after the octahedral wrap, x first and then y"""
    a, b = np.asarray(a).copy(), np.asarray(b).copy()
    if corrupt == "wrap replaced by clamp":
        return np.clip(a, 0, 7) + 8 * np.clip(b, 0, 7)
    out = (a < 0) | (a > 7)
    a, b = np.clip(a, 0, 7), np.where(out, 7 - b, b)
    out = (b < 0) | (b > 7)
    b, a = np.clip(b, 0, 7), np.where(out, 7 - a, a)
    return a + 8 * b


def lookup(u, T=F64, corrupt=None):
    """u [n, 3] in T, none of zero length -> (four tap indices [4, n] in the order t00 t10 t01 t11, fx, fy): the header's octahedral lookup"""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    s = (np.abs(ux) + np.abs(uy)) + np.abs(uz)
    ox, oy = ux / s, uy / s
    fold = uz < 0
    sx, sy = (T(1), T(1)) if corrupt == "fold sign dropped" else (_sgn(ox, T), _sgn(oy, T))
    ox, oy = np.where(fold, (T(1) - np.abs(oy)) * sx, ox), np.where(fold, (T(1) - np.abs(ox)) * sy, oy)
    tx, ty = ox * T(4) + T(3.5), oy * T(4) + T(3.5)
    flx, fly = np.floor(tx), np.floor(ty)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    assert ix.min(initial=0) >= -1 and ix.max(initial=0) <= 7 and iy.min(initial=0) >= -1 and iy.max(initial=0) <= 7
    taps = np.stack([wrap(ix, iy, corrupt), wrap(ix + 1, iy, corrupt), wrap(ix, iy + 1, corrupt), wrap(ix + 1, iy + 1, corrupt)])
    return taps, tx - flx, ty - fly


def visibility_factor(moments, u, T=F64, corrupt=None, parts=None):
    """moments [n, 64, 2] (each row: the map of the probe the row asks), u [n, 3] = biased point - probe, both in T -> vis [n] in T.
    `parts`: a dict that receives branch (0: rr == 0, 1: r <= m1, 2: Chebyshev above the floor, 3: the floor) and the blended m1"""
    n = len(u)
    rr = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    zero = rr == 0
    safe = np.where(zero[:, None], T(1), u)
    r = np.sqrt(np.where(zero, T(1), rr))
    taps, fx, fy = lookup(safe, T, corrupt)
    rows = np.arange(n)
    t00, t10, t01, t11 = (moments[rows, taps[q]] for q in range(4))
    gx, gy = T(1) - fx, T(1) - fy
    m = ((gx[:, None] * t00 + fx[:, None] * t10) * gy[:, None]) + ((gx[:, None] * t01 + fx[:, None] * t11) * fy[:, None])
    m1, m2 = (m[:, 1], m[:, 0]) if corrupt == "moments swapped" else (m[:, 0], m[:, 1])
    var = np.maximum(m2 - m1 * m1, T(2.0 ** -10) * m2)
    over = r - m1
    cheb = np.where(r > m1, var / (var + over * over), T(1))
    cube = cheb if corrupt == "cube dropped" else (cheb * cheb) * cheb
    vis = cube if corrupt == "floor 0.05 dropped" else np.maximum(T(0.05), cube)
    vis = np.where(zero, T(1), vis)
    if parts is not None:
        parts["branch"] = np.where(zero, 0, np.where(~(r > m1), 1, np.where(cube > T(0.05), 2, 3)))
        parts["m1"] = m1
    assert vis.dtype == T
    return vis


# ------------------------------------------------------------------------------------------------
# the bake as a reduction
# ------------------------------------------------------------------------------------------------
def baked(probes):
    """neb_gi_bake_probes' rule under NEB_BAKE_SH, in float32"""
    pr = np.asarray(probes, F)
    with np.errstate(all="ignore"):
        pp = ((pr[:, 0] * pr[:, 0] + pr[:, 1] * pr[:, 1]).astype(F) + pr[:, 2] * pr[:, 2]).astype(F)
        return (pp < np.inf) & (pr[:, 3] >= 0) & (pr[:, 7] > pr[:, 3])


def bake_reduce(directions, t, hit, max_distance, T=F64, is_baked=None, corrupt=None):
    """directions [n, S, 3] float32, t [n, S], hit [n, S] bool: the answers of the closest-hit walk over the rays of the n probes ->
    a VISIBILITY-like dict, moments [n, 64, 2] and weight [n, 64] in T: the sequential sums of the header, in sample order"""
    d, tt = np.asarray(directions, F).astype(T), np.asarray(t, F).astype(T)
    n, S = tt.shape
    D = T(F(max_distance))
    with np.errstate(all="ignore"):
        dist = np.where(np.asarray(hit, bool), np.minimum(tt, D), D)
        nk = texel_directions(T)
        A, M1, M2 = (np.zeros((n, 64), T) for _ in range(3))
        order = range(S - 1, -1, -1) if corrupt == "sample order reversed" else range(S)
        for s in order:
            c = (nk[None, :, 0] * d[:, s, None, 0] + nk[None, :, 1] * d[:, s, None, 1]) + nk[None, :, 2] * d[:, s, None, 2]
            g = c
            for _ in range(5):
                g = g * g
            counts = ~(c < T(0.25))
            ds = dist[:, s, None]
            A = np.where(counts, A + g, A)
            M1 = np.where(counts, M1 + g * ds, M1)
            M2 = np.where(counts, M2 + g * (ds * ds), M2)
        filled = A > 0
        if is_baked is not None:
            filled &= np.asarray(is_baked, bool)[:, None]
        safe = np.where(filled, A, T(1))
        moments = np.stack([np.where(filled, M1 / safe, D), np.where(filled, M2 / safe, D * D)], -1)
        weight = np.where(filled, A, T(0))
    assert moments.dtype == T and weight.dtype == T
    return dict(moments=moments, weight=weight)


def as_array(v):
    """a float32 dict of bake_reduce -> a VISIBILITY array, the device's buffer"""
    out = np.zeros(len(v["weight"]), VISIBILITY)
    out["moments"], out["weight"] = v["moments"], v["weight"]
    return out


def all_visible(n, D):
    """n maps whose every texel is (D, D^2)"""
    out = np.zeros(n, VISIBILITY)
    out["moments"][..., 0], out["moments"][..., 1], out["weight"] = F(D), F(D) * F(D), 1.0
    return out


def judge_bake(got, want, name, tol=None):
    """a VISIBILITY array or dict against bake_reduce's float64 dict -> the largest error in units of max(1, |word|)"""
    tol = TOL["bake"] if tol is None else tol
    worst = 0.0
    for k in ("moments", "weight"):
        a, b = np.asarray(got[k], F64), np.asarray(want[k], F64)
        assert np.isfinite(a).all(), f"{name}: {k} is not finite"
        err = float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(initial=0.0))
        assert err <= tol, f"{name}: {k} is off by {err:.3e}, tolerance {tol:.1e}"
        worst = max(worst, err)
    return worst


def synthetic_samples(n=6, S=256, seed=11):
    """(directions float32 [n, S, 3] of unit length, t [n, S], hit [n, S], max_distance): what a walk could answer, with hits beyond
    max_distance and misses"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, S, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)
    t = rng.uniform(0.05, 2.5, (n, S)).astype(F)
    hit = rng.uniform(size=(n, S)) < 0.8
    return d, np.where(hit, t, F(np.inf)), hit, 1.75


# ------------------------------------------------------------------------------------------------
# the accumulation
# ------------------------------------------------------------------------------------------------
def accumulate64(acc, add, prior_bound=None, acc_value=None, folds=None, acc_weight=None):
    """one step on VISIBILITY arrays -> (a VISIBILITY array: the float32 rounding of the float64 result, moments in float64 [n, 64, 2],
    bound [n, 64, 2], folds [n, 64], weight in float64 [n, 64]); `acc_value`, `acc_weight`: acc's moments and weights in float64, where they
    are known better than acc holds them.  The bound of a blended moment, with e = 2^-24 and k = the blends the texel's weight has been
    through (`folds`): the device's weight wa is a sum of k + 1 positive terms with k roundings, off by at most k e relatively, which
    moves wa / W and wb / W by at most k e; W, the two quotients, a product and the sum are five more roundings on either path, one more
    is margin:  (k + 6) e (|a| fa + |b| fb) + prior fa + 2^-149,  `prior` being what acc's own moments may already be off by."""
    acc, add = np.asarray(acc), np.asarray(add)
    n = len(acc)
    wa, wb = acc["weight"].astype(F64) if acc_weight is None else np.asarray(acc_weight, F64), add["weight"].astype(F64)
    a = acc["moments"].astype(F64) if acc_value is None else np.asarray(acc_value, F64)
    b = add["moments"].astype(F64)
    prior = np.zeros((n, 64, 2)) if prior_bound is None else np.asarray(prior_bound, F64)
    k = np.zeros((n, 64)) if folds is None else np.asarray(folds, F64)
    keep, take = wb == 0, (wa == 0) & (wb != 0)
    blend = ~keep & ~take
    out, value, bound, k_out = acc.copy(), a.copy(), prior.copy(), k.copy()
    out["moments"][take], out["weight"][take], value[take], bound[take], k_out[take] = add["moments"][take], add["weight"][take], b[take], 0.0, 0.0
    W = np.where(blend, wa + wb, 1.0)
    fa, fb = (wa / W)[..., None], (wb / W)[..., None]
    mean = a * fa + b * fb
    step = (k[..., None] + 6.0) * 2.0 ** -24 * (np.abs(a) * fa + np.abs(b) * fb) + prior * fa + 2.0 ** -149
    value[blend], bound[blend], k_out[blend] = mean[blend], step[blend], k[blend] + 1.0
    out["moments"][blend] = mean[blend].astype(F)
    out["weight"][blend] = (acc["weight"] + add["weight"]).astype(F)[blend]  # (the device's own float32 sum: what it must hold, bit for bit)
    weight = np.where(keep, wa, np.where(take, wb, wa + wb))
    return out, value, bound, k_out, weight


class Accumulator64:
    """the float64 running mean of several maps with the bound the device's float32 one must stay inside"""

    def __init__(self, n):
        self.records, self.value, self.bound, self.folds = np.zeros(n, VISIBILITY), np.zeros((n, 64, 2)), np.zeros((n, 64, 2)), np.zeros((n, 64))
        self.weight = np.zeros((n, 64))

    def add(self, maps):
        self.records, self.value, self.bound, self.folds, self.weight = accumulate64(self.records, maps, self.bound, self.value, self.folds, self.weight)
        return self


def judge_accumulation(got, want, value, bound, name):
    """device maps against accumulate64's: weights bit for bit, every moment within its bound -> the largest error in bounds"""
    assert np.array_equal(got["weight"].view(U32), want["weight"].view(U32)), f"{name}: a weight differs"
    err = np.abs(got["moments"].astype(F64) - value)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0))
    assert worst <= 1.0, f"{name}: a moment is {worst:.2f} bounds from the float64 mean"
    return worst


# ------------------------------------------------------------------------------------------------
# the visible gather
# ------------------------------------------------------------------------------------------------
def _gather(g, records, visibility, normal_bias, points, T, corrupt=None, parts=None):
    """probe_volume_ref._gather, its text, with the factor between w_n and w.  `parts`: receives branch [8, n] per corner (-1: the corner
    does not exist or its record is invalid) of visibility_factor"""
    assert corrupt is None or corrupt in GATHER_CORRUPTIONS
    pts, rec = np.asarray(points, F), np.asarray(records)
    n = len(pts)
    ok = PV.usable(pts)
    dims = [int(d) for d in g["dims"]]
    origin, spacing, limit = g["origin"].astype(T), g["spacing"].astype(T), T(g["backface_limit"])
    pos = PV.grid_positions32(g).astype(T)
    sh = rec["sh"].reshape(len(rec), 27).astype(T)
    maps = np.asarray(visibility)["moments"].astype(T)
    bias = T(F(normal_bias))
    samples, backfaces = rec["samples"].astype(T), rec["backfaces"].astype(T)
    branch = np.full((8, n), -1)
    with np.errstate(all="ignore"):
        valid = (rec["samples"] != 0) & ((rec["flags"] & _lib.PROBE_NOT_BAKED) == 0) & ~(backfaces > limit * samples)
        safe = np.where(ok[:, None], pts, F(1.0))  # (rows that are not usable are computed on ones and blanked at the end)
        p, nrm = safe[:, 0:3].astype(T), safe[:, 4:7].astype(T)
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        N = nrm / np.sqrt(nn)[:, None]
        pb = p if corrupt == "r taken to the unbiased point" else p + bias * N
        base, f = np.zeros((n, 3), np.int64), np.zeros((n, 3), T)
        clamped = np.zeros(n, bool)
        for a in range(3):
            t = (p[:, a] - origin[a]) / spacing[a]
            tc = np.minimum(np.maximum(t, T(0)), T(dims[a] - 1))
            clamped |= tc != t
            base[:, a] = np.minimum(np.floor(tc).astype(np.int64), max(dims[a] - 2, 0))
            f[:, a] = tc - base[:, a].astype(T)
        cell = base[:, 0] + dims[0] * (base[:, 1] + dims[1] * base[:, 2])
        w, idx = np.zeros((8, n), T), np.zeros((8, n), np.int64)
        W = np.zeros(n, T)
        for c in range(8):
            bit = (c & 1, (c >> 1) & 1, c >> 2)
            if any(bit[a] and dims[a] < 2 for a in range(3)):
                continue
            k = base + np.array(bit)
            idx[c] = k[:, 0] + dims[0] * (k[:, 1] + dims[1] * k[:, 2])
            side = [f[:, a] if bit[a] else T(1) - f[:, a] for a in range(3)]
            w_tri = (side[0] * side[1]) * side[2]
            v = pos[idx[c]] - p
            vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            dot = (v[:, 0] * N[:, 0] + v[:, 1] * N[:, 1]) + v[:, 2] * N[:, 2]
            d = np.where(vv > 0, dot / np.sqrt(np.where(vv > 0, vv, T(1))), T(0))
            h = (d + T(1)) * T(0.5)
            w_n = h * h + T(0.2)
            sub = {}
            vis = visibility_factor(maps[idx[c]], pb - pos[idx[c]], T, corrupt, sub)
            w[c] = np.where(valid[idx[c]], (w_tri * w_n) * vis, T(0))
            branch[c] = np.where(valid[idx[c]] & ok, sub["branch"], -1)
            W = W + w[c]
        some = W > 0
        r = T(1) / np.where(some, W, T(1))
        blend = np.zeros((n, 27), T)
        corners = np.zeros(n, U32)
        for c in range(8):
            counts = w[c] > 0
            corners |= (counts.astype(U32) << U32(c))
            wn = (w[c] * r)[:, None]
            blend = np.where(counts[:, None], blend + wn * np.where(counts[:, None], sh[idx[c]], T(0)), blend)
        x, y, z = N[:, 0], N[:, 1], N[:, 2]
        k00, k1, k2a, k20, k22 = (T(k) for k in (K00, K1, K2A, K20, K22))
        Y = [np.full(n, k00, T), k1 * y, k1 * z, k1 * x, k2a * (x * y), k2a * (y * z), k20 * ((T(3) * z) * z - T(1)), k2a * (x * z), k22 * (x * x - y * y)]
        A = [T(a) for a in PV.A32] if T is F else [T(np.pi), T(2.0 * np.pi / 3.0), T(np.pi / 4.0)]
        E = np.zeros((n, 3), T)
        for lm in range(9):
            E = E + blend[:, 3 * lm:3 * lm + 3] * (A[PV.BAND[lm]] * Y[lm])[:, None]
        E = np.maximum(T(0), E)
    flags = np.where(clamped, U32(_lib.GATHER_CLAMPED), U32(0)) | np.where(some, U32(0), U32(_lib.GATHER_NO_PROBE))
    out = dict(irradiance=np.where((ok & some)[:, None], E, T(0)), weight=np.where(ok & some, W, T(0)), corners=np.where(ok, corners, U32(0)),
               cell=np.where(ok, cell, 0).astype(U32), flags=np.where(ok, flags, U32(_lib.GATHER_NOT_GATHERED)).astype(U32))
    assert out["irradiance"].dtype == T and out["weight"].dtype == T
    if parts is not None:
        parts["branch"] = branch
    return out


def gather64(g, records, visibility, normal_bias, points, corrupt=None, parts=None):
    return _gather(g, records, visibility, normal_bias, points, F64, corrupt, parts)


def gather32(g, records, visibility, normal_bias, points, corrupt=None, parts=None):
    return _gather(g, records, visibility, normal_bias, points, F, corrupt, parts)


def judge_gather(got, want, name, tol=None):
    return PV.judge_gather(got, want, name, TOL["gather"] if tol is None else tol)


# ------------------------------------------------------------------------------------------------
# the inputs of the GPU test (and of the calibration)
# ------------------------------------------------------------------------------------------------
KINDS = PV.KINDS[:3]  # "one cell", "all cells", "one stray lane"
NORMAL_BIAS = 0.0625  # a quarter of the smallest spacing of probe_volume_ref's grids


def random_maps(g, seed=3):
    """maps with m1 in 0.2 .. 2 spacings (the grid's median one) and m2 = m1^2 (1 + v), v in 0.01 .. 0.5, per texel: both branches of the
    Chebyshev test and its floor each decide a good share of the corners (test_probe_visibility_cpu asserts a tenth each)"""
    rng = np.random.default_rng(seed)
    n = PV.count(g)
    out = np.zeros(n, VISIBILITY)
    m1 = (rng.uniform(0.2, 2.0, (n, 64)) * float(np.median(g["spacing"]))).astype(F)
    out["moments"][..., 0] = m1
    out["moments"][..., 1] = (m1 * m1).astype(F) * (1.0 + rng.uniform(0.01, 0.5, (n, 64))).astype(F)
    out["weight"] = rng.uniform(0.5, 20.0, (n, 64))
    return out


def branch_shares(parts):
    """of the corners that were looked up: the share with r <= m1, with the factor above the floor, with the floor"""
    b = parts["branch"]
    looked = b >= 0
    return tuple(float((b == q).sum() / max(looked.sum(), 1)) for q in (1, 2, 3))


# ------------------------------------------------------------------------------------------------
# the leak fixture: a closed box of 4 x 2 x 2, divided at x = 0 by a wall 0.05 thick, open above its x < 0 half only
# ------------------------------------------------------------------------------------------------
LEAK_DIMS, LEAK_SPACING = (5, 3, 3), 0.5
LEAK_ORIGIN = (-0.75, -0.5, -0.5)  # probes at x = -0.75, -0.25, 0.25, 0.75, 1.25: the cells of the layer -0.25 .. 0.25 straddle the wall
LEAK_MAX_DISTANCE = 1.5 * 0.5 * 3.0 ** 0.5  # 1.5 cell diagonals
LEAK_BIAS = 0.05
LEAK_SAMPLES = 256


def leak_parts():
    """[(lo, hi)] of the axis-parallel slabs the scene is made of: floor, walls, the divider, and the ceiling of the x > 0 half"""
    t = 0.05
    return [((-2.0, -1.0 - t, -1.0), (2.0, -1.0, 1.0)),            # floor
            ((0.0, 1.0, -1.0), (2.0, 1.0 + t, 1.0)),               # ceiling, the dark half only
            ((-2.0 - t, -1.0, -1.0), (-2.0, 1.0, 1.0)),            # the lit half's end wall
            ((2.0, -1.0, -1.0), (2.0 + t, 1.0, 1.0)),              # the dark half's end wall ("far wall")
            ((-2.0, -1.0, -1.0 - t), (2.0, 1.0, -1.0)),            # back
            ((-2.0, -1.0, 1.0), (2.0, 1.0, 1.0 + t)),              # front
            ((-0.025, -1.0, -1.0), (0.025, 1.0, 1.0))]             # the dividing wall


def leak_scene():
    from nebulae_amd import scene as S
    sc = S.Scene("leak")
    white = sc.add_material(albedo=(0.7, 0.7, 0.7, 1), rm=(1.0, 0.0))
    sc.add_geometry(*S._merge([S._box(lo, hi) for lo, hi in leak_parts()]), material=white)
    return sc


def leak_grid():
    return PV.grid(LEAK_ORIGIN, (LEAK_SPACING,) * 3, LEAK_DIMS, 0.25)


def leak_records(g):
    """SYNTHETIC records: constant radiance 1 on the probes with x < 0 (Y00 coefficient 1 / 0.282095 = 2 sqrt(pi) per channel), 0 on the rest"""
    rec = np.zeros(PV.count(g), RECORD)
    rec["samples"], rec["hits"], rec["segments"] = 64, 64, 64
    lit = PV.grid_positions32(g)[:, 0] < 0
    rec["sh"][lit, 0, :] = F(1.0 / 0.282095)
    return rec


def leak_points(n=200, seed=9):
    """n points of the dark half inside the cell layer that straddles the dividing wall, by turns on the floor (y = -1, normal +y) and on
    the wall across the room from the viewer (z = -1, normal +z): within half a cell of the divider, and farther from it than twice the
    bias, so that the biased point stays on its side"""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), F)
    pts[:, 0] = rng.uniform(0.025 + 2.0 * LEAK_BIAS, 0.25, n)
    a, b = rng.uniform(-0.45, 0.45, n), rng.uniform(-0.95, 0.45, n)
    on_floor = np.arange(n) % 2 == 0
    pts[on_floor, 1], pts[on_floor, 2], pts[on_floor, 4:7] = -1.0, a[on_floor], (0.0, 1.0, 0.0)
    pts[~on_floor, 1], pts[~on_floor, 2], pts[~on_floor, 4:7] = b[~on_floor], -1.0, (0.0, 0.0, 1.0)
    pts[:, 7] = 1.0
    return pts


def probe_directions64(probes, S, frame_index):
    """the directions of neb_gi_probe_rays(..., NEB_BAKE_SH) by probe_ref's float64 formulas -> [n, S, 3]"""
    import probe_ref as B
    return B.rays64(np.asarray(probes, F), S, "sh", frame_index)[:, 4:7].reshape(len(probes), S, 3)
