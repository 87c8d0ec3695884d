"""The reference of neb_gi_probe_rays / neb_gi_bake_probes.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
tests/test_probe_cpu.py shows on the CPU that it is right and able to fail; tests/test_probe_gpu.py judges the device with it.

Three things live here.
* The sample directions of include/nebulae_hip.h in float64 (rays64) and as a float32 numpy restatement (rays32).  The two draws and
  u0 = (float(s) + r0) / float(S) are integer and single IEEE operations, the same bits everywhere; what follows them is judged
  against float64 with a tolerance that is FOUR TIMES the largest error of rays32 under the same check (MEASURED, held to the
  measurement by test_probe_cpu.test_calibration, the rule of path_ref.MEASURED).
* The float32 reducer, which follows the written order with numpy's float32 `+` and `*` only -- IEEE operations, so bake_ref returns
  the record the device must write BIT FOR BIT, given the device's own path records and rays.
* The float64 projection of the same inputs and the bound of float32 summation around it, per word
      (S / 64 + 6 + 4) * 2^-24 * scale * sum |L * Y|
  -- S / 64 additions of the round loop, 6 of the butterfly, at most 3 roundings in Y and 1 in L * Y, each relative to the magnitudes
  summed.  This is the derivation, not a measured number."""
import numpy as np

from nebulae_amd import _lib
from oracle import gi_np

F, U32 = np.float32, np.uint32
PROBE = np.dtype([("position", F, (3,)), ("tmin", F), ("normal", F, (3,)), ("tmax", F)])
RECORD = np.dtype([("sh", F, (9, 3)), ("samples", U32), ("hits", U32), ("backfaces", U32), ("segments", U32), ("flags", U32)])
assert PROBE.itemsize == 32 and RECORD.itemsize == 128
WHAT = {"sh": _lib.BAKE_SH, "irradiance": _lib.BAKE_IRRADIANCE}
GOLDEN = 0x9E3779B9
MASKS = (32, 16, 8, 4, 2, 1)
K00, K1, K2A, K20, K22 = F(0.282095), F(0.488603), F(1.092548), F(0.315392), F(0.546274)
# rays32 against rays64, test_probe_cpu.test_calibration: the largest component error of a direction over n in {1, 3, 65}, S in {64, 192},
# both modes, rounded up from 1.247e-06.  That is ten ulp of a unit vector's component, not one or two: near the poles rho = sqrt(1 - z * z)
# is the root of a difference of nearly equal numbers, whose rounding (6e-8) the root divides by 2 rho -- rho is 0.02 in the first
# stratum of 192.  The formula is the contract, so the device carries the same error; the hemisphere samples alone stay below 3e-7.
MEASURED = dict(direction=1.25e-6)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
ULP1 = float(np.finfo(F).eps)  # the spacing of float32 in [1, 2)


def probes(position, normal=(0.0, 0.0, 1.0), tmin=0.0, tmax=1e4):
    """[n] neb_probe as a float32 [n, 8] array"""
    position = np.atleast_2d(np.asarray(position, F))
    out = np.zeros((len(position), 8), F)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = position, tmin, np.asarray(normal, F), tmax
    return out


def baked(pr, what):
    """the probes the library bakes: a position whose float32 squared length (x x + y y) + z z is finite (the queries' test of an origin),
    tmin >= 0, tmax > tmin (a NaN says no), and under "irradiance" a normal whose float32 squared length is positive and finite"""
    pr = np.asarray(pr, F)
    with np.errstate(all="ignore"):
        oo = gi_np.dot(pr[:, 0:3], pr[:, 0:3])
        ok = (oo < np.inf) & (pr[:, 3] >= 0) & (pr[:, 7] > pr[:, 3])
        if what == "irradiance":
            nn = gi_np.dot(pr[:, 4:7], pr[:, 4:7])
            ok &= (nn > 0) & (nn < np.inf)
    return ok


def sample_draws(n, S, frame_index):
    """(u0, u1) float32 [n * S]: the bits the device has -- integer hashing, one float32 sum and one IEEE division"""
    i = np.arange(n * S, dtype=U32)
    state = gi_np.jenkins_hash(~i ^ gi_np.jenkins_hash(np.array([(int(frame_index) + GOLDEN) & 0xFFFFFFFF], U32)))
    r0 = gi_np.rand(state)
    r1 = gi_np.rand(state)
    s = (i % U32(S)).astype(F)
    return ((s + r0).astype(F) / F(S)).astype(F), r1


def _unit64(v):
    return v / np.sqrt(np.sum(v * v, -1, keepdims=True))


def directions64(u0, u1, what, normal=None):
    """the formulas in float64 on the float32 draws; `normal`: float32 [m, 3], one per direction"""
    u0, u1 = u0.astype(np.float64), u1.astype(np.float64)
    b = float(gi_np.PI_TWO) * u1
    if what == "sh":
        z = 1.0 - 2.0 * u0
        rho = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        return _unit64(np.stack([rho * np.cos(b), rho * np.sin(b), z], -1))
    sn = _unit64(normal.astype(np.float64))
    up_is_z = np.abs(gi_np.normalize(normal.astype(F))[:, 2]) < F(0.999)  # (a discrete choice: made on the float32 normal, as the library makes it)
    a = np.sqrt(u0)
    up = np.where(up_is_z[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    tx = _unit64(np.cross(up, sn))
    ty = np.cross(sn, tx)
    return _unit64((a * np.cos(b))[:, None] * tx + (a * np.sin(b))[:, None] * ty + np.sqrt(1.0 - u0)[:, None] * sn)


def directions32(u0, u1, what, normal=None):
    """the same formulas in numpy float32 (numpy's sin and cos, not the library's fixed sequence: a restatement, not a copy)"""
    if what == "sh":
        z = (F(1.0) - F(2.0) * u0).astype(F)
        rho = np.sqrt(np.maximum(F(0.0), F(1.0) - z * z), dtype=F)
        b = (gi_np.PI_TWO * u1).astype(F)
        return gi_np.normalize(np.stack([rho * np.cos(b, dtype=F), rho * np.sin(b, dtype=F), z], -1).astype(F))
    return gi_np.cosine_sample_hemisphere_surface_aligned(u0, u1, gi_np.normalize(normal.astype(F)))


def _rays(pr, S, what, frame_index, directions, dtype):
    pr = np.asarray(pr, F)
    n = len(pr)
    u0, u1 = sample_draws(n, S, frame_index)
    ok = np.repeat(baked(pr, what), S)
    rep = np.repeat(pr, S, axis=0)
    out = np.zeros((n * S, 8), dtype)
    with np.errstate(all="ignore"):
        d = directions(u0[ok], u1[ok], what, rep[ok, 4:7])
    out[ok, 0:4], out[ok, 4:7], out[ok, 7] = rep[ok, 0:4], d, rep[ok, 7]
    return out


def rays64(pr, S, what, frame_index):
    """what neb_gi_probe_rays writes, in float64: [n * S, 8]; the rays of a probe that is not baked are zero"""
    return _rays(pr, S, what, frame_index, directions64, np.float64)


def rays32(pr, S, what, frame_index):
    return _rays(pr, S, what, frame_index, directions32, F)


def judge_rays(pr, S, what, frame_index, rays, name, tol=None):
    """`rays` (float32 [n * S, 8]) against the float64 formulas and the properties a sample set has -> the largest direction error;
    `tol`: the direction tolerance (default TOL; the calibration measures with none)"""
    tol = TOL["direction"] if tol is None else tol
    pr, rays = np.asarray(pr, F), np.asarray(rays, F)
    n = len(pr)
    assert rays.shape == (n * S, 8), f"{name}: shape"
    want = rays64(pr, S, what, frame_index)
    ok = np.repeat(baked(pr, what), S)
    assert not rays[~ok].view(U32).any(), f"{name}: the rays of a probe that is not baked are not zero"
    rep = np.repeat(pr, S, axis=0)
    assert np.array_equal(rays[ok][:, [0, 1, 2, 3, 7]].view(U32), rep[ok][:, [0, 1, 2, 3, 7]].view(U32)), f"{name}: origin or interval are not the probe's bits"
    d = rays[ok, 4:7].astype(np.float64)
    err = float(np.abs(d - want[ok, 4:7]).max(initial=0.0))
    assert err <= tol, f"{name}: a direction is off by {err:.3e}, tolerance {tol:.1e}"
    length = np.sqrt(np.sum(d * d, -1))
    assert (np.abs(length - 1.0) <= 2.0 * ULP1).all(), f"{name}: |d| is not 1 within 2 ulp ({float(np.abs(length - 1.0).max()):.3e})"
    s = np.tile(np.arange(S, dtype=np.float64), n)[ok]
    if what == "sh":
        lo, hi = 1.0 - 2.0 * (s + 1.0) / S - ULP1, 1.0 - 2.0 * s / S + ULP1
        assert ((d[:, 2] >= lo) & (d[:, 2] <= hi)).all(), f"{name}: z of a sample lies outside its stratum"
    else:
        nrm = _unit64(rep[ok, 4:7].astype(np.float64))
        assert (np.sum(d * nrm, -1) >= -1e-6).all(), f"{name}: a direction points below the probe's surface"
    return err


# ------------------------------------------------------------------------------------------------
# projection and reduction
# ------------------------------------------------------------------------------------------------
def sh_basis64(d):
    """the real basis in the record's order, float64, with the library's float32 constants: [m, 9]"""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    k00, k1, k2a, k20, k22 = (float(k) for k in (K00, K1, K2A, K20, K22))
    return np.stack([np.full_like(x, k00), k1 * y, k1 * z, k1 * x, k2a * x * y, k2a * y * z, k20 * (3.0 * z * z - 1.0), k2a * x * z, k22 * (x * x - y * y)], -1)


def sh_basis32(d):
    """the same in float32, every product and difference in the written order"""
    d = np.asarray(d, F)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full_like(x, K00), K1 * y, K1 * z, K1 * x, K2A * (x * y), K2A * (y * z), K20 * ((F(3.0) * z) * z - F(1.0)), K2A * (x * z),
                     K22 * (x * x - y * y)], -1).astype(F)


def scale32(S, what):
    """the one factor of the reduction, computed in double and rounded once"""
    return F(4.0 * np.pi / S) if what == "sh" else F(float(gi_np.PI) / S)


def words32(radiance, directions, what):
    """the words a lane forms: [m, 27] L.c * Y_lm (word 3 lm + c), or [m, 3] L"""
    L = np.asarray(radiance, F)
    if what == "irradiance":
        return L.copy()
    Y = sh_basis32(directions)
    with np.errstate(all="ignore"):
        return (L[:, None, :] * Y[:, :, None]).astype(F).reshape(len(L), 27)


def butterfly(v):
    """[..., 64, W] float32 -> [..., W]: v[l] = v[l] + v[l ^ m] over the masks in order, the sum of lane 0"""
    v = np.asarray(v, F)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for m in MASKS:
            v = (v + v[..., lanes ^ m, :]).astype(F)
    return v[..., 0, :]


def reduce32(words, S, scale):
    """[n * S, W] float32 words -> [n, W]: per round of 64 the butterfly, the rounds added in order to a total that starts at +0, the
    total multiplied once by `scale`"""
    w = np.asarray(words, F).reshape(-1, S // 64, 64, words.shape[-1])
    total = np.zeros((w.shape[0], w.shape[-1]), F)
    with np.errstate(all="ignore"):
        for r in range(S // 64):
            total = (total + butterfly(w[:, r])).astype(F)
        return (total * F(scale)).astype(F)


def _not_baked(rays, S):
    return ~np.asarray(rays, F).view(U32).reshape(-1, S * 8).any(-1)


def bake_ref(paths, rays, S, what, reducer=reduce32, words=words32):
    """neb_ray_path [n * S] and the rays they were traced along (float32 [n * S, 8]) -> neb_probe_record [n]: the record
    neb_gi_bake_probes must write, bit for bit.  A probe whose rays are all zero is one that was not baked."""
    rays = np.asarray(rays, F)
    n = len(rays) // S
    rec = np.zeros(n, RECORD)
    w = words(paths["radiance"], rays[:, 4:7], what)
    red = reducer(w, S, scale32(S, what))
    rec["sh"].reshape(n, 27)[:, :red.shape[1]] = red
    flags = paths["flags"].reshape(n, S)
    found = (flags & _lib.HIT_FOUND) != 0
    rec["samples"] = S
    rec["hits"] = found.sum(-1)
    rec["backfaces"] = (found & ((flags & _lib.HIT_BACKFACE) != 0)).sum(-1)
    rec["segments"] = paths["segments"].reshape(n, S).astype(np.int64).sum(-1)
    blank = _not_baked(rays, S)
    rec[blank] = np.zeros(1, RECORD)
    rec["flags"][blank] = _lib.PROBE_NOT_BAKED
    return rec


def project64(paths, rays, S, what):
    """the same inputs projected and summed in float64 -> (value [n, 27], bound [n, 27]): the bound of the module's docstring"""
    rays = np.asarray(rays, F)
    n = len(rays) // S
    L = paths["radiance"].astype(np.float64)
    if what == "sh":
        terms = (L[:, None, :] * sh_basis64(rays[:, 4:7])[:, :, None]).reshape(len(L), 27)
    else:
        terms = np.concatenate([L, np.zeros((len(L), 24))], -1)
    scale = float(scale32(S, what))
    terms = terms.reshape(n, S, 27)
    value = scale * terms.sum(1)
    bound = (S / 64 + 6 + 4) * 2.0 ** -24 * scale * np.abs(terms).sum(1)
    blank = _not_baked(rays, S)
    value[blank], bound[blank] = 0.0, 0.0
    return value, bound


def inside_bound(rec, value, bound):
    """-> the largest error of a record's 27 words in units of its bound (<= 1: inside); a word whose bound is 0 must be exact"""
    got = rec["sh"].reshape(len(rec), 27).astype(np.float64)
    err = np.abs(got - value)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0))
