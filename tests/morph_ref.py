"""Morph-target blending in the library's written order, in numpy float32, and the targets, weight sets and cases the
CPU and GPU tests share.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The order, every product and every sum rounded to float32 by itself (numpy never fuses):
    m = rest position;  for each target k with w_k != 0, in target order:  m[c] = m[c] + w_k * dP_k[c]
    n, t.xyz likewise with dN_k, dT_k where the targets carry them, otherwise the rest value with its bits kept;  t.w copied
A target of weight zero (+0 or -0) is skipped: not even the sum is made, so a -0.0 of the rest pose stays -0.0.
morph_then_skin = this, then skin_ref.skin with the blended arrays in the place of the bind pose (glTF: morph, then skin).
"""
import numpy as np

import skin_ref
from skin_ref import _f32

F = np.float32
KEYS = ("positions", "normals", "tangents")


def blend(rest, deltas, weights):
    """rest (n x 3 float32) + sum of the active targets of deltas (T x n x 3 float32), in the written order"""
    v = _f32(np.array(rest, F, copy=True))
    w = _f32(np.asarray(weights, F).reshape(-1))
    d = _f32(np.ascontiguousarray(deltas, F))
    assert d.shape == (w.shape[0],) + v.shape, (d.shape, w.shape, v.shape)
    for k in range(w.shape[0]):
        if w[k] == 0:  # (+0 and -0)
            continue
        v = _f32(v + _f32(w[k] * d[k]))
    return v


def morph(positions, normals, tangents, targets, weights):
    """-> dict(positions, normals, tangents); targets = dict(positions=T x n x 3, normals=... or None, tangents=... or None).
    An attribute given as None stays None; one the targets carry no deltas for keeps its bits."""
    out = dict(positions=blend(positions, targets["positions"], weights), normals=None, tangents=None)
    if normals is not None:
        n = _f32(np.ascontiguousarray(normals, F))
        out["normals"] = blend(n, targets["normals"], weights) if targets.get("normals") is not None else n.copy()
    if tangents is not None:
        t = _f32(np.ascontiguousarray(tangents, F))
        xyz = blend(t[:, :3], targets["tangents"], weights) if targets.get("tangents") is not None else t[:, :3].copy()
        out["tangents"] = _f32(np.concatenate([xyz, t[:, 3:]], axis=1))
    return out


def morph_geometry(g, targets, weights):
    """the arrays a scene rebuilt from the morphed geometry `g` (a Scene.geometries entry) holds"""
    return morph(g["positions"], g["normals"], g["tangents"], targets, weights)


def morph_then_skin(g, targets, weights, joints, skin_weights, matrices):
    m = morph_geometry(g, targets, weights)
    return skin_ref.skin(m["positions"], m["normals"], m["tangents"], joints, skin_weights, matrices)


# ------------------------------------------------------------------------------------------------
# targets: smooth displacement fields of the vertex height and position
# ------------------------------------------------------------------------------------------------
def make_targets(g, T, size, mode="free", attributes=True, seed=0, wavelength=None):
    """-> dict(positions, normals, tangents) of T targets for the Scene.geometries entry `g`, float32, T x n x 3 each (normals and
    tangents None with attributes=False: targets of positions only).  The displacement is a function of the vertex position alone, so
    duplicated vertices of a seam or a box corner move together:
    mode "free": size * (sin(pi (k + 1) h + phase_k) axis_k + 0.5 cos(2 h + 1.3 k) (u - 0.5)), h = skin_ref.height, u = the position
    in the geometry's box, axis_k a unit vector that turns with k;
    mode "normal": size * sin(pi (k + 1) h + phase_k) along the rest normal (a thin sheet stays clear of what lies beside it);
    mode "lift": as "normal" with the sine taken to [0.1, 1]: never below the rest surface.
    wavelength (object units): the sine runs along (0.55, 1.0, 0.35) . position with wavelength / (1 + k / 4) instead of along the
    height -- for a wide flat grid, whose normals a single wave across the whole box would hardly turn.
    Normal and tangent deltas are those of target k applied alone with weight one: the vertex normals of the displaced mesh
    (test_deform_gpu.vertex_normals) and the tangents generated from them, minus the rest arrays."""
    from nebulae_amd import scene as S
    from test_deform_gpu import vertex_normals
    P, N = g["positions"].astype(np.float64), g["normals"].astype(np.float64)
    h = skin_ref.height(P)
    lo, hi = P.min(0), P.max(0)
    u = (P - lo) / np.where(hi > lo, hi - lo, 1.0)
    dP, dN, dT = [], [], []
    for k in range(T):
        if wavelength is None:
            s = np.sin(np.pi * (k + 1) * h + 0.7 * k + 0.4 * seed)
        else:
            s = np.sin(2.0 * np.pi * (1.0 + 0.25 * k) / wavelength * (P @ np.array([0.55, 1.0, 0.35])) + 0.7 * k + 0.4 * seed)
        if mode == "free":
            a = 0.9 * k + 0.5 * seed
            axis = np.array([np.cos(a) * 0.8, 0.6 * (-1.0) ** k, np.sin(a) * 0.8])
            d = size * (s[:, None] * axis[None, :] + 0.5 * np.cos(2.0 * h + 1.3 * k)[:, None] * (u - 0.5))
        elif mode == "normal":
            d = size * s[:, None] * N
        elif mode == "lift":
            d = size * (0.55 + 0.45 * s)[:, None] * N
        else:
            raise ValueError(mode)
        d = np.ascontiguousarray(d, F)
        dP.append(d)
        if attributes:
            Pk = np.ascontiguousarray(g["positions"] + d, F)
            Nk = vertex_normals(Pk, g["indices"], g["normals"])
            Tk = S.generate_tangents(Pk, Nk, g["uvs"], g["indices"])
            dN.append(np.ascontiguousarray(Nk - g["normals"], F))
            dT.append(np.ascontiguousarray(Tk[:, :3] - g["tangents"][:, :3], F))
    return dict(positions=np.stack(dP), normals=np.stack(dN) if attributes else None, tangents=np.stack(dT) if attributes else None)


WEIGHT_KINDS = ("all", "zero_mid", "negative", "none")


def weight_set(T, kind, k=0):
    """T float32 weights: "all" every target active; "zero_mid" a zero in the middle of the list (T >= 3; the last of two; T == 1: as
    "all"); "negative" the first weight negative; "none" all zero, one of them -0.0.  k shifts the values (another pose)."""
    w = np.array([(0.9, 0.7, 0.8, 0.6, 0.75, 0.65)[(i + k) % 6] for i in range(T)], F)
    if kind == "zero_mid" and T > 1:
        w[T // 2 if T >= 3 else T - 1] = 0.0
    elif kind == "negative":
        w[0] = -w[0]
    elif kind == "none":
        w[:] = 0.0
        w[-1] = -0.0
    elif kind not in WEIGHT_KINDS:
        raise ValueError(kind)
    return w


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
SHORT_BOX, TALL_BOX = 1, 2


class Case:
    """a scene at its rest pose, a camera, and per morphed geometry its targets and the kinds of its two weight sets; optionally skins
    (skin_ref.hat_skin) for the same geometries"""

    def __init__(self, sc0, cam, w, h, targets, kinds, least_move, joints=None):
        self.sc0, self.cam, self.w, self.h, self.least_move = sc0, cam, w, h, least_move
        self.targets, self.kinds = targets, kinds
        self.indices = sorted(targets)
        self.skins = {}
        for gi, nj in (joints or {}).items():
            j, wt = skin_ref.hat_skin(sc0.geometries[gi]["positions"], nj, fourth="split", spare=(gi + 1) % nj)
            self.skins[gi] = (j, wt, nj)

    def T(self, gi):
        return self.targets[gi]["positions"].shape[0]

    def weights(self, k=0):
        """{geometry: weights} of weight set k (0 or 1: the case's kinds; 2: all zero)"""
        return {gi: weight_set(self.T(gi), "none" if k == 2 else self.kinds[gi][k], k) for gi in self.indices}

    def morphed(self, k=0, rest=None):
        """{geometry: arrays} morph_ref makes of weight set k, from the rest pose (sc0's, or the arrays given)"""
        return {gi: morph_geometry((rest or {}).get(gi, self.sc0.geometries[gi]), self.targets[gi], w) for gi, w in self.weights(k).items()}

    def pose(self, p=0):
        return {gi: skin_ref.pose(self.sc0.geometries[gi]["positions"], nj, p) for gi, (_, _, nj) in self.skins.items()}

    def morphed_and_skinned(self, k=0, p=0):
        mats = self.pose(p)
        return {gi: morph_then_skin(self.sc0.geometries[gi], self.targets[gi], w, self.skins[gi][0], self.skins[gi][1], mats[gi])
                for gi, w in self.weights(k).items()}

    def skinned(self, p=0):
        mats = self.pose(p)
        return {gi: skin_ref.skin_geometry(self.sc0.geometries[gi], j, wt, mats[gi]) for gi, (j, wt, _) in self.skins.items()}

    def bind(self, r, stream=None):
        for gi in self.indices:
            t = self.targets[gi]
            r.set_morph_targets(gi, t["positions"], t["normals"], t["tangents"], stream=stream)

    def bind_skins(self, r, stream=None):
        for gi, (j, wt, nj) in self.skins.items():
            r.set_skin(gi, j, wt, nj, stream=stream)

    def call(self, r, k=0, pose=None, **kw):
        """ONE neb_gi_morph_vertices for every morphed geometry of the case (pose: the skins' pose to hand over with it)"""
        w = self.weights(k)
        mats = None if pose is None else [self.pose(pose)[gi] for gi in self.indices]
        r.morph_vertices(self.indices, [w[gi] for gi in self.indices], mats, **kw)


def cornell_case(skinned=False):
    """the short box: T = 3, one zero weight in the middle (set 1: a negative weight); with skinned=True also a skin of 2 joints"""
    from test_refit_gpu import H, W, cornell_camera, cornell_parts
    sc0 = cornell_parts()
    t = {SHORT_BOX: make_targets(sc0.geometries[SHORT_BOX], 3, 0.2)}
    return Case(sc0, cornell_camera(), W, H, t, {SHORT_BOX: ("zero_mid", "negative")}, 0.05, joints={SHORT_BOX: 2} if skinned else None)


def room_case():
    """the beamed room's floor patch: T = 2, position deltas only, lifted off the floor"""
    import views_ref as V
    from test_refit_gpu import cornell_camera
    sc0 = V.beamed_room()
    t = {V.RUG: make_targets(sc0.geometries[V.RUG], 2, 0.08, mode="lift", attributes=False)}
    return Case(sc0, cornell_camera(), V.VW, V.VH, t, {V.RUG: ("all", "zero_mid")}, 0.01)


def boxes_case():
    """both Cornell boxes in one call: T = 1 and T = 4"""
    from test_refit_gpu import H, W, cornell_camera, cornell_parts
    sc0 = cornell_parts()
    t = {SHORT_BOX: make_targets(sc0.geometries[SHORT_BOX], 1, 0.2, seed=1), TALL_BOX: make_targets(sc0.geometries[TALL_BOX], 4, 0.2, seed=2)}
    return Case(sc0, cornell_camera(), W, H, t, {SHORT_BOX: ("all", "negative"), TALL_BOX: ("all", "zero_mid")}, 0.05)


ATRIUM_T = (2, 5, 4, 6)  # (five and six: the kernel's groups of four fetched together, and what is left over)


def atrium_case(skinned=False):
    """the four grids of atrium_small in one call, with different T and active sets: 2 / 5 / 3 of 4 / 6 active in set 0"""
    from test_deform_gpu import ATRIUM_GRIDS
    from test_gi_gpu import scenes
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    kinds = (("all", "negative"), ("all", "zero_mid"), ("zero_mid", "all"), ("negative", "zero_mid"))
    t = {gi: make_targets(sc0.geometries[gi], T, 6.0, mode="normal", seed=i, wavelength=130.0) for i, (gi, T) in enumerate(zip(ATRIUM_GRIDS, ATRIUM_T))}
    return Case(sc0, cam, w, h, t, dict(zip(ATRIUM_GRIDS, kinds)), 3.0, joints={gi: 3 for gi in ATRIUM_GRIDS} if skinned else None)


CASES = {"cornell": cornell_case, "room": room_case, "boxes": boxes_case, "atrium_small": atrium_case}


def guard(c, k):
    """what the GPU tests assume of weight set k of case c: every active target moves some vertex by more than the case's least_move,
    and -- where the targets carry normals -- its normal by more than 0.1; no degenerate triangle before or after (test_skin_gpu._guard)"""
    for gi, d in c.morphed(k).items():
        g, t, w = c.sc0.geometries[gi], c.targets[gi], c.weights(k)[gi]
        tri = g["indices"].reshape(-1, 3).astype(np.int64)
        for P in (g["positions"], d["positions"]):
            area = 0.5 * np.linalg.norm(np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]), axis=1)
            assert area.min() > 1e-3 * area.mean(), gi
        assert (w != 0).any(), gi
        for q in np.flatnonzero(w != 0):
            assert np.abs(w[q] * t["positions"][q]).max() > c.least_move, (gi, q)
            if t["normals"] is not None:
                assert np.abs(w[q] * t["normals"][q]).max() > 0.1, (gi, q)
        assert np.abs(d["positions"] - g["positions"]).max() > c.least_move, gi
        if t["normals"] is not None:
            assert np.abs(d["normals"] - g["normals"]).max() > 0.1, gi
        assert all(np.isfinite(d[key]).all() for key in KEYS), gi
