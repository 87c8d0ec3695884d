"""Linear-blend skinning in the library's written order, in numpy float32, and the skins and poses the CPU and GPU
tests share.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The order, with the four influences i = 0..3 as stored, every product and every sum rounded to float32 by itself (numpy never fuses):
    S[q]  = ((w0 J0[q] + w1 J1[q]) + w2 J2[q]) + w3 J3[q]            rows 0-3, columns 0-2 of the 4x4s (row-vector convention)
    p'[c] = ((p.x S[0][c] + p.y S[1][c]) + p.z S[2][c]) + S[3][c]    the bake's order
    n'[c] =  (n.x S[0][c] + n.y S[1][c]) + n.z S[2][c]               not renormalised; tangent .xyz the same, .w copied
"""
import math

import numpy as np

F = np.float32


def _f32(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.float32, getattr(a, "dtype", type(a))  # (every intermediate stays float32)
    return a


def blended(joints, weights, matrices):
    """-> S, n x 4 x 3 float32: the blended rows 0-3, columns 0-2 of every vertex"""
    J = _f32(np.ascontiguousarray(np.asarray(matrices, F).reshape(-1, 4, 4)[:, :, :3]))
    jn = np.asarray(joints).reshape(-1, 4).astype(np.int64)
    w = _f32(np.ascontiguousarray(np.asarray(weights, F).reshape(-1, 4)))
    assert jn.min() >= 0 and jn.max() < J.shape[0]
    term = [_f32(w[:, i, None, None] * J[jn[:, i]]) for i in range(4)]
    return _f32(_f32(_f32(term[0] + term[1]) + term[2]) + term[3])


def _rows(S, v, translate):
    v = _f32(np.ascontiguousarray(v, F))
    out = _f32(_f32(_f32(v[:, 0, None] * S[:, 0]) + _f32(v[:, 1, None] * S[:, 1])) + _f32(v[:, 2, None] * S[:, 2]))
    return _f32(out + S[:, 3]) if translate else out


def skin(positions, normals, tangents, joints, weights, matrices):
    """-> dict(positions, normals, tangents) of the skinned vertices (an attribute given as None stays None)"""
    S = blended(joints, weights, matrices)
    out = dict(positions=_rows(S, positions, True), normals=None, tangents=None)
    if normals is not None:
        out["normals"] = _rows(S, normals, False)
    if tangents is not None:
        t = _f32(np.ascontiguousarray(tangents, F))
        out["tangents"] = _f32(np.concatenate([_rows(S, t[:, :3], False), t[:, 3:]], axis=1))
    return out


def skin_geometry(g, joints, weights, matrices):
    """the arrays a scene rebuilt from the skinned geometry `g` (a Scene.geometries entry) holds"""
    return skin(g["positions"], g["normals"], g["tangents"], joints, weights, matrices)


# ------------------------------------------------------------------------------------------------
# skins: overlapping hat functions of the height
# ------------------------------------------------------------------------------------------------
def height(positions):
    """[0, 1] per vertex: the position in the box of the geometry, each axis scaled to the box, along (0.55, 1.0, 0.35) -- a box, whose
    corners are all a mesh has, still gets fractional weights"""
    P = np.asarray(positions, np.float64)
    lo, hi = P.min(0), P.max(0)
    u = (P - lo) / np.where(hi > lo, hi - lo, 1.0)
    d = np.array([0.55, 1.0, 0.35])
    return u @ d / d.sum()


def hat_skin(positions, n_joints, fourth="zero", spare=0):
    """-> joints (n x 4 uint16), weights (n x 4 float32).  Joint k sits at height k / (n_joints - 1); its weight is a hat function about
    it, wide enough to overlap EVERY other joint's (a quadratic hat of half-width 1.5 times the skeleton's height plus a floor), so all
    joints act on all vertices and every term of the written order carries a non-zero weight somewhere.  The weights of a vertex add
    up to one in float64 and are then rounded; slots are in no particular order of size.
    n_joints >= 4: the four heaviest joints of the vertex, four distinct joints with four non-zero weights.
    n_joints < 4: slots 0 .. n_joints - 1 are the joints; a slot beyond them names a joint again -- with fourth == "split" it takes 30 %
    of that joint's weight (on two vertices of three when it is slot 3: the rest have a zero fourth weight), with fourth == "zero" slot 3
    has weight zero and names the arbitrary valid joint `spare` (three non-zero influences at most)."""
    assert fourth in ("zero", "split") and n_joints >= 2
    h = height(positions)
    n = h.shape[0]
    at = np.arange(n_joints) / (n_joints - 1)
    raw = np.maximum(0.0, 1.0 - np.abs(h[:, None] - at[None, :]) / 1.5) ** 2 + 0.02
    raw /= raw.sum(1, keepdims=True)
    joints, weights = np.zeros((n, 4), np.int64), np.zeros((n, 4))
    rows = np.arange(n)
    if n_joints >= 4:
        top = np.sort(np.argsort(-raw, axis=1, kind="stable")[:, :4], axis=1)
        joints[:] = top
        weights[:] = raw[rows[:, None], top]
        weights /= weights.sum(1, keepdims=True)
    else:
        for s in range(n_joints):
            joints[:, s], weights[:, s] = s, raw[:, s]
        for s in range(n_joints, 4):
            if s == 3 and fourth == "zero":
                joints[:, s] = spare
                continue
            again = (s + 1) % n_joints
            share = np.where((rows % 3 != 0) | (s < 3), 0.3, 0.0) * weights[:, again]
            joints[:, s], weights[:, s] = again, share
            weights[:, again] -= share
    return np.ascontiguousarray(joints.astype(np.uint16)), np.ascontiguousarray(weights.astype(F))


def identity_skin(n):
    """weights (1, 0, 0, 0) on joint 0"""
    w = np.zeros((n, 4), F)
    w[:, 0] = 1.0
    return np.zeros((n, 4), np.uint16), w


# ------------------------------------------------------------------------------------------------
# poses: one rotation of 10 .. 25 degrees and a translation per joint, in the geometry's object space
# ------------------------------------------------------------------------------------------------
def _axis_rotation(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, s, -s, c
    return R


def pose(positions, n_joints, k=0, shift=0.02):
    """-> n_joints x 4 x 4 float32, row-vector convention (p' = p R + t): joint j turns by 10 .. 25 degrees (all in one sense: a blend of
    them still turns by 10 degrees or more; pose k shifts the angles inside that range) about the longest axis of the geometry's box through the box's centre, and moves by `shift`
    of the box's diagonal times (j + 1) / n_joints"""
    P = np.asarray(positions, np.float64)
    lo, hi = P.min(0), P.max(0)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    axis = int(np.argmax(hi - lo))
    out = np.zeros((n_joints, 4, 4))
    for j in range(n_joints):
        deg = 10.0 + 15.0 * (((j + 1) / n_joints + 0.37 * k) % 1.0)
        R = _axis_rotation(axis, deg)
        t = shift * diag * (j + 1) / n_joints * np.array([0.6, 0.3 if k % 2 == 0 else -0.3, -0.74])
        out[j, :3, :3] = R
        out[j, 3, :3] = c - c @ R + t
        out[j, 3, 3] = 1.0
    return np.ascontiguousarray(out, F)


def identity_pose(n_joints):
    return np.ascontiguousarray(np.broadcast_to(np.eye(4, dtype=F), (n_joints, 4, 4)))
