"""neb_gi_set_skin / neb_gi_skin_vertices / neb_gi_download_vertices: submeshes skinned on the device from joint matrices, the tree kept
(DESIGN.md 3.4d).

The pools after a skin call equal tests/skin_ref.py -- the written order in numpy float32 -- bit for bit, so everything the sibling
tests establish for a vertex update carries over with the skin_ref arrays as the deformation: frames equal a context built from the
skinned scene up to exact ties (test_refit_gpu.assert_same_frames, its cap unchanged), and equal a device-sourced update of the same
arrays exactly.  Cases: the Cornell parts' short box with 2 joints, the beamed room's post with 3, four grid submeshes of
atrium_small with 3 joints each in ONE call, and both Cornell boxes with 4 and 5 joints.  Skins are overlapping hat functions of the
height (skin_ref.hat_skin): every case but the room carries non-zero weights in all four slots, the last one on four distinct joints,
so each term of the written order and each half of the joint words decides bits.  Poses are rotations of 10 .. 25 degrees plus a
translation per joint (skin_ref.pose)."""
import ctypes as C

import numpy as np
import pytest
import torch

import skin_ref
import views_ref as V
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import NebError, PLANE_DEPTH, PLANE_NORMAL, PLANE_PREV_POINT, PLANE_RADIANCE
from test_deform_gpu import ATRIUM_COLUMNS, ATRIUM_GRIDS, twist_and_shear, with_arrays
from test_gi_gpu import scenes
from test_refit_gpu import H, W, _free_bytes, assert_same_frames, clone, cornell_camera, cornell_parts, frame, make_renderer, \
    moved_matrices, world_transform
from test_vertex_motion_gpu import all_sentinel, is_sentinel, raycast, vm_renderer

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("positions", "normals", "tangents")
SHORT_BOX, TALL_BOX = 1, 2


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
class Case:
    """a scene at its bind pose, a camera, and per skinned geometry its joints, weights and joint count"""

    def __init__(self, sc0, cam, w, h, joints, least_move, fourth="zero"):
        self.sc0, self.cam, self.w, self.h = sc0, cam, w, h
        self.skins = {}
        for gi, nj in joints.items():
            j, wt = skin_ref.hat_skin(sc0.geometries[gi]["positions"], nj, fourth=fourth, spare=(gi + 1) % nj)
            self.skins[gi] = (j, wt, nj)
        self.indices = sorted(self.skins)
        for k in (0, 1):
            _guard(sc0, self.skinned(k), least_move)

    def pose(self, k=0, bind=None):
        """{geometry: joint matrices} of pose k (about the box of the bind pose: sc0's, or the arrays given)"""
        return {gi: skin_ref.pose((bind or {}).get(gi, self.sc0.geometries[gi])["positions"], nj, k) for gi, (_, _, nj) in self.skins.items()}

    def skinned(self, k=0, bind=None):
        """{geometry: arrays} skin_ref makes of pose k, from the bind pose"""
        out = {}
        for gi, mats in self.pose(k, bind).items():
            j, wt, _ = self.skins[gi]
            out[gi] = skin_ref.skin_geometry((bind or {}).get(gi, self.sc0.geometries[gi]), j, wt, mats)
        return out

    def bind(self, r, stream=None):
        for gi, (j, wt, nj) in self.skins.items():
            r.set_skin(gi, j, wt, nj, stream=stream)

    def call(self, r, k=0, bind=None, **kw):
        """ONE neb_gi_skin_vertices for every skinned geometry of the case"""
        mats = self.pose(k, bind)
        r.skin_vertices(self.indices, [mats[gi] for gi in self.indices], **kw)


def _guard(sc0, arrays, least_move):
    """as test_deform_gpu._checked: no degenerate triangle before or after, positions move by more than least_move, normals by more than 0.1"""
    for gi, d in arrays.items():
        g = sc0.geometries[gi]
        tri = g["indices"].reshape(-1, 3).astype(np.int64)
        for P in (g["positions"], d["positions"]):
            area = 0.5 * np.linalg.norm(np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]), axis=1)
            assert area.min() > 1e-3 * area.mean(), gi
        assert np.abs(d["positions"] - g["positions"]).max() > least_move, gi
        assert np.abs(d["normals"] - g["normals"]).max() > 0.1, gi
        assert all(np.isfinite(d[k]).all() for k in KEYS), gi


def room_camera():
    """close to the post, which is four centimetres wide: about two pixels at 64 x 48 from here"""
    return V.look((-0.05, 0.15, 0.25), (-0.45, -0.05, -0.5))


def cornell_case():
    """2 joints: slots 2 and 3 name them again and carry 30 % of their weights"""
    return Case(cornell_parts(), cornell_camera(), W, H, {SHORT_BOX: 2}, 0.05, fourth="split")


def room_case():
    """3 joints, three non-zero influences, the fourth zero on an arbitrary valid joint"""
    return Case(V.beamed_room(), room_camera(), V.VW, V.VH, {V.POST: 3}, 0.01, fourth="zero")


def atrium_case():
    """3 joints each: three distinct joints with non-zero weights, the fourth slot non-zero on two vertices of three"""
    make, cam, w, h = scenes()["atrium_small"]
    return Case(make(), cam, w, h, {gi: 3 for gi in ATRIUM_GRIDS}, 3.0, fourth="split")


def four_joint_case():
    """both boxes of the Cornell parts with 4 and 5 joints: four DISTINCT joints with four non-zero weights on every vertex"""
    return Case(cornell_parts(), cornell_camera(), W, H, {SHORT_BOX: 4, TALL_BOX: 5}, 0.05)


CASES = {"cornell": cornell_case, "room": room_case, "atrium_small": atrium_case, "four_joints": four_joint_case}
NAMES = list(CASES)


def test_the_cases_weigh_every_term_of_the_written_order():
    """(needs no device, but belongs with the cases) slots 2 and 3 carry non-zero weights in the cornell, atrium and four-joint cases;
    the four-joint case names four distinct joints per vertex; the room keeps its fourth slot at zero"""
    for name, make in CASES.items():
        for gi, (j, w, nj) in make().skins.items():
            assert (w[:, :3] > 1e-3).all(), (name, gi)
            if name == "room":
                assert (w[:, 3] == 0).all()
            else:
                assert (w[:, 3] > 1e-3).mean() > 0.6, (name, gi)
            if name == "four_joints":
                assert all(len(set(row)) == 4 for row in j.tolist()), gi


def _renderer(*a, **k):
    r = make_renderer(*a, **k)
    r._hits_on = k.get("hits", True)
    return r


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def pools(r, sc, indices=None):
    """{geometry: (positions, normals, tangents)} as the device holds them"""
    return {gi: r.download_vertices(gi) for gi in (range(len(sc.geometries)) if indices is None else indices)}


def assert_pools(got, want, what):
    for gi, arrays in want.items():
        for key, a in zip(KEYS, got[gi]):
            assert np.array_equal(bits(a), bits(arrays[key])), f"{what}: geometry {gi} {key}"


def on_device(arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(arrays[k], F)).cuda() for k in KEYS}


# ------------------------------------------------------------------------------------------------
# 1: the pools
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_pools_after_a_skin_call_equal_the_written_order_bit_for_bit(name):
    c = CASES[name]()
    sc = clone(c.sc0)
    r = _renderer(sc, c.cam, c.w, c.h, sun_table=0)
    before = pools(r, sc)
    assert_pools(before, {gi: g for gi, g in enumerate(c.sc0.geometries)}, "download before any update")
    c.bind(r)
    c.call(r, 0)
    assert r.update_status() == {"accepted": 1, "refused": 0}
    after = pools(r, sc)
    assert_pools(after, c.skinned(0), f"{name} skinned")
    assert_pools(after, {gi: g for gi, g in enumerate(c.sc0.geometries) if gi not in c.skins}, f"{name} unskinned geometries keep their bits")
    # a sub-range reads the same values
    gi = c.indices[-1]
    n = len(c.sc0.geometries[gi]["positions"])
    part = r.download_vertices(gi, first_vertex=n // 3, n=n // 2)
    for a, b in zip(part, after[gi]):
        assert np.array_equal(bits(a), bits(b[n // 3:n // 3 + n // 2]))
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: skin == rebuild
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_skin_equals_rebuild(name, sun_table):
    c = CASES[name]()
    arrays = c.skinned(0)
    sa, sb = clone(c.sc0), with_arrays(c.sc0, arrays)
    ra, rb = _renderer(sa, c.cam, c.w, c.h, sun_table=sun_table), _renderer(sb, c.cam, c.w, c.h, sun_table=sun_table)
    depth, info = ra.bvh_depth(), ra.scene_info()
    c.bind(ra)
    frame(ra, sa, c.cam, 2)  # (a dispatch before the update: with the table on, it exists and is then invalidated)
    c.call(ra, 0, mirror=True)
    assert ra.bvh_depth() == depth and ra.scene_info() == info  # the tree is kept
    assert all(np.array_equal(bits(sa.geometries[gi][k]), bits(sb.geometries[gi][k])) for gi in arrays for k in KEYS)  # mirror=True: the scene followed
    if sun_table:  # both contexts get to a table of the skinned scene: the hold is two dispatches
        for f in (3, 4):
            frame(ra, sa, c.cam, f), frame(rb, sb, c.cam, f)
        assert ra.sun_table_stats()["builds"] == 2 and rb.sun_table_stats()["builds"] == 1
    for f, spp, mpv in ((5, 1, 2), (6, 4, 2), (7, 1, 4)):
        a, b = frame(ra, sa, c.cam, f, spp, mpv), frame(rb, sb, c.cam, f, spp, mpv)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_same_frames(a, b, f"{name} skinned table={sun_table} spp={spp} mpv={mpv}", hits_visible=(mpv == 2))
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 3: skin == device-sourced update of the skin_ref arrays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_skin_equals_a_device_sourced_update_of_the_same_arrays(name):
    c = CASES[name]()
    arrays = c.skinned(1)
    sa, sb = clone(c.sc0), clone(c.sc0)
    ra, rb = _renderer(sa, c.cam, c.w, c.h), _renderer(sb, c.cam, c.w, c.h)
    c.bind(ra)
    for r, s in ((ra, sa), (rb, sb)):
        frame(r, s, c.cam, 2)
    c.call(ra, 1)
    for gi, a in arrays.items():
        rb.update_vertices_device(gi, mirror=False, **on_device(a))
    (alo, ahi), (blo, bhi) = ra.scene_box(), rb.scene_box()
    assert np.array_equal(bits(alo), bits(blo)) and np.array_equal(bits(ahi), bits(bhi))
    for f, spp, mpv in ((5, 1, 2), (6, 4, 2), (7, 1, 4)):
        a, b = frame(ra, sa, c.cam, f, spp, mpv), frame(rb, sb, c.cam, f, spp, mpv)
        assert_same_frames(a, b, f"{name} skin against device-sourced update spp={spp} mpv={mpv}", ties_allowed=False, hits_visible=(mpv == 2))
        for key in ("rays", "bounce_nodes", "bounce_tris"):  # (the same tree, the same boxes: the same walks)
            assert a["stats"][key] == b["stats"][key], (key, a["stats"], b["stats"])
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 4: no drift, and back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_pose_a_then_pose_b_equals_pose_b_alone(name):
    c = CASES[name]()
    s1, s2 = clone(c.sc0), clone(c.sc0)
    r1, r2 = _renderer(s1, c.cam, c.w, c.h, sun_table=0), _renderer(s2, c.cam, c.w, c.h, sun_table=0)
    c.bind(r1), c.bind(r2)
    c.call(r1, 0), c.call(r1, 1)
    c.call(r2, 1)
    p1, p2 = pools(r1, s1), pools(r2, s2)
    assert_pools(p1, {gi: dict(zip(KEYS, p2[gi])) for gi in p2}, "A then B against B alone")
    assert_pools(p1, c.skinned(1), "A then B against the reference of B")
    assert_same_frames(frame(r1, s1, c.cam, 2), frame(r2, s2, c.cam, 2), "A then B against B alone", ties_allowed=False)
    r1.destroy(), r2.destroy()


def test_identity_matrices_with_unit_weights_restore_the_bind_pose():
    c = cornell_case()
    sa, sn = clone(c.sc0), clone(c.sc0)
    ra, rn = _renderer(sa, c.cam, c.w, c.h, sun_table=0), _renderer(sn, c.cam, c.w, c.h, sun_table=0)
    j, w = skin_ref.identity_skin(len(c.sc0.geometries[SHORT_BOX]["positions"]))
    ra.set_skin(SHORT_BOX, j, w, 2)
    ra.skin_vertices(SHORT_BOX, c.pose(0)[SHORT_BOX])  # (joint 0 of the pose carries the whole box away)
    moved = frame(ra, sa, c.cam, 2)
    ra.skin_vertices(SHORT_BOX, skin_ref.identity_pose(2))
    a, n = frame(ra, sa, c.cam, 3), frame(rn, sn, c.cam, 3)
    assert not np.array_equal(moved["depth"], a["depth"])
    assert_same_frames(a, n, "skinned and back", ties_allowed=False)
    assert a["stats"] == n["stats"]  # (the traversal counts do depend on the boxes)
    ra.destroy(), rn.destroy()


# ------------------------------------------------------------------------------------------------
# 5: composition
# ------------------------------------------------------------------------------------------------
def test_skin_calls_and_transform_updates_compose_in_either_order():
    c = cornell_case()
    arrays = c.skinned(0)
    mats = moved_matrices(c.sc0, [SHORT_BOX], world_transform("translate"))
    sb = with_arrays(c.sc0, arrays, {SHORT_BOX: mats[0]})
    rb = _renderer(sb, c.cam, c.w, c.h)
    s1, s2 = clone(c.sc0), clone(c.sc0)
    r1, r2 = _renderer(s1, c.cam, c.w, c.h), _renderer(s2, c.cam, c.w, c.h)
    c.bind(r1), c.bind(r2)
    c.call(r1, 0), r1.update_transforms([SHORT_BOX], mats)
    r2.update_transforms([SHORT_BOX], mats), c.call(r2, 0)
    for f, spp in ((2, 1), (3, 1), (4, 4)):
        b = frame(rb, sb, c.cam, f, spp)
        for tag, r, s in (("skin then transform", r1, s1), ("transform then skin", r2, s2)):
            assert_same_frames(frame(r, s, c.cam, f, spp), b, f"{tag} spp={spp}")
    for r in (r1, r2, rb):
        r.destroy()


def test_a_skin_bound_after_a_vertex_update_binds_the_deformed_pose():
    c = cornell_case()
    deformed = {SHORT_BOX: twist_and_shear(c.sc0, SHORT_BOX, 12.0, 0.05)}
    arrays = c.skinned(0, bind=deformed)
    sa, sb = clone(c.sc0), with_arrays(c.sc0, arrays)
    ra, rb = _renderer(sa, c.cam, c.w, c.h), _renderer(sb, c.cam, c.w, c.h)
    ra.update_vertices(SHORT_BOX, **deformed[SHORT_BOX])
    c.bind(ra)
    c.call(ra, 0, bind=deformed)
    assert_pools(pools(ra, sa, [SHORT_BOX]), arrays, "bound after a host-sourced update")
    # a later vertex update overwrites the pools, not the bind pose: the next skin call starts from the bind pose again
    ra.update_vertices(SHORT_BOX, **twist_and_shear(c.sc0, SHORT_BOX, 5.0, 0.3))
    c.call(ra, 0, bind=deformed)
    assert_pools(pools(ra, sa, [SHORT_BOX]), arrays, "after a vertex update in between")
    for f, spp in ((2, 1), (3, 4)):
        assert_same_frames(frame(ra, sa, c.cam, f, spp), frame(rb, sb, c.cam, f, spp), f"bound after an update spp={spp}")
    ra.destroy(), rb.destroy()


@pytest.mark.parametrize("sun_table", [0, 1])
def test_a_build_after_a_skin_call_starts_from_the_skinned_vertices(sun_table):
    c = atrium_case()
    arrays = c.skinned(0)
    sa, sb = clone(c.sc0), with_arrays(c.sc0, arrays)
    ra, rb = _renderer(sa, c.cam, c.w, c.h, sun_table=sun_table), _renderer(sb, c.cam, c.w, c.h, sun_table=sun_table)
    c.bind(ra)
    c.call(ra, 0)
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    assert ra.scene_info() == rb.scene_info() and ra.bvh_depth() == rb.bvh_depth()
    for f, spp in ((2, 1), (3, 4)):
        a, b = frame(ra, sa, c.cam, f, spp), frame(rb, sb, c.cam, f, spp)
        assert_same_frames(a, b, f"rebuilt after a skin call table={sun_table} spp={spp}", ties_allowed=False)  # the same tree: no mask
        for key in ("rays", "bounce_nodes", "bounce_tris") + (("shadow_nodes", "shadow_tris") if not sun_table else ()):
            assert a["stats"][key] == b["stats"][key], (key, a["stats"], b["stats"])
    # the build keeps the skin: pose 1 from the same bind pose
    c.call(ra, 1)
    assert_pools(pools(ra, sa, c.indices), c.skinned(1), "a skin call after the build")
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 6: refusals
# ------------------------------------------------------------------------------------------------
def _bake(M, P):
    """gi_bake_point's order in float32"""
    M, P = M.astype(F), P.astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((P[:, 0, None] * M[0, :3] + P[:, 1, None] * M[1, :3]) + P[:, 2, None] * M[2, :3]) + M[3, :3]


def test_a_skinned_vertex_that_overflows_is_refused_on_the_device_and_changes_nothing():
    c = cornell_case()
    sa, sn = clone(c.sc0), clone(c.sc0)
    ra, rn = _renderer(sa, c.cam, c.w, c.h), _renderer(sn, c.cam, c.w, c.h)
    # (the short box scaled by 1.35 along the world's y in both contexts: a skinned position of 2.7e38 is finite, its world position is not)
    scaled = moved_matrices(c.sc0, [SHORT_BOX], world_transform("scale"))
    ra.update_transforms([SHORT_BOX], scaled), rn.update_transforms([SHORT_BOX], scaled)
    c.bind(ra)
    j, w, nj = c.skins[SHORT_BOX]
    far = c.pose(0)[SHORT_BOX].copy()
    far[nj - 1, 3, :3] = 3.0e38
    with np.errstate(over="ignore", invalid="ignore"):
        sk = skin_ref.skin_geometry(c.sc0.geometries[SHORT_BOX], j, w, far)["positions"]
        world = _bake(scaled[0], sk)
    assert np.isfinite(far).all() and (np.abs(sk) <= 3.0e38).all()  # every entry and every skinned position is in range ...
    assert 1 <= int((~(np.abs(world) <= 3.0e38)).any(1).sum()) < len(sk)  # ... the world position of some vertices, not of all, is not
    before = pools(ra, sa)
    f0 = frame(ra, sa, c.cam, 2)
    status = ra.update_status()
    ra.skin_vertices(SHORT_BOX, far)  # NEB_OK: the refusal comes later, on the device
    assert ra.update_status() == {"accepted": status["accepted"], "refused": status["refused"] + 1}
    assert_pools(pools(ra, sa), {gi: dict(zip(KEYS, before[gi])) for gi in before}, "after a refusal on the device")
    a, n = frame(ra, sa, c.cam, 3), frame(rn, sn, c.cam, 3)
    assert_same_frames(a, n, "after a refusal on the device", ties_allowed=False)
    assert np.array_equal(a["depth"], f0["depth"])
    # mirror=True leaves the scene object alone after a refusal
    ra.skin_vertices(SHORT_BOX, far, mirror=True)
    assert all(np.array_equal(bits(sa.geometries[SHORT_BOX][k]), bits(c.sc0.geometries[SHORT_BOX][k])) for k in KEYS)
    # the next valid call is accepted
    status = ra.update_status()
    c.call(ra, 0)
    assert ra.update_status() == {"accepted": status["accepted"] + 1, "refused": status["refused"]}
    assert_pools(pools(ra, sa, [SHORT_BOX]), c.skinned(0), "a valid call after a refusal")
    ra.destroy(), rn.destroy()


def test_refusals_at_the_call_change_nothing():
    c = cornell_case()
    sa, sn = clone(c.sc0), clone(c.sc0)
    ra, rn = _renderer(sa, c.cam, c.w, c.h), _renderer(sn, c.cam, c.w, c.h)
    lib, ctx = ra._lib, ra._ctx
    nv = len(c.sc0.geometries[SHORT_BOX]["positions"])
    j, w, nj = c.skins[SHORT_BOX]
    j2, w2 = skin_ref.hat_skin(c.sc0.geometries[2]["positions"], 2)
    keep = []

    def D(gi, joints=j, weights=w, n=nj, strides=(8, 16)):
        d = _lib.SkinDesc(geometry=gi, numJoints=n, jointStride=strides[0], weightStride=strides[1])
        for key, a, dt in (("joints", joints, np.uint16), ("weights", weights, F)):
            if a is not None:
                a = np.ascontiguousarray(a, dt)
                keep.append(a)
                setattr(d, key, a.ctypes.data)
        return d

    def set_skin(*descs, n=None):
        arr = (_lib.SkinDesc * max(1, len(descs)))(*descs)
        return lib.neb_gi_set_skin(ctx, arr if descs else None, len(descs) if n is None else n, None)

    def U(gi, mats):
        u = _lib.SkinUpdate(geometry=gi)
        if mats is not None:
            m = np.ascontiguousarray(mats, F)
            keep.append(m)
            u.jointMatrices = m.ctypes.data_as(C.POINTER(C.c_float))
        return u

    def skin(*ups, n=None):
        arr = (_lib.SkinUpdate * max(1, len(ups)))(*ups)
        return lib.neb_gi_skin_vertices(ctx, arr if ups else None, len(ups) if n is None else n, None)

    pose = c.pose(0)[SHORT_BOX]
    big, nanw, infw = j.copy(), w.copy(), w.copy()
    big[6, 3] = nj  # (an influence of weight zero)
    assert w[6, 3] == 0.0
    nanw[3, 2], infw[nv - 1, 0] = np.nan, np.inf
    nanm, infm, col3 = pose.copy(), pose.copy(), pose.copy()
    nanm[1, 2, 1], infm[0, 3, 0] = np.nan, -np.inf
    col3[:, :, 3] = np.nan  # (column 3 is ignored: accepted, below)
    pos = (C.c_float * (3 * nv))()
    dl = lambda gi, first, n, p=pos: lib.neb_gi_download_vertices(ctx, gi, first, n, p, None, None, None)
    # set_skin's refusals come first: the box is bound only after them, so that a skin call without a skin has its case
    cases = [("set_skin: null skins", b"neb_gi_set_skin", lambda: set_skin(n=1), -1),
             ("set_skin: geometry out of range", b"neb_gi_set_skin", lambda: set_skin(D(2, j2, w2), D(5)), -1),
             ("set_skin: geometry far out of range", b"neb_gi_set_skin", lambda: set_skin(D(0xFFFFFFFF)), -1),
             ("set_skin: a geometry named twice", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX), D(SHORT_BOX)), -1),
             ("set_skin: numJoints 0", b"neb_gi_set_skin", lambda: set_skin(D(2, j2, w2), D(SHORT_BOX, n=0)), -1),
             ("set_skin: numJoints 65536", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX, n=65536)), -1),
             ("set_skin: joints without weights", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX, weights=None)), -1),
             ("set_skin: joint stride too small", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX, strides=(6, 16))), -1),
             ("set_skin: weight stride too small", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX, strides=(8, 12))), -1),
             ("set_skin: a joint index of a zero-weight influence beyond numJoints", b"neb_gi_set_skin", lambda: set_skin(D(2, j2, w2), D(SHORT_BOX, joints=big)), -1),
             ("set_skin: nan weight", b"neb_gi_set_skin", lambda: set_skin(D(SHORT_BOX, weights=nanw)), -5),
             ("set_skin: inf weight", b"neb_gi_set_skin", lambda: set_skin(D(2, j2, w2), D(SHORT_BOX, weights=infw)), -5),
             ("set_skin: n == 0", None, lambda: set_skin(), 0),
             ("skin: a geometry without a skin", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, pose)), -4),
             ("bind the short box", None, lambda: set_skin(D(SHORT_BOX)), 0),
             ("skin: null updates", b"neb_gi_skin_vertices", lambda: skin(n=1), -1),
             ("skin: null matrices", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, None)), -1),
             ("skin: geometry out of range", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, pose), U(5, pose)), -1),
             ("skin: a geometry named twice", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, pose), U(SHORT_BOX, pose)), -1),
             ("skin: a geometry without a skin beside one with", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, pose), U(2, pose)), -4),
             ("skin: nan in a matrix", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, nanm)), -5),
             ("skin: inf in a matrix", b"neb_gi_skin_vertices", lambda: skin(U(SHORT_BOX, infm)), -5),
             ("skin: n == 0", None, lambda: skin(), 0),
             ("skin: n == 0 with a pointer", None, lambda: skin(U(SHORT_BOX, pose), n=0), 0),
             ("download: geometry out of range", b"neb_gi_download_vertices", lambda: dl(5, 0, 1), -1),
             ("download: range beyond numVertices", b"neb_gi_download_vertices", lambda: dl(SHORT_BOX, 1, nv), -1),
             ("download: range beyond numVertices, wrapping", b"neb_gi_download_vertices", lambda: dl(SHORT_BOX, 0xFFFFFFF0, nv), -1),
             ("download: null positions", b"neb_gi_download_vertices", lambda: dl(SHORT_BOX, 0, nv, None), -1),
             ("download: empty range", None, lambda: dl(SHORT_BOX, nv, 0), 0)]
    f = 2
    for what, name, fn, want in cases:
        assert fn() == want, what
        if name:
            assert name in lib.neb_last_error(ctx), what
        a, n = frame(ra, sa, c.cam, f), frame(rn, sn, c.cam, f)
        assert_same_frames(a, n, f"after {what}", ties_allowed=False)
        assert a["stats"] == n["stats"], what
        assert ra.sun_table_stats() == rn.sun_table_stats(), what
        f += 1
    assert ra.update_status() == {"accepted": 0, "refused": 0}
    # the skin set before the refused rebinds is still the one in force; column 3 of the matrices is ignored
    assert skin(U(SHORT_BOX, col3)) == 0
    assert_pools(pools(ra, sa, [SHORT_BOX]), c.skinned(0), "after the refusals")
    # removing the skin: the pools keep what they hold, the next skin call has no skin
    ra.remove_skin(SHORT_BOX)
    assert_pools(pools(ra, sa, [SHORT_BOX]), c.skinned(0), "after remove_skin")
    assert skin(U(SHORT_BOX, pose)) == -4
    with pytest.raises(NebError):
        ra.set_skin(SHORT_BOX, j[:-1], w[:-1], nj)
    with pytest.raises(NebError):
        ra.skin_vertices([SHORT_BOX, 2], [pose])
    ra.destroy(), rn.destroy()
    # before a scene, and before a successful build
    r = DeferredRenderer()
    r.init(64, 48)
    d, u = D(SHORT_BOX), U(SHORT_BOX, pose)
    assert r._lib.neb_gi_set_skin(r._ctx, C.byref(d), 1, None) == -4
    assert r._lib.neb_gi_skin_vertices(r._ctx, C.byref(u), 1, None) == -4
    assert r._lib.neb_gi_download_vertices(r._ctx, SHORT_BOX, 0, nv, pos, None, None, None) == -4
    G, ng, M, nm, T, nt = c.sc0.descs()
    assert r._lib.neb_gi_set_scene(r._ctx, G, ng, M, nm, T, nt) == 0
    assert r._lib.neb_gi_set_skin(r._ctx, C.byref(d), 1, None) == 0  # (a set-up call: a scene is enough)
    assert r._lib.neb_gi_skin_vertices(r._ctx, C.byref(u), 1, None) == -4
    assert b"neb_gi_skin_vertices" in r._lib.neb_last_error(r._ctx)
    assert r._lib.neb_gi_build_bvh(r._ctx, None) == 0
    assert r._lib.neb_gi_skin_vertices(r._ctx, C.byref(u), 1, None) == 0
    assert r._lib.neb_gi_download_vertices(r._ctx, SHORT_BOX, 0, nv, pos, None, None, None) == 0
    assert np.array_equal(bits(np.array(pos[:], F).reshape(-1, 3)), bits(c.skinned(0)[SHORT_BOX]["positions"]))
    r.destroy()


def test_a_geometry_set_without_its_attribute_streams_gets_positions_only():
    c = cornell_case()
    g1 = c.sc0.geometries[SHORT_BOX]
    from nebulae_amd import scene as S
    sv = S.Scene("no-tangents")
    sv.add_material(albedo=(0.5, 0.5, 0.5, 1))
    sv.add_geometry(g1["positions"], g1["normals"], g1["uvs"], g1["indices"], material=0, M=g1["M"], omit=("tangents",))
    r = _renderer(sv, c.cam, 64, 48)
    j, w, nj = c.skins[SHORT_BOX]
    r.set_skin(0, j, w, nj)
    r.skin_vertices(0, c.pose(0)[SHORT_BOX], mirror=True)
    p, n, t = r.download_vertices(0)
    assert np.array_equal(bits(p), bits(c.skinned(0)[SHORT_BOX]["positions"]))
    assert np.array_equal(bits(n), bits(g1["normals"])) and not t.any()  # (the normal pool keeps the bind normals, the tangent pool its zeros)
    assert np.array_equal(bits(sv.geometries[0]["positions"]), bits(p)) and sv.geometries[0]["tangents"] is None
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 7: reprojection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "room"])
def test_the_previous_point_plane_follows_a_skin_call_as_it_follows_a_device_sourced_update(name):
    c = CASES[name]()
    arrays = c.skinned(0)
    planes = []
    for mode in ("skin", "device"):
        sc = clone(c.sc0)
        r = vm_renderer(c.w, c.h)
        raycast(r, sc, c.cam, 1)
        if mode == "skin":
            c.bind(r)
            c.call(r, 0)
        else:
            for gi, a in arrays.items():
                r.update_vertices_device(gi, mirror=False, **on_device(a))
        d2 = raycast(r, sc, c.cam, 2)
        planes.append((r.svgf.download(PLANE_PREV_POINT), d2))
        raycast(r, sc, c.cam, 3)
        assert all_sentinel(r.svgf.download(PLANE_PREV_POINT)), mode  # nothing moved since: the roll has run
        r.destroy()
    (pa, da), (pb, db) = planes
    moved = int((~is_sentinel(pa)).sum())
    print(f"[skin reprojection {name}] pixels with a previous point: {moved}")
    assert moved > (200 if name == "cornell" else 20)
    assert np.array_equal(bits(pa), bits(pb))
    for x, y in zip(da, db):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------
# 8: streams, strips, memory
# ------------------------------------------------------------------------------------------------
def test_skin_calls_with_two_dispatches_in_flight_on_two_streams():
    """test_deform_gpu.test_vertex_updates_with_two_dispatches_in_flight_on_two_streams with skin calls: one per frame for four frames,
    enqueued on a stream of its own while the previous frame's dispatch is in flight on a side stream; nothing but the library orders
    them, and every frame equals the serial context's."""
    c = atrium_case()
    outs = []
    for mode in ("plain", "two_streams"):
        sc = clone(c.sc0)
        r = DeferredRenderer()
        r.init(c.w, c.h, atrous_levels=4)
        main = torch.cuda.current_stream()
        sides = [torch.cuda.Stream() for _ in range(2)]
        mover = torch.cuda.Stream()
        r.begin_frame(RenderInfo(scene=sc, camera=c.cam, frame_index=1, stream=main.cuda_stream))
        r.submit_commands_gbuffer()
        c.bind(r, stream=(mover if mode == "two_streams" else main).cuda_stream)
        torch.cuda.synchronize()
        for pl in (PLANE_NORMAL, PLANE_DEPTH):
            r.svgf.plane_tensor(pl, 0).copy_(r.svgf.plane_tensor(pl, 1))
        rad = [r.svgf.plane_tensor(PLANE_RADIANCE, 0), r.svgf.plane_tensor(PLANE_RADIANCE, 1)]
        direct = torch.full_like(rad[0], 0.125)
        r.svgf.set_option("gi_sun_hold", 2)
        if mode == "two_streams":
            r.set_defer_resolve(2)
        resolved = [None, None]
        frames = []
        for f in range(2, 11):
            if f in (4, 5, 6, 7):
                gi = ATRIUM_GRIDS[f % 4]
                r.skin_vertices(gi, c.pose(f)[gi], stream=(mover if mode == "two_streams" else main).cuda_stream)
            side, slot = sides[f % 2], f % 2
            r.begin_frame(RenderInfo(scene=sc, camera=c.cam, frame_index=f, stream=main.cuda_stream))
            cur = r.svgf.get_current_resource_index()
            if mode == "two_streams":
                if resolved[slot] is not None:
                    side.wait_event(resolved[slot])
                r.submit_commands_gi_pathtrace(stream=side.cuda_stream)
                rad[cur].copy_(direct, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
                main.wait_event(done)
                r.submit_commands_gi_resolve()
                resolved[slot] = torch.cuda.Event()
                resolved[slot].record(main)
            else:
                rad[cur].copy_(direct, non_blocking=True)
                r.submit_commands_gi_pathtrace()
            r.submit_commands_svgf_denoising()
            frames.append(rad[cur].clone())  # (on the main stream, behind the frame's last pass)
            r.end_frame()
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in frames])
        assert r.update_status() == {"accepted": 4, "refused": 0}
        r.destroy()
    assert float(np.abs(outs[0][-1][..., :3]).max()) > 0.2
    assert not np.array_equal(outs[0][1], outs[0][-1])
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), f"frame {k + 2}"


def test_two_strip_contexts_given_the_same_skin_equal_the_full_frame():
    c = cornell_case()
    cut = 88  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = clone(c.sc0), clone(c.sc0), clone(c.sc0)
    full = _renderer(sf, c.cam)
    up = _renderer(s_up, c.cam, row_begin=0, row_end=cut)
    dn = _renderer(s_dn, c.cam, row_begin=cut, row_end=H)
    for r in (full, up, dn):
        c.bind(r)
        c.call(r, 0)
    by = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], x.shape[1], -1)
    for f, spp in ((2, 1), (3, 4)):
        a, u, d = frame(full, sf, c.cam, f, spp), frame(up, s_up, c.cam, f, spp), frame(dn, s_dn, c.cam, f, spp)
        for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
            assert np.array_equal(by(a[name]), by(np.concatenate([u[name], d[name]], axis=0))), (name, f)
        assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
        assert a["rays"] == u["rays"] + d["rays"]
    for r in (full, up, dn):
        r.destroy()


def test_a_hundred_skin_calls_hold_no_more_device_memory_and_removal_gives_everything_back():
    """Every column of atrium_small skinned with 3 joints: 64 bytes a vertex, 2.8 MB of skins.  Steady state allocates nothing (the
    sibling tests' bar of 4 MB); thirty rebinds and thirty bind / remove cycles would hold 85 MB each if the replaced or the removed
    skin stayed; a destroyed context gives back what test_soak_gpu's bar asks."""
    start = _free_bytes()
    make, cam, w, h = scenes()["atrium_small"]
    c = Case(make(), cam, w, h, {gi: 3 for gi in ATRIUM_COLUMNS}, 3.0)
    sc = clone(c.sc0)
    r = _renderer(sc, c.cam, c.w, c.h, exact=False, hits=False)
    c.bind(r)
    poses = [c.pose(k) for k in range(4)]
    free = {}
    for k in range(104):
        r.skin_vertices(c.indices, [poses[k % 4][gi] for gi in c.indices])
        if k % 4 == 0 or 40 <= k < 50:  # (rests of a few frames: tables are built and dropped along the way)
            assert np.isfinite(frame(r, sc, c.cam, 2 + k)["radiance"]).all()
        if k % 3 == 0 and k < 90:
            c.bind(r)  # binding again replaces the skin -- and captures the skinned pools as the new bind pose
        if k in (3, 103):
            free[k] = _free_bytes()
    assert r.update_status() == {"accepted": 104, "refused": 0}
    for gi in c.indices:
        r.remove_skin(gi)
    free["removed"] = _free_bytes()
    for _ in range(30):
        c.bind(r)
        for gi in c.indices:
            r.remove_skin(gi)
    free["cycled"] = _free_bytes()
    in_use = start - free["cycled"]
    r.destroy()
    free["destroyed"] = _free_bytes()
    print(f"[skin soak] free device memory (MB) after call 4 / 104: {free[3] >> 20} / {free[103] >> 20}; skins removed {free['removed'] >> 20}; "
          f"after 30 bind / remove cycles {free['cycled'] >> 20}; before init / after destroy {start >> 20} / {free['destroyed'] >> 20}")
    assert free[3] - free[103] < 4 << 20, free
    assert free["removed"] >= free[103] and free["removed"] - free["cycled"] < 4 << 20, free
    assert in_use > 2 << 20 and start - free["destroyed"] < 32 << 20, free


# ------------------------------------------------------------------------------------------------
# 9: cost
# ------------------------------------------------------------------------------------------------
def test_a_skin_call_costs_less_device_time_than_a_build():
    """the project's condition for a refit: cheaper on the device than neb_gi_build_bvh was on the same scene in the
    same process.  The four grid submeshes of the case in one call."""
    c = atrium_case()
    r = _renderer(clone(c.sc0), c.cam, c.w, c.h, exact=False, hits=False)
    build_ms = r.build_ms()
    c.bind(r)
    poses = [c.pose(k) for k in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for k in range(22):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.skin_vertices(c.indices, [poses[k % 2][gi] for gi in c.indices], stream=st)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times[2:]))
    n_verts = sum(len(c.sc0.geometries[gi]["positions"]) for gi in c.indices)
    print(f"[skin cost] {len(c.indices)} submeshes, {n_verts} vertices, 3 joints each: {med * 1e3:.0f} us on the device; neb_gi_build_ms {build_ms:.2f} ms")
    assert r.update_status() == {"accepted": 22, "refused": 0}
    assert med < build_ms, (med, build_ms)
    r.destroy()
