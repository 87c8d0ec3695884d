"""The lane -> range lookup the per-vertex update kernels share (lane_range, gi_refit.hip), at range boundaries chosen on purpose.

One small scene: five fans of 3, 61, 64, 65 and 257 vertices (every vertex referenced; normals, uvs and tangents) and a floor.  One call
that names all five has 450 lanes, its ranges start at lanes 0, 3, 64, 128 and 193: a boundary inside a wave, two on wave boundaries,
and the boundary between the two 256-lane blocks inside the last range.  Every comparison is bit for bit: the expected arrays are the
inputs themselves, skin_ref.skin_geometry or morph_ref.morph_geometry, which test_skin_gpu.py and test_morph_gpu.py hold the device to.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import morph_ref
import skin_ref
from nebulae_amd import _lib
from nebulae_amd import scene as S
from test_refit_gpu import H, W, clone, make_renderer

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("positions", "normals", "tangents")
COUNTS = (3, 61, 64, 65, 257)
FANS = range(len(COUNTS))
FIRST_LANES = (0, 3, 64, 128, 193)
STRIDES = dict(positionStride=12, normalStride=12, tangentStride=16)


def fan(n, k):
    """n vertices: an apex and n - 1 rim points on three quarters of a wavy circle, triangles (0, i, i + 1): every vertex is referenced"""
    a = np.linspace(0.0, 1.5 * math.pi, n - 1)
    r = 0.25 + 0.05 * np.cos(3.0 * a + k)
    P = np.concatenate([[[0.0, 0.12, 0.0]], np.stack([r * np.cos(a), 0.04 * np.sin(5.0 * a + k), r * np.sin(a)], 1)])
    N = np.stack([0.3 * np.cos(a), np.ones_like(a), 0.3 * np.sin(a)], 1)
    N = np.concatenate([[[0.0, 1.0, 0.0]], N / np.linalg.norm(N, axis=1, keepdims=True)])
    UV = 0.5 + P[:, [0, 2]]
    i = np.arange(1, n - 1)
    return P.astype(F), N.astype(F), UV.astype(F), np.stack([np.zeros_like(i), i + 1, i], 1).reshape(-1).astype(np.uint32)


def make_scene():
    sc = S.Scene("update-lanes")
    grey = sc.add_material(albedo=(0.6, 0.6, 0.6, 1), rm=(0.8, 0.0))
    for k, n in enumerate(COUNTS):
        M = np.eye(4, dtype=F)
        M[3, :3] = (0.7 * (k - 2), 0.0, 0.3 * (k % 2))
        sc.add_geometry(*fan(n, k), material=grey, M=M)
    sc.add_geometry(*S._quad((-2.5, -0.2, 1.5), (2.5, -0.2, 1.5), (2.5, -0.2, -1.5), (-2.5, -0.2, -1.5)), material=grey)
    return sc


@pytest.fixture(scope="module")
def sc0():
    sc = make_scene()
    assert [len(g["positions"]) for g in sc.geometries[:5]] == list(COUNTS)
    assert tuple(int(x) for x in np.cumsum((0,) + COUNTS[:-1])) == FIRST_LANES and sum(COUNTS) == 450
    for g in sc.geometries[:5]:
        assert set(g["indices"].tolist()) == set(range(len(g["positions"])))
        assert all(g[k] is not None for k in KEYS + ("uvs",))
    return sc


@pytest.fixture
def renderer(sc0):
    sc = clone(sc0)
    r = make_renderer(sc, S.orbit_camera(origin=(0.0, 0.0, 0.0), yaw_deg=35.0, pitch_deg=70.0, distance=4.0), W, H, sun_table=0)
    yield r
    r.destroy()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def pools(r):
    return {gi: dict(zip(KEYS, r.download_vertices(gi))) for gi in range(len(COUNTS) + 1)}


def assert_pools(got, want, what):
    for gi, arrays in want.items():
        for key in KEYS:
            assert np.array_equal(bits(got[gi][key]), bits(arrays[key])), f"{what}: geometry {gi} {key}"


def new_arrays(sc0, seed):
    """other positions, normals and tangents for the five fans, finite and of the order of the old ones"""
    rng = np.random.default_rng(seed)
    out = {}
    for gi in FANS:
        g = sc0.geometries[gi]
        out[gi] = {k: np.ascontiguousarray(g[k] + rng.uniform(-0.05, 0.05, g[k].shape), F) for k in KEYS}
    return out


def vertex_updates(arrays, pointer, first=None):
    """one neb_vertex_update per fan, all three streams: the whole fan, or with first = {geometry: vertex} that one vertex"""
    ups = []
    for gi in FANS:
        a, f = arrays[gi], 0 if first is None else first[gi]
        n = len(a["positions"])
        ups.append(_lib.VertexUpdate(geometry=gi, firstVertex=f, numVertices=n, positions=pointer(a["positions"]), normals=pointer(a["normals"]),
                                     tangents=pointer(a["tangents"]), **STRIDES))
    return (_lib.VertexUpdate * len(ups))(*ups)


def on_device(arrays):
    return {gi: {k: torch.from_numpy(a[k]).cuda() for k in KEYS} for gi, a in arrays.items()}


def test_host_vertices_of_all_five_fans_in_one_call(renderer, sc0):
    r, new = renderer, new_arrays(sc0, 1)
    before = pools(r)
    assert_pools(before, dict(enumerate(sc0.geometries)), "before any update")
    assert r._lib.neb_gi_update_vertices(r._ctx, vertex_updates(new, lambda a: a.ctypes.data), len(COUNTS), None) == 0
    after = pools(r)
    assert_pools(after, new, "neb_gi_update_vertices")
    assert_pools(after, {5: before[5]}, "the floor")
    assert r.update_status() == {"accepted": 0, "refused": 0}  # (counts device-sourced calls only)


def test_device_vertices_of_all_five_fans_in_one_call(renderer, sc0):
    r, new = renderer, new_arrays(sc0, 2)
    before = pools(r)
    dev = on_device(new)
    assert r._lib.neb_gi_update_vertices_device(r._ctx, vertex_updates(dev, lambda t: t.data_ptr()), len(COUNTS), None) == 0
    assert r.update_status() == {"accepted": 1, "refused": 0}
    after = pools(r)
    assert_pools(after, new, "neb_gi_update_vertices_device")
    assert_pools(after, {5: before[5]}, "the floor")


def test_skins_of_all_five_fans_in_one_call(renderer, sc0):
    r = renderer
    before = pools(r)
    want, keep, ups = {}, [], []
    for gi in FANS:
        g = sc0.geometries[gi]
        j, w = skin_ref.hat_skin(g["positions"], 2, fourth="split")
        mats = skin_ref.pose(g["positions"], 2, 0)
        r.set_skin(gi, j, w, 2)
        want[gi] = skin_ref.skin_geometry(g, j, w, mats)
        keep.append(mats)
        ups.append(_lib.SkinUpdate(geometry=gi, jointMatrices=mats.ctypes.data_as(C.POINTER(C.c_float))))
    assert r._lib.neb_gi_skin_vertices(r._ctx, (_lib.SkinUpdate * len(ups))(*ups), len(ups), None) == 0
    assert r.update_status() == {"accepted": 1, "refused": 0}
    after = pools(r)
    assert_pools(after, want, "neb_gi_skin_vertices")
    assert_pools(after, {5: before[5]}, "the floor")
    assert any(not np.array_equal(bits(after[gi]["positions"]), bits(before[gi]["positions"])) for gi in FANS)


def test_morphs_of_all_five_fans_in_one_call(renderer, sc0):
    """5 targets, all active: morph_accumulate takes its unrolled group of four and then its one-at-a-time tail"""
    r = renderer
    before = pools(r)
    want, keep, ups = {}, [], []
    for gi in FANS:
        g = sc0.geometries[gi]
        t = morph_ref.make_targets(g, 5, 0.05, seed=gi)
        w = morph_ref.weight_set(5, "all", gi)
        assert (w != 0).all()
        r.set_morph_targets(gi, t["positions"], t["normals"], t["tangents"])
        want[gi] = morph_ref.morph_geometry(g, t, w)
        keep.append(w)
        ups.append(_lib.MorphUpdate(geometry=gi, weights=w.ctypes.data_as(C.POINTER(C.c_float))))
    assert r._lib.neb_gi_morph_vertices(r._ctx, (_lib.MorphUpdate * len(ups))(*ups), len(ups), None) == 0
    assert r.update_status() == {"accepted": 1, "refused": 0}
    after = pools(r)
    assert_pools(after, want, "neb_gi_morph_vertices")
    assert_pools(after, {5: before[5]}, "the floor")
    assert any(not np.array_equal(bits(after[gi]["positions"]), bits(before[gi]["positions"])) for gi in FANS)


def test_five_one_vertex_ranges_change_five_vertices(renderer, sc0):
    """the last vertex of every fan, lanes 0-4 of one call: one lane per range"""
    r, new = renderer, new_arrays(sc0, 3)
    last = {gi: COUNTS[gi] - 1 for gi in FANS}
    one = {gi: {k: np.ascontiguousarray(new[gi][k][last[gi]:]) for k in KEYS} for gi in FANS}
    assert all(len(one[gi]["positions"]) == 1 for gi in FANS)
    before = pools(r)
    assert r._lib.neb_gi_update_vertices(r._ctx, vertex_updates(one, lambda a: a.ctypes.data, first=last), len(COUNTS), None) == 0
    after = pools(r)
    for gi in FANS:
        for key in KEYS:
            assert np.array_equal(bits(after[gi][key][:-1]), bits(before[gi][key][:-1])), (gi, key)
            assert np.array_equal(bits(after[gi][key][-1]), bits(new[gi][key][-1])), (gi, key)
            assert not np.array_equal(bits(after[gi][key][-1]), bits(before[gi][key][-1])), (gi, key)
    assert_pools(after, {5: before[5]}, "the floor")


def test_a_nan_in_the_last_lane_of_the_second_block_refuses_the_call(renderer, sc0):
    r, new = renderer, new_arrays(sc0, 4)
    new[4]["positions"][-1, 1] = np.nan  # lane 449
    before = pools(r)
    dev = on_device(new)
    assert r._lib.neb_gi_update_vertices_device(r._ctx, vertex_updates(dev, lambda t: t.data_ptr()), len(COUNTS), None) == 0  # (refused later, on the device)
    assert r.update_status() == {"accepted": 0, "refused": 1}
    assert_pools(pools(r), before, "after the refusal")
