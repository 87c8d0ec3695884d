"""The sun-table audit (tests/sun_audit_ref.py) shown to be right, and able to fail, before a device is involved:
- its decoding of a record's hints against pack_hints / unpack_hints of gi_internal.h, compiled for the host (tools/hints_proto.hip);
- its any-hit against oracle.gi_np.FlatScene.intersect;
- on every scene of tests/test_sun_audit_gpu.py the flags of the CPU prototype (tools/lit_proto.cpp: the device's certificate header,
  candidates from a uniform grid) pass it, in an arbitrary slot order, and reach the floors the GPU test asserts on the lit share;
- four tampered tables fail it, each in the list it belongs to.
(The device's own records are audited in tests/test_sun_audit_gpu.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sun_audit_cases as cases
import sun_audit_ref as A
from nebulae_amd import build
from test_sun_table_cpu import _world_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nebulae_amd", "csrc")


@pytest.fixture(scope="module")
def proto(tmp_path_factory):
    so = tmp_path_factory.mktemp("lit_audit") / "liblit_proto.so"
    subprocess.check_call(["g++", "-O2", "-fopenmp", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tools", "lit_proto.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


def proto_flags(proto, sc, sun, tan_half, visible=None):
    """lit_proto_flags for the visible triangles of a scene -> uint8 per triangle of the scene (bit 0: +GN side, bit 1: -GN); a hidden
    geometry and one without all its attribute streams carry 0 (no shadow ray starts there: gi_sun_table.hip leaves them unmarked)"""
    V, N, first = _world_triangles(sc)
    counts = [len(g["indices"]) // 3 for g in sc.geometries]
    geom = np.repeat(np.arange(len(counts)), counts)
    vis = np.ones(len(counts), bool) if visible is None else np.asarray(visible, bool)
    keep = vis[geom]
    Vk, Nk = np.ascontiguousarray(V[keep]), np.ascontiguousarray(N[keep])
    sd = np.array(sun, np.float32)
    fk = np.zeros(len(Vk), np.uint8)
    if len(Vk):
        proto.lit_proto_flags(len(Vk), Vk.ctypes.data_as(C.c_void_p), Nk.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), C.c_float(tan_half),
                              fk.ctypes.data_as(C.c_void_p), None)
    flags = np.zeros(len(V), np.uint8)
    flags[keep] = fk
    shaded = np.array([all(g[k] is not None for k in ("positions", "normals", "uvs", "tangents")) for g in sc.geometries], bool)
    flags[~shaded[geom]] = 0
    return flags


def records_from_flags(sc, flags, seed=3):
    """records as the device would hold them for per-triangle flags, no hints, the slots in an arbitrary order -> (records, order)"""
    counts = [len(g["indices"]) // 3 for g in sc.geometries]
    geom = np.repeat(np.arange(len(counts)), counts)
    prim = np.concatenate([np.arange(c) for c in counts])
    order = np.random.default_rng(seed).permutation(len(geom))
    none = np.full((len(geom), A.K_HINTS), A.K_NO_HINT)
    return A.encode(geom[order], flags[order], prim[order], none, np.zeros(len(geom), np.int64)), order


# ------------------------------------------------------------------------------------------------
def test_decode_agrees_with_pack_hints_field_for_field(tmp_path):
    so = tmp_path / "libhints_proto.so"
    subprocess.check_call([build._hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "hints_proto.hip"), "-o", str(so)])
    lib = C.CDLL(str(so))
    for fn in (lib.hints_no_hint, lib.hints_count, lib.hints_lit_shift, lib.hints_geom_mask):
        fn.restype = C.c_uint32
    assert (lib.hints_no_hint(), lib.hints_count(), lib.hints_lit_shift(), lib.hints_geom_mask()) == (A.K_NO_HINT, A.K_HINTS, A.K_LIT_SHIFT, A.K_GEOM_MASK)
    rng = np.random.default_rng(1)
    special = [A.K_NO_HINT, 0, 0x7FFFFE, 1, 0x400000, 0x3FFFFF, 0x040000, 0x03FFFF]
    rows = [[a, b, c, d] for a in special[:3] for b in special[:3] for c in special[:3] for d in special[:3]]
    rows += [[special[rng.integers(len(special))] if rng.random() < 0.4 else int(rng.integers(0, A.K_NO_HINT)) for _ in range(4)] for _ in range(2000)]
    rec = np.zeros((len(rows), 32), np.uint32)
    sides = rng.integers(0, 2, len(rows))
    rec[:, 27] = rng.integers(0, 1 << 32, len(rows), dtype=np.uint64).astype(np.uint32)
    rec[:, 28] = rng.integers(0, 1 << 32, len(rows), dtype=np.uint64).astype(np.uint32)
    for i, (h, s) in enumerate(zip(rows, sides)):
        words = (C.c_uint32 * 3)()
        lib.hints_pack((C.c_uint32 * 4)(*h), C.c_uint32(int(s)), words)
        rec[i, 29:32] = words[:]
        back, side = (C.c_uint32 * 4)(), C.c_uint32()
        lib.hints_unpack(words, back, C.byref(side))
        assert list(back) == h and side.value == s  # (the header's own round trip)
    dec = A.decode(rec)
    assert np.array_equal(dec["hints"], np.array(rows)) and np.array_equal(dec["hint_side"], sides)
    assert np.array_equal(dec["geometry"], rec[:, 27] & A.K_GEOM_MASK) and np.array_equal(dec["lit"], rec[:, 27] >> A.K_LIT_SHIFT)
    assert np.array_equal(dec["primitive"], rec[:, 28])
    # ... and encode, which the tests below make records with, is its inverse
    again = A.encode(dec["geometry"], dec["lit"], dec["primitive"], dec["hints"], dec["hint_side"])
    assert np.array_equal(again[:, 27:], rec[:, 27:])
    # arbitrary words (not only what pack_hints writes): unpack_hints agrees on every bit pattern
    raw = rng.integers(0, 1 << 32, (500, 32), dtype=np.uint64).astype(np.uint32)
    dec = A.decode(raw)
    for i in range(len(raw)):
        back, side = (C.c_uint32 * 4)(), C.c_uint32()
        lib.hints_unpack((C.c_uint32 * 3)(*[int(x) for x in raw[i, 29:32]]), back, C.byref(side))
        assert list(back) == list(dec["hints"][i]) and side.value == dec["hint_side"][i]


def test_the_any_hit_agrees_with_the_oracle_restatement():
    """sun_audit_ref.occluded computes Moeller-Trumbore's three triple products as matrix products per sun direction; FlatScene.intersect
    computes them ray by triangle.  Same acceptance, float64 both: they may differ only where a ray passes an edge within rounding
    (1e-9 of a barycentric here, six orders above float64's), and no ray of these scenes does."""
    for name in ("sphere", "grazed", "mirrored"):
        case = cases.cases()[name]
        sc = A.AuditScene(case.make())
        dirs = A.disk_dirs(case.sun, A.sun_tan_half(case.disk))
        tris = np.arange(sc.n)
        rays = A.shadow_rays(sc, tris, A.sample_points(sc.n), dirs)
        hit, first = A.occluded(sc, rays, dirs)
        t, i, u, v = sc.fs.intersect(rays["origin"], dirs[rays["dir"]], A.RAY_TMIN, A.G.TRACING_MAX_DISTANCE, any_hit=True)
        assert np.array_equal(hit, np.isfinite(t)), name
        assert hit.sum() > 100 and (~hit).sum() > 100, name
        # the occluder named is one the oracle's restatement accepts too
        sub = {k: w[hit] for k, w in rays.items()}
        again, _ = A.occluded(sc, sub, dirs, only=first[hit][:, None])
        assert again.all(), name


ALL = sorted(cases.cases())


@pytest.mark.parametrize("name", ALL)
def test_the_prototypes_flags_pass_the_audit(proto, name):
    """List (a) is empty when the CPU prototype's flags stand in for the device's, in a permuted slot order; where the GPU test asserts a
    floor on the lit share, the prototype reaches it."""
    case = cases.cases()[name]
    sc = case.make()
    tan_half = A.sun_tan_half(case.disk)
    flags = proto_flags(proto, sc, case.sun, tan_half)
    rec, _ = records_from_flags(sc, flags)
    res = A.audit(A.decode(rec), A.AuditScene(sc), case.sun, tan_half, shares=case.shares)
    print(f"[{name}] {sc.num_triangles} triangles, prototype lit sides {res['lit_sides']}, rays traced {res['rays']}, lit share {res['lit_share']}"
          f" of {res['clear_sides']} all-clear sides")
    assert res["n_occluded_lit"] == 0, res["occluded_lit"][:3]
    assert res["violations"] == []
    assert res["rays"] * sc.num_triangles <= 1e8
    if not case.table:
        assert not flags.any()
    if case.shares and case.floor:
        assert res["clear_sides"] > 50 and res["lit_share"] >= case.floor, res["lit_share"]


def test_the_prototypes_flags_pass_the_audit_through_the_updates(proto):
    sc0 = cases.update_scene()
    moved = cases.with_matrix(sc0, cases.UPDATE_OCCLUDER, cases.update_matrix(True))
    tan_half = A.sun_tan_half(cases.DISK)
    lit_floor = {}
    for what, sc, visible in (("start", sc0, None), ("moved", moved, None), ("hidden", moved, [True, False, True]), ("shown", moved, None)):
        flags = proto_flags(proto, sc, cases.SUN, tan_half, visible)
        rec, order = records_from_flags(sc, flags)
        res = A.audit(A.decode(rec), A.AuditScene(sc, visible), cases.SUN, tan_half, shares=True)
        assert res["n_occluded_lit"] == 0 and res["violations"] == [], (what, res["occluded_lit"][:3], res["violations"][:3])
        lit_floor[what] = int((flags[:128] & 1).sum())
    print(f"[updates] floor sides lit on top: {lit_floor}")
    assert lit_floor["start"] == 128 and lit_floor["hidden"] == 128 and lit_floor["moved"] < 128 and lit_floor["shown"] == lit_floor["moved"]


# ------------------------------------------------------------------------------------------------
# mutations: the audit can fail
# ------------------------------------------------------------------------------------------------
def _audited(proto, name, mutate):
    case = cases.cases()[name]
    sc = case.make()
    tan_half = A.sun_tan_half(case.disk)
    flags = proto_flags(proto, sc, case.sun, tan_half)
    rec, order = records_from_flags(sc, flags)
    dec = A.decode(rec)
    mutate(dec, order, flags)
    rec = A.encode(dec["geometry"], dec["lit"], dec["primitive"], dec["hints"], dec["hint_side"])
    return A.audit(A.decode(rec), A.AuditScene(sc), case.sun, tan_half), order


@pytest.mark.parametrize("position", ["first", "middle", "last"])
def test_a_lit_bit_on_the_sliver_receiver_fails_the_audit(proto, position):
    def mutate(dec, order, flags):
        slot = int(np.nonzero(order == 0)[0][0])  # triangle 0 of the scene: the receiver whose corner the sliver shadows
        assert dec["lit"][slot] & 1 == 0, "the prototype calls the receiver under the sliver lit"
        dec["lit"][slot] |= 1
    res, order = _audited(proto, f"sliver_{position}", mutate)
    assert res["n_occluded_lit"] > 0 and res["violations"] == []
    assert all(r["triangle"] == 0 and r["side"] == 0 and r["geometry"] == 0 and r["occluder"] == 2 for r in res["occluded_lit"]), res["occluded_lit"][:3]
    assert res["n_occluded_lit"] <= 7  # the seven rays of the one corner sample the sliver covers


def test_a_lit_bit_under_the_canopy_fails_the_audit(proto):
    hit = {}

    def mutate(dec, order, flags):
        under = np.nonzero((flags[order] & 1) == 0)[0]  # slots the prototype leaves unproven on top: the floor under the roof
        under = under[dec["geometry"][under] == 0]
        assert len(under) > 0
        hit["slot"] = int(under[len(under) // 2])
        dec["lit"][hit["slot"]] |= 1
    res, order = _audited(proto, "grid_129", mutate)
    assert res["n_occluded_lit"] > 0 and all(r["slot"] == hit["slot"] for r in res["occluded_lit"])
    assert all(r["occluder"] >= 127 for r in res["occluded_lit"])  # the roof's two triangles come last in the scene


def test_a_hint_out_of_range_fails_the_audit(proto):
    def mutate(dec, order, flags):
        slot = int(np.nonzero((dec["lit"] & 1) == 0)[0][0])
        dec["hints"][slot] = [len(order), A.K_NO_HINT, A.K_NO_HINT, A.K_NO_HINT]
    res, _ = _audited(proto, "grid_129", mutate)
    assert res["n_occluded_lit"] == 0 and len(res["violations"]) == 1 and "n_slots" in res["violations"][0][1]


def test_a_hole_before_a_hint_fails_the_audit(proto):
    def mutate(dec, order, flags):
        slot = int(np.nonzero((dec["lit"] & 1) == 0)[0][0])
        dec["hints"][slot] = [(slot + 1) % len(order), A.K_NO_HINT, (slot + 2) % len(order), A.K_NO_HINT]
    res, _ = _audited(proto, "grid_129", mutate)
    assert res["n_occluded_lit"] == 0 and len(res["violations"]) == 1 and "behind a kNoHint" in res["violations"][0][1]


def test_the_other_structural_violations_are_told_apart():
    n = 6
    geom, prim = np.zeros(n, np.int64), np.arange(n)
    none = A.K_NO_HINT
    hints = np.array([[1, 2, none, none], [1, none, none, none], [3, 3, none, none], [4, none, none, none], [none] * 4, [0, 1, 2, 3]])
    lit = np.array([0, 0, 0, 1, 3, 2])
    side = np.array([0, 0, 1, 0, 0, 0])
    bad = A.hint_violations(A.decode(A.encode(geom, lit, prim, hints, side)))
    assert [(s, w.split()[0]) for s, w in bad] == [(1, "a"), (2, "duplicate"), (3, "hints")], bad  # own slot; duplicates; hints on a lit side


def test_the_export_refuses_a_null_context():
    from nebulae_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.neb_gi_debug_shade_records(None, None, 0, C.byref(n), None) == -1 and n.value == 7
