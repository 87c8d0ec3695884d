"""Refitted trees looked at from many viewpoints, on trees that hold split references.

test_refit_gpu.py, test_deform_gpu.py and test_motion_gpu.py rest on one argument: results cannot depend on the boxes, so a tree
refitted in place renders what a tree built from the updated scene renders.  That holds only while every refitted box is
conservative, and a box left slightly too small goes unnoticed unless a ray needs it.  Here the updated contexts are looked at from
eight cameras per update instead of one, with closest-hit walks (neb_gbuffer_raycast, the GI bounce rays) and any-hit walks
(neb_pbr_direct under three suns), against a context built from the updated scene AND against a float64 brute-force caster over
the scene's triangles (tests/views_ref.py), on scenes whose trees hold clipped references of oversized triangles; and through the
moves the other tests leave out: out of the scene box, a mirror, a pile that makes the walk spill its stack.

Every cap is test_refit_gpu.TIE_CAP or a bar of the test it is taken from.  tests/test_views_ref_cpu.py shows on the CPU that two
correct casters (float32 and float64) differ at no more than TIE_CAP // 2 pixels at every (scene state, camera) pair used here.
Measured counts are printed and recorded in docs/NOTEBOOK.md."""
import numpy as np
import pytest

import views_ref as V
from motion_ref import NO_SUBMESH
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import PLANE_DEPTH, PLANE_RADIANCE, PLANE_ROUGH_METAL, PLANE_SUBMESH_ID
from oracle_lib import OracleTracer
from reproject_ref import surface
from svgf_cases import rel_l2
from test_deform_gpu import _deform_against_rebuild, sine_along_normal, update as update_vertices
from test_gi_gpu import scenes, upload_gbuffer
from test_refit_gpu import TIE_CAP, _bits, _refit_against_rebuild, _renderer, assert_same_frames, clone, cornell_camera, frame, \
    moved_matrices, with_matrices

pytestmark = pytest.mark.gpu

F = np.float32
SUNS = [(0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.23, -0.31, -0.92)]  # the first two: test_gi_gpu.test_axis_parallel_sun_rays; the third shines in through the room's open front


# ------------------------------------------------------------------------------------------------
# one view of two contexts that hold the same scene, and of the float64 caster
# ------------------------------------------------------------------------------------------------
def _motion_on(r):
    """option svgf_motion: neb_gbuffer_raycast writes the submesh-id plane"""
    r.svgf.set_option("svgf_reproject", 1)
    r.svgf.set_option("svgf_motion", 1)
    return r


def _look(r, sc, cam, f):
    """one GI frame with its G-buffer and hit records (test_refit_gpu.frame), the id plane, and the direct light of three suns"""
    out = frame(r, sc, cam, f)
    out["ids"] = r.svgf.download(PLANE_SUBMESH_ID)  # (the slots turn at begin_frame: this is still the frame's)
    out["rough_metal"] = r.svgf.download(PLANE_ROUGH_METAL, 0)
    out["constants"] = r.global_constants()
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f + 1))
    r.submit_commands_gbuffer()
    sun, disk = r.sun.direction, r.sun.rough_diameter
    out["direct"] = []
    for d in SUNS:
        r.sun.direction, r.sun.rough_diameter = d, 0.0
        r.submit_commands_pbr_lighting()
        out["direct"].append(r.svgf.download(PLANE_RADIANCE))
    r.sun.direction, r.sun.rough_diameter = sun, disk
    r.end_frame()
    return out


def _assert_view(a, b, sc, cam, w, h, what, tris=None, stats=None):
    """a: the updated context, b: a context built from the updated scene `sc`, both through _look.
    - G-buffer and GI frame: test_refit_gpu.assert_same_frames (depth bit for bit, ties <= TIE_CAP); the id plane likewise
    - direct light of each sun: bit for bit except at <= TIE_CAP pixels
    - coverage and submesh ids of a against the float64 caster: <= TIE_CAP pixels
    - the bounce rays' hits of a against the float64 caster, fed the rays rebuilt from a's G-buffer and the dispatch's constants
      (views_ref.bounce_rays: the ray generation of oracle/gi_np.py) -- on pixels that show a surface: <= TIE_CAP rays"""
    assert_same_frames(a, b, what)
    ids_diff = int((a["ids"] != b["ids"]).sum())
    assert np.array_equal(surface(a["depth"]), a["ids"] != NO_SUBMESH), what
    lit = []
    for k, (da, db) in enumerate(zip(a["direct"], b["direct"])):
        n = int((_bits(da) != _bits(db)).any(-1).sum())
        lit.append((int((da[..., 0] > 0).sum()), n))
        assert n <= TIE_CAP, f"{what}: direct light of sun {SUNS[k]} differs at {n} pixels"
    assert ids_diff <= TIE_CAP, f"{what}: id plane differs at {ids_diff} pixels"
    tris = tris if tris is not None else V.triangles(sc)
    ref = V.primary(sc, cam, w, h, np.float64, tris)
    got = dict(covered=surface(a["depth"]), geometry=a["ids"])
    wrong = V.differing(got, ref)
    n_wrong = int(wrong.sum())
    # the bounce rays
    gb = dict(albedo=a["albedo"], world_pos=a["world_pos"], normal=a["normal"], rough_metal=a["rough_metal"])
    o, d = V.bounce_rays(gb, a["constants"])
    want = V.cast(tris, o, d, tmin=0.01, tmax=10000.0, dtype=np.float64)
    hits = a["hits"].reshape(-1)
    found = hits["t"] >= 0
    same = np.where(found, (hits["geometry"] == want["geometry"]) & (hits["primitive"] == want["primitive"]), want["geometry"] == NO_SUBMESH)
    bad = ~same & got["covered"].reshape(-1)
    n_bad = int(bad.sum())
    print(f"[{what}] ids against the rebuild differ at {ids_diff} px; direct light (lit px, differing px) {lit}; against float64: "
          f"coverage / ids differ at {n_wrong} of {int(ref['covered'].sum())} covered px, bounce hits at {n_bad} of {int(found.sum())} that hit")
    if stats is not None:
        stats.append((what, ids_diff, n_wrong, n_bad))
    if n_wrong > TIE_CAP:
        y, x = [int(v[0]) for v in np.nonzero(wrong)]
        raise AssertionError(f"{what}: {n_wrong} pixels differ from the float64 caster; first ({x}, {y}): device covered {bool(got['covered'][y, x])} "
                             f"submesh {int(a['ids'][y, x])}, caster covered {bool(ref['covered'][y, x])} submesh {int(ref['geometry'][y, x])} "
                             f"primitive {int(ref['primitive'][y, x])} t {float(ref['t'][y, x]):.6f}")
    if n_bad > TIE_CAP:
        k = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {n_bad} bounce rays differ from the float64 caster; first at pixel ({k % w}, {k // w}): device "
                             f"({int(hits['geometry'][k])}, {int(hits['primitive'][k])}, t {float(hits['t'][k]):.6f}), caster "
                             f"({int(want['geometry'][k])}, {int(want['primitive'][k])}, t {float(want['t'][k]):.6f})")


def _pair(sa, sb, cam, sun_table=0):
    ra, rb = (_motion_on(_renderer(s, cam, V.VW, V.VH, sun_table=sun_table)) for s in (sa, sb))
    return ra, rb


def _assert_split(r, sc, what):
    refs = r.scene_bytes()["triangles"] // 176  # (176 bytes of triangle + shading record per reference: test_gi_gpu.test_gi_matches_oracle)
    print(f"[{what}] {refs} references for {sc.num_triangles} triangles")
    assert refs > sc.num_triangles, f"{what}: the tree holds no split reference ({refs} for {sc.num_triangles} triangles)"


# ------------------------------------------------------------------------------------------------
# b: many viewpoints against a rebuild and against brute force
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [0, 1, 2], ids=["rotate the boxes", "then shift the beams", "then a sine on patch and post"])
def test_every_kind_of_update_seen_from_eight_cameras(last):
    """The beamed room (views_ref.beamed_room; measured: 1 296 references for its 1 246 triangles), three updates one after the other
    on one context -- the boxes rotated, the beams shifted, a sine on the floor patch and the post -- and after the last of them the
    eight cameras of views_ref.swept_views at 64 x 48.  Sun table off: every shadow ray walks the tree.  Measured on an MI355X
    (docs/NOTEBOOK.md): no view of the 24 differs from the rebuild or from float64 at any pixel or bounce ray."""
    sc0, updates = V.room_updates()
    views = V.swept_views(cornell_camera())
    sa = clone(sc0)
    ra = _motion_on(_renderer(sa, views["room"], V.VW, V.VH, sun_table=0))
    _assert_split(ra, sc0, "beamed room")
    depth, info = ra.bvh_depth(), ra.scene_info()
    for name, kind, payload, sc in updates[:last + 1]:
        if kind == "transforms":
            ra.update_transforms(*payload)
        else:
            update_vertices(ra, payload)
        assert ra.bvh_depth() == depth and ra.scene_info() == info  # the tree is kept
    sb = clone(sc)
    rb = _motion_on(_renderer(sb, views["room"], V.VW, V.VH, sun_table=0))
    f, stats, tris = 2, [], V.triangles(sc)
    for vname, cam in views.items():
        a, b = _look(ra, sa, cam, f), _look(rb, sb, cam, f)
        _assert_view(a, b, sc, cam, V.VW, V.VH, f"{name} / {vname}", tris, stats)
        f += 2
    ra.destroy(), rb.destroy()
    print("[views] worst per view: ids against the rebuild %d, against float64 %d px, %d bounce rays" % tuple(max(s[k] for s in stats) for k in (1, 2, 3)))


# ------------------------------------------------------------------------------------------------
# c: a move out of the scene box, and back
# ------------------------------------------------------------------------------------------------
def test_a_move_out_of_the_scene_box_and_back():
    """The short box carried to three room sizes outside the room and the beams beyond +-218 units in one update: the root and every
    ancestor grow, every quantised node on the way gets a new corner and scale, and the sun table finds no certificate (no build from
    there on).  Three views at 64 x 48 with the far plane at 1000.  A second update brings both back: the frames equal those of a
    context that never moved; the node visits may exceed that context's, because the leaves that held clipped pieces of the beams'
    triangles took whole-triangle bounds when they were refitted and keep them (gi_refit.hip, refit_level_kernel) -- the never-moved
    tree still has the builder's clipped boxes."""
    sc0, indices, mats, far = V.carried_updates()
    views = V.outside_views()
    inside = views["from inside"]
    sa, sb, sn = clone(sc0), clone(far), clone(sc0)
    ra, rb = _pair(sa, sb, inside, sun_table=1)
    rn = _motion_on(_renderer(sn, inside, V.VW, V.VH, sun_table=1))
    _assert_split(ra, sc0, "beamed room")
    for f in (2, 3):
        frame(ra, sa, inside, f), frame(rn, sn, inside, f), frame(rb, sb, inside, f)
    assert ra.sun_table_stats()["builds"] == 1 and rb.sun_table_stats()["builds"] == 0, (ra.sun_table_stats(), rb.sun_table_stats())
    orig = np.stack([sa.geometries[i]["M"] for i in indices])
    ra.update_transforms(indices, mats)
    lo, hi = far.world_aabb()
    assert lo[2] < -218.0 and hi[0] > 5.0
    f, tris = 4, V.triangles(far)
    for vname, cam in views.items():
        a, b = _look(ra, sa, cam, f), _look(rb, sb, cam, f)
        _assert_view(a, b, far, cam, V.VW, V.VH, f"carried out / {vname}", tris)
        f += 2
    st = ra.sun_table_stats()
    assert st["builds"] == 1 and st["lit_plus"] == 0 and st["lit_minus"] == 0, st  # eight dispatches past the hold of two: no table out there
    assert rb.sun_table_stats()["builds"] == 0
    ra.update_transforms(indices, orig)
    tris = V.triangles(sc0)
    for vname in ("from inside", "looking back"):
        cam = views[vname]
        a, n = _look(ra, sa, cam, f), _look(rn, sn, cam, f)
        _assert_view(a, n, sc0, cam, V.VW, V.VH, f"brought back / {vname}", tris)
        print(f"[brought back / {vname}] traversal {a['stats']} / never moved {n['stats']}")
        f += 2
    assert ra.sun_table_stats()["builds"] == 2  # back inside +-218: a table again
    for r in (ra, rb, rn):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# d: a mirror
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_table", [0, 1])
def test_a_mirrored_box_equals_a_rebuild(sun_table):
    """The tall box reflected in a vertical plane through its centre and turned (determinant -1): winding and geometric normal flip
    in the re-bake, and the sides the sun table calls lit swap.  test_refit_gpu._refit_against_rebuild: after the hold of two
    dispatches both contexts have a table of the mirrored scene."""
    T = V.mirror_of_the_tall_box()
    assert abs(np.linalg.det(T[:3, :3]) + 1.0) < 1e-12
    _refit_against_rebuild(V.beamed_room(), cornell_camera(), [2], T, sun_table, 256, 192, "mirror")


def _updated_against_oracle(tag, sa, sm, cam, w, h, apply, bar=2e-5):
    """test_refit_gpu.test_an_updated_context_matches_the_oracle_on_the_moved_scene with the scene, the update and -- for
    atrium_longthin, as in test_gi_gpu.test_gi_matches_oracle -- the bar on agreeing pixels as arguments; every other bar is that test's"""
    r = DeferredRenderer()
    r.init(w, h, atrous_levels=4)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=4))
    apply(r)
    o = OracleTracer(sm)
    assert all(np.array_equal(g[k], q[k]) for g, q in zip(sa.geometries, sm.geometries) for k in ("M", "positions", "normals", "tangents"))
    gb = o.gbuffer(w, h, cam)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=5))
    r.submit_commands_gbuffer()
    d = r.svgf.download(PLANE_DEPTH)
    covered = (d >> 24) == (gb["depth"] >> 24)
    assert covered.mean() >= 1.0 - 2e-4
    dz = np.abs((d & 0xFFFFFF).astype(np.int64) - (gb["depth"] & 0xFFFFFF).astype(np.int64))
    assert np.percentile(dz, 99.9) <= 4
    upload_gbuffer(r, gb)
    base = np.full((h, w, 4), 0.25, F)
    base[..., 3] = 1.0
    r.svgf.upload(PLANE_RADIANCE, -1, base)
    r.set_debug_hits(True)
    r.ray_count(reset=True)
    r.submit_commands_gi_pathtrace()
    got, hits, rays = r.svgf.download(PLANE_RADIANCE), r.download_hits(), r.ray_count()
    spill = r.node_index_stats()["deep_stack_phases"]
    want, ohits, orays = o.gi(gb, r.global_constants(), radiance=base.copy())
    same = (hits["geometry"] == ohits["geometry"]) & (hits["primitive"] == ohits["primitive"]) & ((hits["flags"] & 1) == (ohits["flags"] & 1))
    print(f"[oracle {tag}] hit mismatch {1.0 - same.mean():.2e}, rays {rays} / {orays}, rel-L2 {rel_l2(got[..., :3], want[..., :3]):.2e}, "
          f"on agreeing pixels {rel_l2(got[same][:, :3], want[same][:, :3]):.2e}; node phases with more than 12 stack entries {spill}")
    assert 1.0 - same.mean() <= 2e-4
    assert abs(rays - orays) <= max(4, 4e-4 * orays)
    assert rel_l2(got[..., :3], want[..., :3]) <= 2e-3
    assert rel_l2(got[same][:, :3], want[same][:, :3]) <= bar
    t_err = np.abs(hits["t"][same] - ohits["t"][same]) / np.maximum(np.abs(ohits["t"][same]), 1e-6)
    assert t_err.max() <= 1e-4
    r.destroy()
    return spill


def test_a_mirrored_context_matches_the_oracle():
    sc0, T = V.beamed_room(), V.mirror_of_the_tall_box()
    mats = moved_matrices(sc0, [2], T)
    _updated_against_oracle("mirror", clone(sc0), with_matrices(sc0, [2], mats), cornell_camera(), 256, 192, lambda r: r.update_transforms([2], mats))


# ------------------------------------------------------------------------------------------------
# a: atrium_longthin -- a tree with split references
# ------------------------------------------------------------------------------------------------
LONGTHIN_BAR = 1e-4  # test_gi_gpu.test_gi_matches_oracle's bar on agreeing pixels for this scene (its reasons are written there)
_longthin = {}


def longthin():
    """-> (make, camera, w, h, submeshes that hold oversized triangles, small submeshes that hold none), the last two from the scene"""
    if not _longthin:
        make, cam, w, h = scenes()["atrium_longthin"]
        sc = make()
        big, gi = V.oversized(sc)
        with_big = sorted(set(gi[big].tolist()))
        spans = []
        for g in sc.geometries:
            P = g["positions"] @ g["M"][:3, :3] + g["M"][3, :3]
            spans.append(float(np.linalg.norm(P.max(0) - P.min(0))))
        small = [k for k in range(len(sc.geometries)) if k not in with_big and spans[k] < 8.0]  # (columns and arches: the floor holds no oversized triangle either)
        assert len(with_big) >= 8 and len(small) >= 30, (with_big, small)
        _longthin.update(make=make, cam=cam, w=w, h=h, with_big=with_big, small=small, spans=spans)
    t = _longthin
    return t["make"], t["cam"], t["w"], t["h"], t["with_big"], t["small"]


def longthin_moved():
    """the last three submeshes with oversized triangles (two outer walls' strips and the beams), the first (a gallery floor's strips),
    and four of the small ones"""
    _, _, _, _, with_big, small = longthin()
    return with_big[-3:] + with_big[:1] + small[::11][:4]


def _shift():
    T = np.eye(4)
    T[3, :3] = (0.31, 0.07, -0.23)  # (test_refit_gpu's move of atrium_small)
    return T


@pytest.mark.parametrize("sun_table", [0, 1])
def test_refit_equals_rebuild_on_a_tree_with_split_references(sun_table):
    """The rebuilt context splits the moved triangles afresh; the refitted one keeps the old pieces, each with the bounds of its
    whole triangle.  Frames are equal all the same."""
    make, cam, w, h, _, _ = longthin()
    _refit_against_rebuild(make(), cam, longthin_moved(), _shift(), sun_table, w, h, "atrium_longthin translate")


def longthin_case():
    make, cam, w, h, _, _ = longthin()
    sc0 = make()
    deform = {gi: sine_along_normal(sc0, gi, phase=0.4 * k) for k, gi in enumerate(longthin_moved()[1:7])}
    for gi, d in deform.items():
        assert np.abs(d["positions"] - sc0.geometries[gi]["positions"]).max() > 3.0 and np.isfinite(d["tangents"]).all()
    return sc0, cam, w, h, deform


@pytest.mark.parametrize("shape", ["all", "partial"])
def test_deform_equals_rebuild_on_a_tree_with_split_references(shape):
    """a wall's strips, the beams, a gallery floor's strips and three small submeshes under test_deform_gpu's sine along the normal;
    every stream, and half the vertices from firstVertex > 0"""
    _deform_against_rebuild(longthin_case, shape, 1, "atrium_longthin")


def test_an_updated_context_matches_the_oracle_on_a_tree_with_split_references():
    make, cam, w, h, _, _ = longthin()
    sc0 = make()
    moved = longthin_moved()
    mats = moved_matrices(sc0, moved, _shift())
    sa = clone(sc0)
    r = DeferredRenderer()
    r.init(w, h)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=1))
    _assert_split(r, sc0, "atrium_longthin")
    r.destroy()
    _updated_against_oracle("atrium_longthin", clone(sc0), with_matrices(sc0, moved, mats), cam, w, h, lambda r: r.update_transforms(moved, mats), LONGTHIN_BAR)


# ------------------------------------------------------------------------------------------------
# e: a pile
# ------------------------------------------------------------------------------------------------
def pile():
    """24 small submeshes of atrium_longthin (columns of both storeys and arches) moved onto the spot the camera looks at, each turned,
    tilted and scaled by amounts of its own about its centre -- no two of them are the same geometry in the world, so the pile
    manufactures no exact ties -- and, with them, the beams (oversized triangles) moved a little.  Sibling boxes all over the tree
    now overlap at one spot."""
    make, cam, w, h, with_big, small = longthin()
    sc0 = make()
    chosen = small[::2][:24]
    spot = np.array([0.3, 0.0, 0.4])
    mats = []
    for k, gi in enumerate(chosen):
        g = sc0.geometries[gi]
        P = g["positions"].astype(np.float64) @ g["M"][:3, :3].astype(np.float64) + g["M"][3, :3]
        c = 0.5 * (P.min(0) + P.max(0))
        T = V._rotation(1, 23.0 * k, c) @ V._rotation(0, 2.5 * (k % 7) - 7.0, c)
        Sc = np.eye(4)
        Sc[:3, :3] = np.diag([1.0 - 0.02 * k, 1.0 + 0.015 * k, 1.0 - 0.011 * k])
        Sc[3, :3] = c - c @ Sc[:3, :3]
        T = T @ Sc
        T[3, :3] += (spot[0] - c[0] + 0.07 * np.cos(1.7 * k), 0.03 * k, spot[2] - c[2] + 0.07 * np.sin(1.7 * k))
        mats.append(moved_matrices(sc0, [gi], T)[0])
    nudge = np.eye(4)
    nudge[3, :3] = (0.21, 0.09, 0.13)
    beams = with_big[-1]
    mats.append(moved_matrices(sc0, [beams], nudge)[0])
    return sc0, cam, w, h, chosen + [beams], np.stack(mats)


def test_a_pile_spills_the_stack_and_still_equals_a_rebuild():
    """The closest-hit walk keeps 12 stack entries per lane in LDS and spills deeper ones to a private array; neb_gi_node_index_stats
    out[4] counts the node phases that end with more than 12 entries.  On the pile it must be > 0 on the UPDATED context -- the spill
    path then walked a refitted tree -- and the frames equal the rebuild's.  Measured on an MI355X (docs/NOTEBOOK.md 10.17): 0 before
    the update; updated / rebuilt 1 451 / 174 at 1 spp, 6 029 / 624 at 4 spp, 1 455 / 146 with four path vertices; no tie on any frame."""
    sc0, cam, w, h, indices, mats = pile()
    sa, sb = clone(sc0), with_matrices(sc0, indices, mats)
    ra, rb = _renderer(sa, cam, w, h, sun_table=0), _renderer(sb, cam, w, h, sun_table=0)
    frame(ra, sa, cam, 2)
    before = ra.node_index_stats()["deep_stack_phases"]
    ra.update_transforms(indices, mats)
    for f, spp, mpv in ((3, 1, 2), (4, 4, 2), (5, 1, 4)):
        a, b = frame(ra, sa, cam, f, spp, mpv), frame(rb, sb, cam, f, spp, mpv)
        spill = ra.node_index_stats()["deep_stack_phases"], rb.node_index_stats()["deep_stack_phases"]
        print(f"[pile spp={spp} mpv={mpv}] node phases with more than 12 stack entries: before the update {before}, updated {spill[0]}, rebuilt {spill[1]}; "
              f"traversal {a['stats']} / {b['stats']}")
        assert spill[0] > 0, "the walk of the updated tree never went past its 12 LDS stack entries: the pile does not exercise the spill path"
        assert_same_frames(a, b, f"pile spp={spp} mpv={mpv}", hits_visible=(mpv == 2))
    ra.destroy(), rb.destroy()


def test_a_piled_context_matches_the_oracle():
    sc0, cam, w, h, indices, mats = pile()
    spill = _updated_against_oracle("pile", clone(sc0), with_matrices(sc0, indices, mats), cam, w, h, lambda r: r.update_transforms(indices, mats), LONGTHIN_BAR)
    assert spill > 0
