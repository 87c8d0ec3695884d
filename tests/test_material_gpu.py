"""Materials and texels updated in place: neb_gi_update_materials, neb_gi_set_geometry_materials, neb_gi_update_textures[_device]
(DESIGN.md 3.4g).

None of the calls touches a triangle, a node or a shading record, so a context that reached a scene through them holds THE tree of a
context built from the edited scene: there are no ties to excuse.  Every G-buffer plane, the radiance, the hit records and the ray
counts are compared with np.array_equal on the bits, no pixel left out -- stricter than test_refit_gpu.assert_same_frames, which is
used only where geometry moved as well (composition)."""
import ctypes as C

import numpy as np
import pytest
import torch

import texture_tables_ref as T
from nebulae_amd import _lib, scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import PLANE_ALBEDO, PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE
from oracle_lib import OracleTracer
from svgf_cases import rel_l2
from test_gi_gpu import scenes, upload_gbuffer
from test_material_cpu import rectangles
from test_refit_gpu import (_bits, _renderer, assert_same_frames, cornell_camera, cornell_parts, frame, moved_matrices, with_matrices,
                            world_transform)

pytestmark = pytest.mark.gpu

W, H = 64, 48
F = np.float32


# ------------------------------------------------------------------------------------------------
# scenes and edits
# ------------------------------------------------------------------------------------------------
def copy_scene(sc):
    """a copy whose material list, texture list and geometry dicts are its own (vertex streams and images shared until replaced)"""
    out = S.Scene(sc.name + "-copy")
    out.materials, out.textures = [dict(m) for m in sc.materials], list(sc.textures)
    out.geometries = [dict(g) for g in sc.geometries]
    return out


def cornell_five():
    """the five submeshes of cornell_parts under five hand-made materials, one per submesh:
    0: three 256^2 maps, bundled;  1: an albedo-only 4x4 map (roughness and metalness from its factors);  2, 3: bundled 16^2 maps that SHARE
    one roughness-metalness map;  4: maps of three different sizes (8x4, 67x5, 256^2), all standalone -- its third map is material 0's, so
    that texture sits in a bundle and has a standalone table as well."""
    sc = cornell_parts(textured=False)
    sc.materials, sc.textures = [], []
    rng = np.random.default_rng(55)
    ta, tn, tr = (sc.add_texture(S._proc_texture(k, s)) for k, s in (("albedo", 11), ("normal", 12), ("rm", 13)))
    sc.add_material(textures=(ta, tn, tr))
    sc.add_material(albedo=(0.6, 0.5, 0.4, 1), rm=(0.7, 0.0), textures=(sc.add_texture(S._proc_texture("albedo", 21, 4)), -1, -1))
    shared = sc.add_texture(S._proc_texture("rm", 31, 16))
    for s in (41, 51):
        sc.add_material(textures=(sc.add_texture(S._proc_texture("albedo", s, 16)), sc.add_texture(S._proc_texture("normal", s + 1, 16)), shared))
    small = rng.integers(40, 256, (4, 8, 4), dtype=np.uint8)         # 8 columns x 4 rows
    bumps = rng.integers(100, 156, (5, 67, 4), dtype=np.uint8)       # 67 x 5: tangent-space normals near +z
    bumps[..., 2] = 255
    sc.add_material(textures=(sc.add_texture(small), sc.add_texture(bumps), tr))
    for gi, gm in enumerate(sc.geometries):
        gm["material"] = gi
    return sc


def apply_to_renderer(r, edits, stream=None):
    keep = []
    for e in edits:
        if e[0] == "factors":
            r.update_materials(e[1], albedo=e[2], rough_metal=e[3], stream=stream)
        elif e[0] == "assign":
            r.set_geometry_materials(e[1], e[2], stream=stream)
        else:
            _, tex, x, y, px, via = e
            if via == "device":  # rows inside a wider tensor: a pitch that is not tight, read in place
                wide = torch.zeros((px.shape[0], px.shape[1] + 3, 4), dtype=torch.uint8, device=f"cuda:{r.svgf.device}")
                wide[:, :px.shape[1]] = torch.from_numpy(px).to(wide.device)
                torch.cuda.current_stream().synchronize()  # (written: the update may be enqueued on any stream)
                keep.append(wide)
                px = wide[:, :px.shape[1]]
            r.update_texture(tex, px, x=x, y=y, stream=stream)
    return keep  # (device sources stay alive until the caller has synchronised)


def apply_to_scene(sc, edits):
    """the edited scene, written independently of the renderer's own mirror"""
    out = copy_scene(sc)
    for e in edits:
        if e[0] == "factors":
            for k, mi in enumerate(e[1]):
                m = out.materials[mi]
                if e[2] is not None:
                    m["albedo"] = tuple(float(F(v)) for v in e[2][k][:3]) + (m["albedo"][3],)
                if e[3] is not None:
                    m["rm"] = tuple(float(F(v)) for v in e[3][k])
        elif e[0] == "assign":
            for gi, mi in zip(e[1], e[2]):
                out.geometries[gi]["material"] = int(mi)
        else:
            _, tex, x, y, px, _ = e
            full = out.textures[tex].copy()
            full[y:y + px.shape[0], x:x + px.shape[1]] = px
            out.textures[tex] = full
    return out


def rectangle_edits(sc, textures, seed):
    """the CPU test's rectangle lists on each of `textures`, sources random, the host and the device call taking turns"""
    rng = np.random.default_rng(seed)
    edits = []
    for tex in textures:
        h, w = sc.textures[tex].shape[:2]
        for rects in rectangles(w, h).values():
            for (x, y, rw, rh) in rects:
                edits.append(("texels", tex, x, y, rng.integers(0, 256, (rh, rw, 4), dtype=np.uint8), ("host", "device")[len(edits) % 2]))
    return edits


def scene_only(sc):
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=4)
    r.init_pathtracer_scene(sc)
    return r


def assert_equal_frames(a, b, what):
    """every plane, the radiance, the hit records and the ray counts: the same bits, no pixel left out"""
    for name in ("depth", "normal", "world_pos", "albedo", "radiance"):
        diff = (_bits(a[name]) != _bits(b[name])).any(-1)
        assert not diff.any(), f"{what}: {name} differs at {int(diff.sum())} pixels"
    assert np.array_equal(a["hits"].view(np.uint8), b["hits"].view(np.uint8)), f"{what}: hit records differ"
    assert a["rays"] == b["rays"], (what, a["rays"], b["rays"])


# ------------------------------------------------------------------------------------------------
# 1: tables
# ------------------------------------------------------------------------------------------------
def _tables_case(sc0, textures, seed, extra=()):
    edits = rectangle_edits(sc0, textures, seed) + list(extra)
    sa = copy_scene(sc0)
    ra = scene_only(sa)
    before = ra.texture_tables()
    assert np.array_equal(before, T.tables(sc0))  # (the restatement agrees with neb_gi_set_scene before anything is patched)
    bytes0 = ra.scene_bytes()
    keep = apply_to_renderer(ra, edits)
    got = ra.texture_tables()
    del keep
    assert not np.array_equal(got, before)
    sb = apply_to_scene(sc0, edits)
    rb = scene_only(sb)
    want = rb.texture_tables()
    assert got.size == want.size > 0 and ra.scene_bytes() == bytes0 == rb.scene_bytes()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from a fresh context's tables"
    assert np.array_equal(got, T.tables(sb))
    assert all(np.array_equal(x, y) for x, y in zip(sa.textures, sb.textures))  # the renderer's scene followed
    ra.destroy(), rb.destroy()
    return len(edits)


def test_tables_after_rectangle_updates_equal_a_fresh_scenes_on_the_mixed_atrium():
    sc0 = scenes()["atrium_mixed_tex"][0]()
    mats = [m["textures"] for m in sc0.materials]
    use = T.uses(mats, sc0.textures)
    # one texture of every kind this scene has: standalone only (64^2 and the 48x32 normal map), bundled only, the 4x4 map, and a
    # roughness-metalness map shared by a bundled and two unbundled materials (standalone AND in a bundle)
    both = [t for t, (alone, b) in use.items() if alone and b]
    only_alone = [t for t, (alone, b) in use.items() if alone and not b]
    only_bundle = [t for t, (alone, b) in use.items() if not alone and b]
    nonsquare = [t for t in only_alone if sc0.textures[t].shape[0] != sc0.textures[t].shape[1]]
    tiny = [t for t in only_alone if sc0.textures[t].shape[0] == 4]
    assert both and only_bundle and nonsquare and tiny
    picked = [both[0], only_bundle[0], only_bundle[1], nonsquare[0], tiny[0], mats[0][0]]
    _tables_case(sc0, picked, seed=7)


def test_tables_after_rectangle_updates_equal_a_fresh_scenes_on_the_five_material_cornell():
    sc0 = cornell_five()
    use = T.uses([m["textures"] for m in sc0.materials], sc0.textures)
    assert use[2] == (True, [(0, T.ROLE_RM)]) and use[4] == (False, [(2, T.ROLE_RM), (3, T.ROLE_RM)]) and use[3] == (True, [])
    rng = np.random.default_rng(8)
    # every texture but the two 256^2 maps only material 0 uses; of those, ONE full 256 x 256 update each way: 65 536 entries, 256 workgroups
    extra = [("texels", 0, 0, 0, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), "host"),
             ("texels", 1, 0, 0, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), "device")]
    _tables_case(sc0, [2, 3, 4, 5, 6, 7, 8, 9, 10], seed=9, extra=extra)


# ------------------------------------------------------------------------------------------------
# 2: frames
# ------------------------------------------------------------------------------------------------
def _edit_script(sc, rng):
    """factor updates, reassignments (to none and back, to another material) and texel updates on every table kind of the scene"""
    nm, ng = len(sc.materials), len(sc.geometries)
    texels = []
    for tex in range(len(sc.textures)):
        h, w = sc.textures[tex].shape[:2]
        rw, rh = max(1, (2 * w) // 3), max(1, (2 * h) // 3)
        texels.append(("texels", tex, w - rw, 0, rng.integers(0, 256, (rh, rw, 4), dtype=np.uint8), ("host", "device")[tex % 2]))
    return [("factors", list(range(nm)), rng.uniform(0.1, 0.9, (nm, 3)).astype(F), rng.uniform(0.2, 1.0, (nm, 2)).astype(F)),
            ("assign", [1, 2], [-1, -1]),
            ("factors", [nm - 1], None, np.array([[0.35, 0.0]], F)),
            ("assign", [2, 3, 1], [sc.geometries[2]["material"], (sc.geometries[3]["material"] + 1) % nm, 0])] + texels


def _restore_script(sc0, sa):
    """the edits that bring `sa` back to sc0"""
    nm = len(sc0.materials)
    return [("factors", list(range(nm)), np.array([m["albedo"][:3] for m in sc0.materials], F), np.array([m["rm"] for m in sc0.materials], F)),
            ("assign", list(range(len(sc0.geometries))), [g["material"] for g in sc0.geometries])] + \
           [("texels", t, 0, 0, sc0.textures[t], ("device", "host")[t % 2]) for t in range(len(sc0.textures))]


@pytest.mark.parametrize("sun_table", [0, 1])
@pytest.mark.parametrize("which", ["cornell_parts", "cornell_five"])
def test_frames_after_updates_equal_a_fresh_context_and_restoring_restores(which, sun_table):
    sc0 = cornell_parts() if which == "cornell_parts" else cornell_five()
    cam = cornell_camera()
    edits = _edit_script(sc0, np.random.default_rng(3))
    sa, sb, sn = copy_scene(sc0), apply_to_scene(sc0, edits), copy_scene(sc0)
    ra, rb, rn = (_renderer(s, cam, W, H, sun_table=sun_table) for s in (sa, sb, sn))
    for r, s in ((ra, sa), (rb, sb), (rn, sn)):
        frame(r, s, cam, 2)  # (a dispatch before the update: with the table on, the hold of two dispatches has begun)
    keep = apply_to_renderer(ra, edits)
    moved = False
    for f, spp in ((3, 1), (4, 4), (5, 1)):
        a, b, n = frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp), frame(rn, sn, cam, f, spp)
        assert float(a["radiance"][..., :3].max()) > 0.05
        assert_equal_frames(a, b, f"{which} table={sun_table} frame {f} spp {spp}")
        moved = moved or not np.array_equal(a["radiance"], n["radiance"])
    assert moved  # (the edits are visible: the comparison above is not one of two untouched scenes)
    if sun_table:  # the table survived: one build in either context, and it was not dropped in between
        assert ra.sun_table_stats()["builds"] == rb.sun_table_stats()["builds"] == 1
    keep += apply_to_renderer(ra, _restore_script(sc0, sa))
    for f, spp in ((6, 1), (7, 4)):
        frame(rb, sb, cam, f, spp)
        a, n = frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp)
        assert_equal_frames(a, n, f"{which} table={sun_table} restored, frame {f}")
    assert np.array_equal(ra.texture_tables(), rn.texture_tables())
    assert ra.sun_table_stats()["builds"] == rn.sun_table_stats()["builds"]
    for r in (ra, rb, rn):
        r.destroy()


def test_updates_before_the_first_build_and_a_build_after_them():
    """the calls need a scene only; a later neb_gi_build_bvh keeps what they set"""
    sc0, cam = cornell_five(), cornell_camera()
    edits = _edit_script(sc0, np.random.default_rng(4))
    sa, sb = copy_scene(sc0), apply_to_scene(sc0, edits)
    ra = DeferredRenderer()
    ra.init(W, H, atrous_levels=4)
    G, ng, M, nm, Tx, nt = sa.descs()
    ra._check(ra._lib.neb_gi_set_scene(ra._ctx, G, ng, M, nm, Tx, nt), "neb_gi_set_scene")
    ra._scene = sa
    keep = apply_to_renderer(ra, edits)  # no tree yet
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")
    ra.set_debug_hits(True)
    ra._hits_on = True
    rb = _renderer(sb, cam, W, H, exact=False)
    for f in (2, 3):
        assert_equal_frames(frame(ra, sa, cam, f), frame(rb, sb, cam, f), f"edited before the build, frame {f}")
    ra._check(ra._lib.neb_gi_build_bvh(ra._ctx, C.c_void_p(0)), "neb_gi_build_bvh")  # ... and again after frames
    for f in (4, 5):
        assert_equal_frames(frame(ra, sa, cam, f), frame(rb, sb, cam, f), f"rebuilt after the edits, frame {f}")
    del keep
    ra.destroy(), rb.destroy()


# ------------------------------------------------------------------------------------------------
# 3: the oracle
# ------------------------------------------------------------------------------------------------
def test_an_updated_context_matches_the_oracle_on_the_edited_scene():
    """test_gi_gpu.test_gi_matches_oracle's comparison, at its bars, under gi_exact_shade, for a context that reached the scene through one
    update of each kind: the result is pinned to the checker, not only to this back end's own fresh context."""
    sc0, cam, w, h = cornell_parts(), cornell_camera(), 96, 72
    rng = np.random.default_rng(6)
    edits = [("factors", [1, 3], np.array([[0.2, 0.6, 0.7], [0.8, 0.7, 0.2]], F), np.array([[0.5, 0.0], [0.9, 0.0]], F)),
             ("assign", [2], [3]),
             ("texels", 0, 64, 32, rng.integers(0, 256, (128, 160, 4), dtype=np.uint8), "host")]
    sa = copy_scene(sc0)
    r = DeferredRenderer()
    r.init(w, h, atrous_levels=4)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=4))
    r.svgf.set_option("gi_exact_shade", 1)
    apply_to_renderer(r, edits)
    sm = apply_to_scene(sc0, edits)
    o = OracleTracer(sm)
    gb = o.gbuffer(w, h, cam)
    r.begin_frame(RenderInfo(scene=sa, camera=cam, frame_index=5))
    upload_gbuffer(r, gb)
    base = np.full((h, w, 4), 0.25, F)
    base[..., 3] = 1.0
    r.svgf.upload(PLANE_RADIANCE, -1, base)
    r.set_debug_hits(True)
    r.ray_count(reset=True)
    r.submit_commands_gi_pathtrace()
    got, hits, rays = r.svgf.download(PLANE_RADIANCE), r.download_hits(), r.ray_count()
    want, ohits, orays = o.gi(gb, r.global_constants(), radiance=base.copy())
    same = (hits["geometry"] == ohits["geometry"]) & (hits["primitive"] == ohits["primitive"]) & ((hits["flags"] & 1) == (ohits["flags"] & 1))
    print(f"[oracle, edited cornell] hit mismatch {1.0 - same.mean():.2e}, rays {rays} / {orays}, rel-L2 {rel_l2(got[..., :3], want[..., :3]):.2e}, "
          f"on agreeing pixels {rel_l2(got[same][:, :3], want[same][:, :3]):.2e}")
    assert 1.0 - same.mean() <= 2e-4
    assert abs(rays - orays) <= max(4, 4e-4 * orays)
    assert np.array_equal(got[..., 3], base[..., 3])
    assert rel_l2(got[..., :3], want[..., :3]) <= 2e-3
    assert rel_l2(got[same][:, :3], want[same][:, :3]) <= 2e-5
    t_err = np.abs(hits["t"][same] - ohits["t"][same]) / np.maximum(np.abs(ohits["t"][same]), 1e-6)
    assert t_err.max() <= 1e-4
    r.destroy()
    o.close()


# ------------------------------------------------------------------------------------------------
# 4: composition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["material_first", "material_last"])
def test_material_updates_between_the_other_update_calls_equal_a_rebuild(order):
    sc0, cam = cornell_parts(), cornell_camera()
    rng = np.random.default_rng(12)
    mats = moved_matrices(sc0, [1, 2], world_transform("rotate"))
    bent = (sc0.geometries[2]["positions"] * F(0.9)).astype(F)
    look = [("factors", [1, 2], np.array([[0.3, 0.4, 0.8], [0.7, 0.2, 0.3]], F), None), ("assign", [4, 2], [3, 1]),
            ("texels", 0, 10, 200, rng.integers(0, 256, (56, 200, 4), dtype=np.uint8), "device")]
    sa = copy_scene(sc0)
    ra = _renderer(sa, cam, W, H)
    frame(ra, sa, cam, 2)
    steps = [lambda: ra.update_transforms([1, 2], mats), lambda: ra.update_vertices(2, bent), lambda: ra.set_visible([3], False)]
    keep = []
    if order == "material_first":
        keep += apply_to_renderer(ra, look[:1])
        steps[0](), steps[1]()
        keep += apply_to_renderer(ra, look[1:])
        steps[2]()
    else:
        steps[2](), steps[0]()
        keep += apply_to_renderer(ra, look[:2])
        steps[1]()
        keep += apply_to_renderer(ra, look[2:])
    sb = apply_to_scene(with_matrices(sc0, [1, 2], mats), look)
    sb.geometries[2]["positions"] = bent
    rb = _renderer(sb, cam, W, H)
    rb.set_visible([3], False)
    frame(rb, sb, cam, 2)
    for f, spp in ((3, 1), (4, 4), (5, 1)):
        assert_same_frames(frame(ra, sa, cam, f, spp), frame(rb, sb, cam, f, spp), f"composition {order} frame {f}")
    assert np.array_equal(ra.texture_tables(), rb.texture_tables())
    del keep
    ra.destroy(), rb.destroy()


def test_the_albedo_plane_follows_a_texel_update_under_demodulation():
    sc0, cam = cornell_parts(), cornell_camera()
    rng = np.random.default_rng(13)
    edits = [("texels", 0, 0, 0, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), "host")]
    sa, sb = copy_scene(sc0), apply_to_scene(sc0, edits)
    out = []
    for sc, late in ((sa, True), (sb, False)):
        r = DeferredRenderer()
        r.albedo_demodulation = True
        r.init(W, H)
        planes = []
        for f in (1, 2, 3, 4):
            if late and f == 2:
                apply_to_renderer(r, edits)
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
            r.submit_commands_gbuffer()
            r.submit_commands_pbr_lighting()
            r.submit_commands_gi_pathtrace()
            r.submit_commands_svgf_denoising()
            if f >= 2:
                planes.append((r.svgf.download(PLANE_ALBEDO, 0), r.svgf.download(PLANE_RADIANCE)))
            r.end_frame()
        out.append(planes)
        r.destroy()
    assert np.array_equal(_bits(out[0][0][0]), _bits(out[1][0][0])) and np.array_equal(_bits(out[0][-1][0]), _bits(out[1][-1][0]))
    fresh = DeferredRenderer()
    fresh.init(W, H)
    fresh.begin_frame(RenderInfo(scene=copy_scene(sc0), camera=cam, frame_index=1))
    fresh.submit_commands_gbuffer()
    assert not np.array_equal(fresh.svgf.download(PLANE_ALBEDO, 0), out[0][0][0])  # (the update is visible in the plane)
    fresh.destroy()


# ------------------------------------------------------------------------------------------------
# 5: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    sc0, cam = cornell_five(), cornell_camera()
    sa, sn = copy_scene(sc0), copy_scene(sc0)
    ra, rn = _renderer(sa, cam, W, H), _renderer(sn, cam, W, H)
    lib, ctx = ra._lib, ra._ctx
    bytes0, tables0 = ra.scene_bytes(), ra.texture_tables()
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)

    def descs(indices, **change):
        d = (S.MaterialDesc * max(1, len(indices)))()
        for k, mi in enumerate(indices):
            m = sc0.materials[min(mi, len(sc0.materials) - 1)]
            d[k].textureIndices[:] = change.get("textures", m["textures"])
            d[k].albedo[:] = change.get("albedo", m["albedo"])
            d[k].roughnessMetalness[:] = change.get("rm", m["rm"])
        return d

    def factors(indices, n=None, **change):
        idx = np.asarray(indices, np.uint32)
        return lib.neb_gi_update_materials(ctx, idx.ctypes.data_as(u32p), descs(indices, **change), len(indices) if n is None else n, None)

    def assign(geoms, mats):
        g, m = np.asarray(geoms, np.uint32), np.asarray(mats, np.int32)
        return lib.neb_gi_set_geometry_materials(ctx, g.ctypes.data_as(u32p), m.ctypes.data_as(i32p), len(geoms), None)

    host_px = np.full((8, 8, 4), 200, np.uint8)
    dev_px = torch.full((8, 8, 4), 200, dtype=torch.uint8, device="cuda")

    def texels(fn, ptr, tex=5, x=0, y=0, w=4, h=4, pitch=32):
        u = _lib.TextureUpdate(texture=tex, x=x, y=y, width=w, height=h, pitchBytes=pitch, rgba8=ptr)
        return fn(ctx, C.byref(u), 1, None)

    host, dev = lib.neb_gi_update_textures, lib.neb_gi_update_textures_device
    hp, dp = host_px.ctypes.data, dev_px.data_ptr()
    one = np.zeros(1, np.uint32)
    cases = [("factors: null indices", lambda: lib.neb_gi_update_materials(ctx, None, descs([0]), 1, None), -1),
             ("factors: null descs", lambda: lib.neb_gi_update_materials(ctx, one.ctypes.data_as(u32p), None, 1, None), -1),
             ("factors: index past the table", lambda: factors([5], rm=(0.1, 0.2)), -5),
             ("factors: index twice", lambda: factors([1, 4, 1], rm=(0.1, 0.2)), -1),
             ("factors: textureIndices differ", lambda: factors([1], textures=(3, 4, -1), rm=(0.1, 0.2)), -1),
             ("factors: a map taken away", lambda: factors([0], textures=(0, 1, -1), rm=(0.1, 0.2)), -1),
             ("factors: nan", lambda: factors([1], rm=(float("nan"), 0.0)), -5),
             ("factors: inf", lambda: factors([1], albedo=(0.1, float("inf"), 0.1, 1.0)), -5),
             ("assign: null", lambda: lib.neb_gi_set_geometry_materials(ctx, None, None, 1, None), -1),
             ("assign: geometry past the table", lambda: assign([5], [0]), -5),
             ("assign: geometry twice", lambda: assign([1, 1], [0, 2]), -1),
             ("assign: material past the table", lambda: assign([1], [5]), -5),
             ("texels: null array", lambda: host(ctx, None, 1, None), -1),
             ("texels: null source", lambda: texels(host, None), -1),
             ("texels (device): null source", lambda: texels(dev, None), -1),
             ("texels: texture past the table", lambda: texels(host, hp, tex=11), -5),
             ("texels: empty", lambda: texels(host, hp, w=0), -5),
             ("texels: leaves on the right", lambda: texels(host, hp, x=14, w=4), -5),
             ("texels: leaves at the bottom", lambda: texels(dev, dp, y=13, h=4), -5),
             ("texels: origin outside", lambda: texels(host, hp, x=16, w=1), -5),
             ("texels: wraps as 32-bit sum", lambda: texels(host, hp, x=0xFFFFFFFE, w=4), -5),
             ("texels: pitch below a row", lambda: texels(host, hp, pitch=12), -1),
             ("texels: pitch no multiple of 4", lambda: texels(dev, dp, pitch=34), -1),
             ("texels (device): host memory", lambda: texels(dev, hp), -1),
             ("texels (device): misaligned", lambda: texels(dev, dp + 2, w=2, h=2), -1),
             ("n == 0", lambda: lib.neb_gi_update_materials(ctx, None, None, 0, None) or lib.neb_gi_set_geometry_materials(ctx, None, None, 0, None) or
              host(ctx, None, 0, None) or dev(ctx, None, 0, None), 0),
             ("no-op factors", lambda: factors([0, 1, 2, 3, 4]), 0),
             ("no-op assignment", lambda: assign([0, 1, 2, 3, 4], [0, 1, 2, 3, 4]), 0)]
    # 300 rectangles of 256 KB, each valid on its own, make 75 MB in one host-sourced call
    many = (_lib.TextureUpdate * 300)(*[_lib.TextureUpdate(texture=0, x=0, y=0, width=256, height=256, pitchBytes=1024, rgba8=sc0.textures[0].ctypes.data)
                                        for _ in range(300)])
    cases.append(("texels: more than 64 MB in one call", lambda: host(ctx, many, 300, None), -5))
    for what, call, want in cases:
        assert call() == want, what
    assert ra.scene_bytes() == bytes0
    assert np.array_equal(ra.texture_tables(), tables0)
    for f, spp in ((2, 1), (3, 4)):
        assert_equal_frames(frame(ra, sa, cam, f, spp), frame(rn, sn, cam, f, spp), f"after the refusals, frame {f}")
    # without a scene: NEB_ERR_STATE
    bare = DeferredRenderer()
    bare.init(W, H, atrous_levels=4)
    n = C.c_size_t(0)
    assert bare._lib.neb_gi_update_materials(bare._ctx, one.ctypes.data_as(u32p), descs([0]), 1, None) == -4
    assert bare._lib.neb_gi_set_geometry_materials(bare._ctx, one.ctypes.data_as(u32p), np.zeros(1, np.int32).ctypes.data_as(i32p), 1, None) == -4
    u = _lib.TextureUpdate(texture=0, x=0, y=0, width=1, height=1, pitchBytes=4, rgba8=hp)
    assert bare._lib.neb_gi_update_textures(bare._ctx, C.byref(u), 1, None) == -4
    assert bare._lib.neb_gi_update_textures_device(bare._ctx, C.byref(u), 1, None) == -4
    assert bare._lib.neb_gi_debug_texture_tables(bare._ctx, None, 0, C.byref(n), None) == -4
    for r in (ra, rn, bare):
        r.destroy()


# ------------------------------------------------------------------------------------------------
# 6: two streams
# ------------------------------------------------------------------------------------------------
def test_material_updates_with_two_dispatches_in_flight_on_two_streams():
    """test_refit_gpu.test_updates_with_two_dispatches_in_flight_on_two_streams with the scene's look changing instead of its pose: a texel
    update, a factor update and a reassignment are enqueued on a stream of their own while the previous frame's dispatch is in flight on a
    side stream ("gi_defer_resolve" = 2), and the next dispatch goes to the other side stream.  Nothing but the library orders them; the
    denoised sequence equals the serial one."""
    make, cam, w, h = scenes()["atrium_small"]
    sc0 = make()
    named = [3, 11, 12, 27, 41, 58]
    nm = len(sc0.materials)
    outs = []
    for mode in ("plain", "two_streams"):
        rng = np.random.default_rng(21)
        sc = copy_scene(sc0)
        r = DeferredRenderer()
        r.init(w, h, atrous_levels=4)
        main = torch.cuda.current_stream()
        sides = [torch.cuda.Stream() for _ in range(2)]
        mover = torch.cuda.Stream()
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1, stream=main.cuda_stream))
        r.submit_commands_gbuffer()
        torch.cuda.synchronize()
        for pl in (PLANE_NORMAL, PLANE_DEPTH):
            r.svgf.plane_tensor(pl, 0).copy_(r.svgf.plane_tensor(pl, 1))
        rad = [r.svgf.plane_tensor(PLANE_RADIANCE, 0), r.svgf.plane_tensor(PLANE_RADIANCE, 1)]
        direct = torch.full_like(rad[0], 0.125)
        r.svgf.set_option("gi_sun_hold", 2)
        if mode == "two_streams":
            r.set_defer_resolve(2)
        resolved = [None, None]
        keep = []
        for f in range(2, 16):
            if f in (4, 5, 6, 9, 13):
                st = (mover if mode == "two_streams" else main).cuda_stream
                edits = [("texels", sc0.materials[f]["textures"][0], f, f, rng.integers(0, 256, (40, 48, 4), dtype=np.uint8), "host"),
                         ("texels", sc0.materials[14]["textures"][2], 0, f, rng.integers(0, 256, (16, 64, 4), dtype=np.uint8), "device"),
                         ("factors", [2, f], rng.uniform(0.1, 0.9, (2, 3)).astype(F), rng.uniform(0.2, 1.0, (2, 2)).astype(F)),
                         ("assign", named, [(sc0.geometries[g]["material"] + f) % nm for g in named])]
                keep += apply_to_renderer(r, edits, stream=st)
            side, slot = sides[f % 2], f % 2
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f, stream=main.cuda_stream))
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
            r.end_frame()
        torch.cuda.synchronize()
        outs.append((r.svgf.download(PLANE_RADIANCE), r.texture_tables()))
        del keep
        r.destroy()
    assert float(np.abs(outs[0][0][..., :3]).max()) > 0.2
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0], outs[1][0])


# ------------------------------------------------------------------------------------------------
# 7: strips
# ------------------------------------------------------------------------------------------------
def test_two_strip_contexts_given_the_same_updates_equal_the_full_frame():
    sc0, cam = cornell_five(), cornell_camera()
    edits = _edit_script(sc0, np.random.default_rng(17))
    cut = 24  # (a multiple of the 8-row tiles)
    sf, s_up, s_dn = copy_scene(sc0), copy_scene(sc0), copy_scene(sc0)
    full = _renderer(sf, cam, W, H)
    up = _renderer(s_up, cam, W, H, row_begin=0, row_end=cut)
    dn = _renderer(s_dn, cam, W, H, row_begin=cut, row_end=H)
    keep = []
    for r in (full, up, dn):
        keep += apply_to_renderer(r, edits)
    for f, spp in ((2, 1), (3, 4)):
        a, u, d = frame(full, sf, cam, f, spp), frame(up, s_up, cam, f, spp), frame(dn, s_dn, cam, f, spp)
        for name in ("radiance", "depth", "normal", "world_pos", "albedo"):
            assert np.array_equal(_bits(a[name]), _bits(np.concatenate([u[name], d[name]], axis=0))), (name, f)
        assert np.array_equal(a["hits"], np.concatenate([u["hits"], d["hits"]], axis=0))
        assert a["rays"] == u["rays"] + d["rays"]
    assert np.array_equal(full.texture_tables(), up.texture_tables()) and np.array_equal(full.texture_tables(), dn.texture_tables())
    del keep
    for r in (full, up, dn):
        r.destroy()
