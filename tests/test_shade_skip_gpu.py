"""The shade pass on the LAST path vertex (gi_shade_kernel, nebulae_amd/csrc/gi.hip): a lane whose sun query an occluder hint answers
"occluded" adds nothing and leaves no ray, so it asks for no texture footprint and evaluates no BRDF; the other lanes ask behind the hint
tests instead of in front of them.  None of that may show: with the table on (lists), on with the sorted tail, and off, a frame is the
same bits -- radiance, hit records with their sun-visibility flags, ray counts.  The number of queries the table answers is compared
where it is a fixed quantity: between frames of one context (one table), and between contexts with "gi_sun_hints" = 0.  Two builds of a
table for the same scene and sun choose a few hints differently (ties taken in order of arrival), so with hints on two contexts' counts
differ by a few queries in some thousand -- also before this change (4 436 against 4 433 between "gi_sun_table" = 1 and 2).

Frames of 100 x 52: 13 x 7 tiles of 8 x 8 with partial tiles on both edges (a wave with inactive lanes still passes the barrier and the
gather).  atrium_mixed_tex has materials without a bundle: the three-fetch path.

So that no case compares nothing, every table-on case asserts that the hints answered "occluded" for at least 10 % of the frames' sun
queries.  Counted as: the queries the table answers with the case's hints minus those it answers with "gi_sun_hints" = 0 on the same
frames (the lit proofs do not depend on the hints), over an upper bound of the queries -- half of all rays, as every query follows a
bounce ray that hit.  The one-sample, two-vertex frames check that count against the hit flags as well: it lies between (answered -
pixels flagged visible) and the pixels flagged occluded.  Sun and camera below were chosen for that share; what the build before this
change measured is noted at SHARES."""
import numpy as np
import pytest

from nebulae_amd import scene as S
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import PLANE_RADIANCE, SLOT_CURRENT
from test_gi_gpu import scenes

pytestmark = pytest.mark.gpu

W, H = 100, 52
SUN = (0.5, -1.0, -0.2)
MIN_SHARE = 0.10
MODES = (1, 2, 0)  # "gi_sun_table": lists, sorted tail, off (the reference of every comparison)
# SHARES: on the build before this change (the tests pass there too) the 84 share conditions of this file measured between 0.456 (the
# early-out scene, sorted tail, frame 2: 2 109 of at most 4 624 queries) and 0.606 (atrium_small, 1 spp, 3 vertices: 5 953 of at most
# 9 827); the plain one-sample two-vertex frame 0.586 / 0.588 (atrium_small / atrium_mixed_tex).  The bar is 0.10.


def _camera():
    return S.sponza_camera()


def _renderers(sc, cam, options=(), modes=MODES):
    rs = []
    for mode in modes:
        r = DeferredRenderer()
        r.sun.direction = SUN
        r.init(W, H)
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
        r.svgf.set_option("gi_sun_table", mode)
        if mode == 2:
            r.svgf.set_option("gi_sort_rays", 1)
        for key, value in options:
            r.svgf.set_option(key, value)
        rs.append(r)
    return rs


def _frame(r, sc, cam, f, spp=1, vertices=2, form="one call"):
    """-> radiance, hit records, rays, queries the table answered"""
    r.gi_ui.gi_samples_per_pixel = spp
    r.gi_ui.max_path_vertices = vertices
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
    r.submit_commands_gbuffer()
    r.svgf.upload(PLANE_RADIANCE, SLOT_CURRENT, np.full((H, W, 4), 0.125, np.float32))
    r.set_debug_hits(True)
    r.ray_count(reset=True)
    if form == "one call":
        r.submit_commands_gi_pathtrace()
    elif form == "two calls":
        r.submit_commands_gi_pathtrace_begin()
        r.submit_commands_gi_pathtrace_finish()
    else:  # "deferred": the sums stay in the records until neb_gi_resolve
        r.submit_commands_gi_pathtrace()
        r.submit_commands_gi_resolve()
    rad, hits, rays = r.svgf.download(PLANE_RADIANCE), r.download_hits(), r.ray_count()
    return rad, hits, rays, r.sun_table_stats()["rays_answered"]


def _same(a, b, answered=False):
    (ra, ha, na, ta), (rb, hb, nb, tb) = a, b
    assert np.array_equal(ra, rb), float(np.abs(ra - rb).max())
    for k in ("t", "geometry", "primitive"):
        assert np.array_equal(ha[k], hb[k]), k
    assert np.array_equal(ha["flags"] & 1, hb["flags"] & 1)  # sun visible: the table's answer == the traversal's
    assert na == nb                                         # a ray = a visibility query, however it is answered
    if answered:
        assert ta == tb


def _occluded_by_hints(r, sc, cam, f, spp, vertices, out, hints, label, form="one call"):
    """The share condition of the module's docstring for frame f of table-on renderer r, whose result is `out`."""
    rad, hits, rays, answered = out
    r.svgf.set_option("gi_sun_hints", 0)
    bare = _frame(r, sc, cam, f, spp, vertices, form)
    r.svgf.set_option("gi_sun_hints", hints)
    _same(out, bare)
    by_hints = answered - bare[3]
    share = by_hints / (rays // 2)
    print(f"[{label}] rays {rays}, answered {answered} (without hints {bare[3]}): hints answered 'occluded' {by_hints} = {share:.3f} of at most {rays // 2} queries")
    if spp == 1 and vertices == 2:
        hit = hits["t"] >= 0
        visible = int(((hits["flags"] & 1) != 0)[hit].sum())
        assert answered - visible <= by_hints <= int(hit.sum()) - visible, (answered, visible, by_hints, int(hit.sum()))
    assert share >= MIN_SHARE, (label, share)
    return by_hints


def _three_ways(sc, cam, spp, vertices, label, options=(), hints=4, frames=(2, 3)):
    rs = _renderers(sc, cam, options)
    outs = None
    for f in frames:
        outs = [_frame(r, sc, cam, f, spp, vertices) for r in rs]
        _same(outs[0], outs[2])
        _same(outs[1], outs[2])
        _same(outs[0], outs[1], answered=not hints)
        _same(outs[0], _frame(rs[0], sc, cam, f, spp, vertices), answered=True)
        assert outs[2][3] == 0
        if hints:
            for r, out, mode in zip(rs[:2], outs[:2], MODES):
                _occluded_by_hints(r, sc, cam, f, spp, vertices, out, hints, f"{label} table={mode} frame {f}")
    for r in rs:
        r.destroy()
    return outs


@pytest.mark.parametrize("vertices", [2, 3])
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("name", ["atrium_small", "atrium_mixed_tex"])
def test_samples_and_vertices(name, spp, vertices):
    """At three path vertices, vertex 2 is not the last one: it textures for the next bounce whatever its sun query gives, and vertex 3 skips."""
    sc = scenes()[name][0]()
    _three_ways(sc, _camera(), spp, vertices, f"{name} spp={spp} vertices={vertices}")


@pytest.mark.parametrize("hints", [0, 2, 4])
@pytest.mark.parametrize("name", ["atrium_small", "atrium_mixed_tex"])
def test_number_of_hints(name, hints):
    """"gi_sun_hints" = 0 (nothing to test: every lane asks where it always did), 2 (one pair) and 4 (both pairs: the lanes the first pair
    did not stop ask for their footprint beside the second pair's triangles).  Without hints no query can be answered by one: that case
    is the count the others are measured from and carries no share condition."""
    sc = scenes()[name][0]()
    outs = _three_ways(sc, _camera(), 1, 2, f"{name} hints={hints}", options=(("gi_sun_hints", hints),), hints=hints)
    assert outs[0][3] > 0  # (the table itself answers)


@pytest.mark.parametrize("name", ["atrium_small", "atrium_mixed_tex"])
def test_exact_arithmetic(name):
    """"gi_exact_shade" = 1: gi_shade_kernel<false>, the other instantiation of the same source."""
    sc = scenes()[name][0]()
    _three_ways(sc, _camera(), 1, 2, f"{name} exact", options=(("gi_exact_shade", 1),))
    _three_ways(sc, _camera(), 2, 3, f"{name} exact spp=2 vertices=3", options=(("gi_exact_shade", 1),), frames=(2,))


@pytest.mark.parametrize("name", ["atrium_small", "atrium_mixed_tex"])
def test_submeshes_hidden_without_attributes_and_without_material(name):
    """The early-outs of the surface reconstruction sit in front of the hint tests now.  Of the four submeshes with most shadowed receivers in
    the frame (the ones whose records carry hints), one loses its material (material < 0: the path ends after GN), one its tangent stream
    (`valid` = 0 in its shade header: the path ends at the hit), one is hidden (absent for every ray, also as an occluder a hint names), and
    the first stays as it is."""
    sc, cam = scenes()[name][0](), _camera()
    (probe,) = _renderers(sc, cam, modes=(1,))
    _, hits, _, _ = _frame(probe, sc, cam, 2)
    probe.destroy()
    shadowed = (hits["t"] >= 0) & ((hits["flags"] & 1) == 0)
    counts = np.bincount(hits["geometry"][shadowed].astype(np.int64), minlength=len(sc.geometries))
    order = [int(g) for g in np.argsort(-counts)[:4]]
    assert counts[order[3]] > 0, counts[order]
    keep, no_material, no_tangents, hidden = order
    sc.geometries[no_material]["material"] = -1
    sc.geometries[no_tangents]["tangents"] = None
    rs = _renderers(sc, cam)
    for r in rs:
        r.set_visible([hidden], False)
    for f in (2, 3):
        outs = [_frame(r, sc, cam, f) for r in rs]
        _same(outs[0], outs[2])
        _same(outs[1], outs[2])
        seen = set(int(g) for g in np.unique(outs[0][1]["geometry"][outs[0][1]["t"] >= 0]))
        assert {keep, no_material, no_tangents} <= seen and hidden not in seen, (order, sorted(seen))
        for r, out, mode in zip(rs[:2], outs[:2], MODES):
            _occluded_by_hints(r, sc, cam, f, 1, 2, out, 4, f"{name} early-outs table={mode} frame {f}")
    for r in rs:
        r.destroy()


@pytest.mark.parametrize("name", ["atrium_small", "atrium_mixed_tex"])
def test_two_call_form_and_deferred_resolve(name):
    """neb_gi_trace_begin + neb_gi_trace_finish, and "gi_defer_resolve" = 2 + neb_gi_resolve (the shade pass then finishes no pixel: it carries
    the sums), against the one-call frame with the table off."""
    sc, cam = scenes()[name][0](), _camera()
    (ref,) = _renderers(sc, cam, modes=(0,))
    for form, options in (("two calls", ()), ("deferred", (("gi_defer_resolve", 2),))):
        rs = _renderers(sc, cam, options, modes=(1, 2))
        for f in (2, 3):
            want = _frame(ref, sc, cam, f)
            outs = [_frame(r, sc, cam, f, form=form) for r in rs]
            for r, out, mode in zip(rs, outs, MODES):
                _same(out, want)
                if form == "two calls":  # (the same context and table in one call: the same answers too)
                    _same(out, _frame(r, sc, cam, f), answered=True)
                _occluded_by_hints(r, sc, cam, f, 1, 2, out, 4, f"{name} {form} table={mode} frame {f}", form)
        for r in rs:
            r.destroy()
    ref.destroy()
