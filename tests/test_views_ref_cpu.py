"""tests/views_ref.py, the brute-force caster of tests/test_update_views_gpu.py, checked on the CPU: against the caster it
generalises, against the oracle's G-buffer, and -- the condition under which the GPU tests may cap their disagreement with it at
TIE_CAP -- float32 against float64 at every (scene state, camera) pair those tests use."""
import numpy as np
import pytest

import motion_ref as M
import views_ref as V
from oracle_lib import OracleTracer
from test_refit_gpu import TIE_CAP, cornell_camera, cornell_parts


def test_float64_caster_agrees_with_primary_ids():
    sc, cam, w, h = cornell_parts(), cornell_camera(), 64, 48
    ids, t = M.primary_ids(sc, cam, w, h)
    got = V.primary(sc, cam, w, h)
    assert (ids != M.NO_SUBMESH).sum() > 0.25 * w * h and {0, 1, 2} <= set(ids.reshape(-1).tolist())
    assert np.array_equal(got["geometry"], ids)
    hit = np.isfinite(t)
    assert np.array_equal(np.isfinite(got["t"]), hit) and np.abs(got["t"][hit] - t[hit]).max() <= 1e-12  # (the same formulas in float64, summed in another order)
    # primitives count within their geometry, and a ray list with origins of its own gives what the shared origin gives
    tris = V.triangles(sc)
    assert 2 < got["primitive"][got["geometry"] == 1].max() < 12 and got["primitive"][got["geometry"] == 3].max() <= 1
    assert sum(len(g["indices"]) // 3 for g in sc.geometries) == len(tris[3])


def test_caster_agrees_with_the_oracles_coverage():
    """the oracle's G-buffer marks covered pixels in the top byte of its depth plane (test_gbuffer_raycast_matches_oracle); two views
    of the beamed room, one of them with objects beyond the default far plane's reach"""
    sc0, _, _, far = V.carried_updates()
    for name, sc, cam in (("room", sc0, cornell_camera()), ("looking back", far, V.outside_views()["looking back"])):
        gb = OracleTracer(sc).gbuffer(V.VW, V.VH, cam)
        got = V.primary(sc, cam, V.VW, V.VH)
        differ = ((gb["depth"] >> 24) == 0xFF) != got["covered"]
        print(f"[views_ref] {name}: {int(got['covered'].sum())} covered pixels, {int(differ.sum())} differ from the oracle")
        assert got["covered"].any() and int(differ.sum()) <= TIE_CAP // 2


def test_the_room_has_triangles_the_builder_splits():
    """(a prediction of gi_build.hip's reference splitting from its area rule; the GPU test asserts the references themselves)"""
    sc = V.beamed_room()
    big, gi = V.oversized(sc)
    print(f"[views_ref] beamed room: {sc.num_triangles} triangles, {int(big.sum())} oversized, in submeshes {sorted(set(gi[big].tolist()))}")
    assert 1200 <= sc.num_triangles <= 1400
    assert {0, V.BEAMS, V.POST} <= set(gi[big].tolist()) and V.RUG not in set(gi[big].tolist())


CASES = V.view_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_and_float64_differ_at_few_pixels_of_every_view(name):
    sc, cam, w, h = CASES[name]
    tris = V.triangles(sc)
    a, b = V.primary(sc, cam, w, h, np.float64, tris), V.primary(sc, cam, w, h, np.float32, tris)
    n = int(V.differing(a, b).sum())
    print(f"[views_ref] {name}: {int(a['covered'].sum())} of {w * h} pixels covered, submeshes {sorted(set(a['geometry'][a['covered']].tolist()))}, "
          f"float32 differs at {n}")
    assert int(a["covered"].sum()) >= 100  # (the view looks at something)
    assert n <= TIE_CAP // 2
