"""The judge of tests/ray_query_ref.py shown to be right, and able to fail, before a device is involved; and the calibration its
tolerances and caps rest on: a float32 evaluation of every ray set on every scene state of tests/test_ray_query_gpu.py, through the
judge, against float64."""
import numpy as np
import pytest

import ray_query_ref as Q
from motion_ref import NO_SUBMESH

F = np.float32


@pytest.fixture(scope="module")
def room():
    sc, hidden = Q.states()["room"]
    tris = Q.triangles(sc, hidden)
    sets = Q.ray_sets(*Q.scene_box(sc), tris)
    refs = {name: Q.reference(tris, sets[name]) for name in Q.SETS}
    return tris, sets, refs


def test_the_judge_accepts_float64s_own_answers(room):
    tris, sets, refs = room
    for name in Q.SETS:
        v = Q.judge(tris, sets[name], refs[name], Q.answers(refs[name]))
        assert Q.check(v, f"float64 / {name}", cap=0) == 0
        assert not v["tie"].any() and v["err_t"] < 1e-12 and v["err_u"] < 1e-12 and v["err_v"] < 1e-12
        assert Q.check_any_hit(refs[name]["hit"].astype(np.uint32), refs[name], f"float64 / {name}", cap=0) == 0
    assert not refs["short"]["hit"][refs["scattered"]["hit"]].any()  # (cut short: float64 says miss for every ray that had a hit)
    assert refs["scattered"]["hit"].sum() > Q.N_RAYS // 2


def _partners(tris, rays, ref):
    """brute force: for every ray that hits, another triangle float64 puts at the same distance, inside -> (rays, their partners)"""
    rows, partners = [], []
    nt = len(tris[3])
    for k in np.nonzero(ref["hit"])[0]:
        t, u, v = Q.moller_trumbore(tris, np.arange(nt), np.broadcast_to(rays[k], (nt, 8)))
        with np.errstate(all="ignore"):
            ok = (np.abs(t - ref["t"][k]) <= 1e-12 * max(1.0, ref["t"][k])) & (u >= 0) & (v >= 0) & (u + v <= 1)
        ok &= ~((tris[3] == ref["geometry"][k]) & (tris[4] == ref["primitive"][k]))
        if ok.any():
            rows.append(k)
            partners.append(int(np.nonzero(ok)[0][0]))
    return np.array(rows, np.int64), np.array(partners, np.int64)


def test_the_judge_accepts_a_swapped_coincident_triangle(room):
    tris, sets, refs = room
    # (seen from outside, from below: the boxes stand on the floor, their bottom faces lie in the floor's plane)
    rays, ref = sets["outside"][:1024], {k: v[:1024] for k, v in refs["outside"].items()}
    rows, partners = _partners(tris, rays, ref)
    print(f"[coincident] {len(rows)} of {int(ref['hit'].sum())} hits have a second triangle at the same distance")
    assert len(rows) >= 8, "the room holds no coincident surfaces: nothing to swap"
    got = Q.answers(ref)
    t, u, v = Q.moller_trumbore(tris, partners, rays[rows])
    got["geometry"][rows], got["primitive"][rows] = tris[3][partners], tris[4][partners]
    got["t"][rows], got["u"][rows], got["v"][rows] = t, u, v
    verdict = Q.judge(tris, rays, ref, got)
    assert Q.check(verdict, "swapped", cap=0) == 0
    assert int(verdict["tie"].sum()) == len(rows)


PLANTED = 3 * Q.TIE_CAP


def _plant(room, kind):
    """-> (rays, ref, tampered answers, the tampered rays): PLANTED real rays of the room given an answer of the kind"""
    tris, sets, refs = room
    rays, ref = sets["scattered"], refs["scattered"]
    got = Q.answers(ref)
    behind = refs["second"]  # the same rays' next surface
    if kind == "next surface behind":
        # (not where the surface behind is a coincident twin of the first: that swap is right)
        far = ref["hit"] & behind["hit"] & (behind["t"] > ref["t"] * 1.01 + 1e-3)
        rows = np.nonzero(far)[0][:PLANTED]
        for k in ("t", "u", "v", "geometry", "primitive"):
            got[k][rows] = behind[k][rows]
    elif kind == "miss where there is a hit":
        rows = np.nonzero(ref["hit"])[0][:PLANTED]
        got["t"][rows], got["u"][rows], got["v"][rows] = np.inf, 0.0, 0.0
        got["geometry"][rows] = got["primitive"][rows] = NO_SUBMESH
    elif kind == "hit where there is none":
        ref = refs["short"]  # every ray a miss
        rays, got = sets["short"], Q.answers(refs["short"])
        first = refs["scattered"]
        rows = np.nonzero(first["hit"])[0][:PLANTED]
        for k in ("t", "u", "v", "geometry", "primitive"):
            got[k][rows] = first[k][rows]  # the surface beyond the ray's tmax
    elif kind == "t off by ten tolerances":
        rows = np.nonzero(ref["hit"])[0][:PLANTED]
        got["t"][rows] = ref["t"][rows] + 10.0 * Q.T_TOL * np.maximum(1.0, ref["t"][rows])
    assert len(rows) == PLANTED
    return rays, ref, got, rows


@pytest.mark.parametrize("kind", ["next surface behind", "miss where there is a hit", "hit where there is none", "t off by ten tolerances"])
def test_the_judge_rejects(room, kind):
    tris = room[0]
    rays, ref, got, rows = _plant(room, kind)
    verdict = Q.judge(tris, rays, ref, got)
    flagged = verdict["off"] if kind.startswith("t off") else verdict["wrong"]
    assert np.array_equal(np.nonzero(flagged)[0], rows), kind  # exactly the tampered rays
    with pytest.raises(AssertionError):
        Q.check(verdict, kind)
    if kind in ("miss where there is a hit", "hit where there is none"):
        with pytest.raises(AssertionError):
            Q.check_any_hit((got["geometry"] != NO_SUBMESH).astype(np.uint32), ref, kind)


def test_a_single_tampered_t_is_enough(room):
    tris, sets, refs = room
    got = Q.answers(refs["outside"])
    k = int(np.nonzero(refs["outside"]["hit"])[0][5])
    got["t"][k] *= 1.0 + 10.0 * Q.T_TOL
    with pytest.raises(AssertionError):
        Q.check(Q.judge(tris, sets["outside"], refs["outside"], got), "one t")


def test_calibration():
    """float32 against float64 through the judge, every set on every state of the GPU tests: at most TIE_CAP // 2 wrong rays and
    any-hit flags (measured: 0 and 0), every disagreement a coincident triangle, and the error maxima that T_TOL, U_TOL, V_TOL are
    four times of -- printed, and held to the recorded values so that the constants cannot drift from what they claim to be."""
    worst = dict(t=0.0, u=0.0, v=0.0)
    for sname, (sc, hidden) in Q.states().items():
        tris = Q.triangles(sc, hidden)
        assert not len(hidden) or not (tris[3] == Q.HIDDEN).any()
        sets = Q.ray_sets(*Q.scene_box(sc), tris)
        for name in Q.SETS:
            ref, f32 = Q.reference(tris, sets[name]), Q.reference(tris, sets[name], F)
            verdict = Q.judge(tris, sets[name], ref, Q.answers(f32))
            n_wrong = Q.check(verdict, f"float32 / {sname} / {name}", cap=Q.TIE_CAP // 2)
            n_any = Q.check_any_hit(f32["hit"].astype(np.uint32), ref, f"float32 / {sname} / {name}", cap=Q.TIE_CAP // 2)
            seen = Q.submeshes_seen(name, sets, ref, tris)
            print(f"[calibration {sname} / {name}] wrong {n_wrong}, any-hit {n_any}, ties {int(verdict['tie'].sum())}, hits {int(ref['hit'].sum())}, submeshes {seen}")
            assert len(seen) >= 6, (sname, name, seen)  # what the GPU test asserts of its sets
            for k in worst:
                worst[k] = max(worst[k], verdict["err_" + k])
    print(f"[calibration] largest float32 errors: t {worst['t']:.3e} (relative to max(1, t)), u {worst['u']:.3e}, v {worst['v']:.3e}")
    # (2 %: room for a numpy that rounds a sum of three products in another order)
    assert worst["t"] <= 1.02 * Q.T_MEASURED and worst["u"] <= 1.02 * Q.U_MEASURED and worst["v"] <= 1.02 * Q.V_MEASURED, worst
    assert worst["t"] >= 0.5 * Q.T_MEASURED and worst["u"] >= 0.5 * Q.U_MEASURED and worst["v"] >= 0.5 * Q.V_MEASURED, worst
