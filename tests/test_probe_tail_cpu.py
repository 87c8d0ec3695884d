"""The grid tail's reference and judge (tests/probe_tail_ref.py) on fabricated records: tail32 against tail64 and against
a hand-computed case, and the judge shown to pass a correct "device" and to reject each of five wrong ones.  Plus the mirror's surface:
the prototypes, the constants and the struct layout."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import path_ref as P
import probe_tail_ref as T
import probe_volume_ref as PV
import ray_shade_ref as R
from nebulae_amd import _lib
from nebulae_amd.renderer import ProbeTail

F, F64, U32 = np.float32, np.float64, np.uint32
N, K = 96, 3
SHADED = _lib.HIT_FOUND | _lib.HIT_ATTRIBUTES | _lib.HIT_MATERIAL


def fabricated(seed=3):
    """plain records of N paths with K - 1 = 2 segments: a third end at vertex 1 (miss, or a hit without material), the rest reach
    vertex 2, most of them on a surface with a material, a quarter of those from behind; and the surface records of vertex 2"""
    rng = np.random.default_rng(seed)
    out, vert, surf = np.zeros(N, P.PATH), np.zeros((N, K - 1), P.VERTEX), np.zeros(N, R.SURFACE)
    kind = rng.integers(0, 6, N)  # 0: miss at 1; 1: no material at 1; 2: miss at 2; 3..5: material at 2
    unit = lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)  # noqa: E731
    for k in range(K - 1):
        vert["origin"][:, k], vert["direction"][:, k] = rng.uniform(-1, 1, (N, 3)), unit(rng.standard_normal((N, 3)))
        vert["tmin"][:, k], vert["tmax"][:, k], vert["t"][:, k] = 0.001, 10000.0, rng.uniform(0.1, 3.0, N)
        vert["throughput"][:, k] = 1.0 if k == 0 else rng.uniform(0.05, 1.5, (N, 3))
        vert["rng"][:, k] = rng.integers(0, 2 ** 32, N)
        vert["added"][:, k] = rng.uniform(0.0, 4.0, (N, 3)) * (rng.random((N, 1)) < 0.6)
        vert["flags"][:, k] = SHADED
    vert["pdiff"][:, 0] = rng.uniform(0.1, 0.9, N)
    vert["flags"][kind == 0, 0], vert["flags"][kind == 1, 0], vert["flags"][kind == 2, 1] = 0, _lib.HIT_FOUND, 0
    ended = kind < 2
    vert[ended, 1] = np.zeros((), P.VERTEX)
    vert["pdiff"][ended, 0] = 0.0
    out["segments"] = np.where(ended, 1, 2)
    out["flags"] = vert["flags"][:, 0]
    out["t"], out["geometry"], out["primitive"] = vert["t"][:, 0], 1, 2
    out["radiance"] = P.running_sum(vert, out["segments"].astype(np.int64))
    surf["position"] = vert["origin"][:, 1] + vert["direction"][:, 1] * vert["t"][:, 1, None]
    sn = unit(rng.standard_normal((N, 3))) * rng.uniform(0.5, 2.0, (N, 1)).astype(F)
    facing = np.sum(sn * vert["direction"][:, 1], -1) <= 0
    flip = facing == (rng.random(N) < 0.25)  # a quarter of the normals end up facing away from the ray
    surf["shading_normal"] = np.where(flip[:, None], -sn, sn)
    surf["albedo"], surf["metalness"] = rng.uniform(0.0, 1.0, (N, 3)), rng.uniform(0.0, 1.0, N) * (rng.random(N) < 0.5)
    return (out, vert), surf


def gather(points):
    """a fabricated grid: E depends on the point's normal, so that a normal that is not turned shows; normals near +x find no probe"""
    out = np.zeros(len(points), PV.GATHER)
    n = points[:, 4:7] / np.maximum(np.linalg.norm(points[:, 4:7], axis=-1, keepdims=True), 1e-30)
    out["irradiance"] = (1.5 + n @ np.array([[0.9, 0.1, -0.4], [0.2, 1.1, 0.3], [-0.5, 0.4, 0.8]])).astype(F)
    none = n[:, 0] > 0.9
    out["irradiance"][none], out["flags"][none] = 0.0, _lib.GATHER_NO_PROBE
    out["weight"] = ~none
    return out


CORRUPTIONS = ("no 1 / pi", "Ng not turned toward the ray", "pd instead of 2 - pd", "a tail at vertex 1", "the tail left out of out.rgb")


def device(plain, surf, frame_weight, corrupt=None):
    """what a library that follows the contract -- or breaks it in one way -- would return for the fabricated paths"""
    (out, vert) = (plain[0].copy(), plain[1].copy())
    last = K - 1
    tp = vert[:, last - 1]
    pts = T.points(surf, tp["direction"])
    if corrupt == "Ng not turned toward the ray":
        pts[:, 4:7] = surf["shading_normal"]
    g = gather(pts)
    a = (out["segments"] == last) & ((tp["flags"] & _lib.HIT_MATERIAL) != 0) & ((g["flags"] & T.UNANSWERED) == 0)
    pd = np.random.default_rng(9).uniform(0.1, 0.9, N).astype(F) if frame_weight else None
    tail, added = T.tail32(tp[a], surf[a], g["irradiance"][a], None if pd is None else pd[a])
    if corrupt == "no 1 / pi":
        added = (tp["added"][a] + (tail / T.PI_INV).astype(F)).astype(F)
    if corrupt == "pd instead of 2 - pd":
        k = (tp["throughput"][a] * (surf["albedo"][a] * (F(1) - surf["metalness"][a])[:, None]).astype(F)).astype(F)
        added = (tp["added"][a] + (((k * pd[a][:, None]).astype(F) * g["irradiance"][a]).astype(F) * T.PI_INV).astype(F)).astype(F)
    vert["added"][a, last - 1] = added
    vert["flags"][a, last - 1] |= T.TAIL
    if frame_weight:
        vert["pdiff"][a, last - 1] = pd[a]
    out["flags"][a] |= T.TAIL
    if corrupt == "a tail at vertex 1":
        first = np.flatnonzero((vert["flags"][:, 0] & _lib.HIT_MATERIAL) != 0)[:5]
        vert["added"][first, 0] += F(0.25)
        vert["flags"][first, 0] |= T.TAIL
    out["radiance"] = P.running_sum(vert, out["segments"].astype(np.int64))
    if corrupt == "the tail left out of out.rgb":
        out["radiance"] = plain[0]["radiance"]
    return out, vert


def run_judge(plain, surf, got, frame_weight):
    return T.judge(plain, got, K, frame_weight, lambda rays: surf, gather, "fabricated")


@pytest.mark.parametrize("frame_weight", [False, True])
def test_the_judge_passes_a_device_that_follows_the_contract(frame_weight):
    plain, surf = fabricated()
    verdict = run_judge(plain, surf, device(plain, surf, frame_weight), frame_weight)
    assert 20 < verdict["flagged"] < verdict["candidates"] < N  # (paths that ended early, candidates, and candidates no probe answers)
    turned = np.sum(surf["shading_normal"] * plain[1]["direction"][:, 1], -1) > 0
    assert (turned & verdict["answered"]).sum() > 3  # (terminal hits from behind are among the flagged)


@pytest.mark.parametrize("corrupt", CORRUPTIONS)
def test_the_judge_rejects(corrupt):
    plain, surf = fabricated()
    frame_weight = corrupt == "pd instead of 2 - pd"
    with pytest.raises(AssertionError) as e:
        run_judge(plain, surf, device(plain, surf, frame_weight, corrupt), frame_weight)
    expected = {"a tail at vertex 1": "before the terminal vertex", "the tail left out of out.rgb": "running sum"}.get(corrupt, "added != tail32")
    assert expected in str(e.value), (corrupt, str(e.value)[:200])


def test_tail32_by_hand_and_against_float64():
    vertex, surface = np.zeros(1, P.VERTEX), np.zeros(1, R.SURFACE)
    vertex["throughput"], vertex["added"] = (0.5, 1.0, 2.0), (1.0, 0.0, 0.25)
    surface["albedo"], surface["metalness"] = (0.8, 0.4, 0.2), 0.5
    E = np.array([[2.0, 4.0, 8.0]], F)
    tail, added = T.tail32(vertex, surface, E)
    k = [F(0.5) * (F(0.8) * F(0.5)), F(1.0) * (F(0.4) * F(0.5)), F(2.0) * (F(0.2) * F(0.5))]
    want = np.array([F(F(k[c] * E[0, c]) * T.PI_INV) for c in range(3)], F)
    assert np.array_equal(tail[0].view(U32), want.view(U32)) and np.array_equal(added[0].view(U32), (vertex["added"][0] + want).astype(F).view(U32))
    assert abs(float(tail[0, 0]) - 0.5 * 0.4 * 2.0 / np.pi) < 1e-6
    # the frame weight: pd = 0.25 multiplies by 1.75, a pd that is not > 0 by 1
    weighted = T.tail32(vertex, surface, E, np.array([0.25], F))[0]
    assert np.allclose(weighted, tail * 1.75, rtol=3e-7) and np.array_equal(T.tail32(vertex, surface, E, np.array([0.0], F))[0], tail)
    # float32 against float64 on the fabricated records: three products, one sum
    plain, surf = fabricated()
    tp = plain[1][:, 1]
    Eall = gather(T.points(surf, tp["direction"]))["irradiance"]
    pd = np.linspace(0.1, 0.9, N).astype(F)
    t32, a32 = T.tail32(tp, surf, Eall, pd)
    t64, a64 = T.tail64(tp, surf, Eall, pd)
    assert (np.abs(t32 - t64) <= 6 * 2.0 ** -24 * np.abs(t64) + 1e-45).all() and (np.abs(a32 - a64) <= 8 * 2.0 ** -24 * np.maximum(np.abs(a64), np.abs(t64))).all()
    assert (t32 >= 0).all()


def test_turned_normal_faces_the_ray():
    SN = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0]], F)
    d = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [np.nan, 0, 0]], F)
    Ng = T.turned_normal(SN, d)
    assert np.array_equal(Ng[:3], [[0, 0, 1], [0, 0, -1], [0, 0, 1]]) and np.array_equal(Ng[3], [-1, 0, 0])  # (sd == 0 keeps SN; a NaN is not <= 0)


def test_the_mirror_declares_the_calls_the_constants_and_the_struct():
    header = (Path(__file__).resolve().parent.parent / "include" / "nebulae_hip.h").read_text()
    assert {"neb_gi_trace_paths_tail", "neb_gi_bake_probes_tail"} <= set(_lib.exported_symbols())
    for name, value in (("NEB_TAIL_FRAME_WEIGHT", _lib.TAIL_FRAME_WEIGHT), ("NEB_PATH_TAIL", _lib.PATH_TAIL)):
        assert int(re.search(rf"#define {name} (\d+)u", header).group(1)) == value
    assert _lib.PATH_TAIL == 256 and not _lib.PATH_TAIL & (63 | _lib.PATH_ESCAPED | _lib.PATH_DIVIDED)
    D = _lib.ProbeTailDesc
    assert C.sizeof(D) == 64 and D.grid.offset == 0 and D.records.offset == 40 and D.visibility.offset == 48 and D.normal_bias.offset == 56 and D.flags.offset == 60
    sigs = _lib._gi_sigs()
    plain, tail = sigs["neb_gi_trace_paths"][1], sigs["neb_gi_trace_paths_tail"][1]
    assert tail[:5] == plain[:5] and tail[6:] == plain[5:] and tail[5] is C.POINTER(D)
    plain, tail = sigs["neb_gi_bake_probes"][1], sigs["neb_gi_bake_probes_tail"][1]
    assert tail[:7] == plain[:7] and tail[8:] == plain[7:] and tail[7] is C.POINTER(D)
    t = ProbeTail(grid=None, records=None)
    assert t.visibility is None and t.normal_bias == 0.0 and t.frame_weight is True
