"""neb_gi_probe_grid / neb_gi_accumulate_probes / neb_gi_gather_probes on the device: the grid against
tests/probe_volume_ref.py bit for bit; the accumulation inside its derived bound, its special cases, and over real bakes; the gather
against the float64 reference on synthetic records (every wave shape, both arms of the kernel, the same bits whatever the order of the
points); bake -> accumulate -> gather on the room; ordering, the frame left alone, refusals and the Python mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

import path_ref as P
import probe_ref as B
import probe_volume_ref as PV
import ray_query_ref as Q
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from nebulae_amd.svgf import PLANE_RADIANCE, NebError
from test_probe_gpu import FREE_POINT, cases, enqueue_bake, records  # noqa: F401  (cases: the room fixture of the bake's tests)
from test_ray_query_gpu import H, W, on_device, same_bits
from test_ray_shade_gpu import state_renderer
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
FILL = float("nan")
NO_PROBE, CLAMPED, NOT_GATHERED = _lib.GATHER_NO_PROBE, _lib.GATHER_CLAMPED, _lib.GATHER_NOT_GATHERED
ODD_GRID = dict(origin=(0.1, -0.7, 3.3), spacing=(0.3, 0.7, 0.1))  # no power of two: a fused multiply-add would show


@pytest.fixture(scope="module")
def bare():
    """a renderer without a scene: none of the three calls needs one"""
    r = DeferredRenderer()
    r.init(W, H)
    yield r
    r.destroy()


def records_on_device(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(F).reshape(len(rec), 32)).cuda()


def enqueue_gather(r, g, d_rec, d_pts, stream=None):
    out = torch.full((d_pts.shape[0], 8), FILL, dtype=torch.float32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = r.gather_probes(PV.grid_struct(g), d_rec, d_pts, out=out, stream=None if stream is None else stream.cuda_stream)
    assert res["records"] is out
    return out


def gathered(out):
    return np.ascontiguousarray(out.cpu().numpy()).view(PV.GATHER).reshape(-1)


def gather(r, g, d_rec, pts):
    d = on_device(pts)
    torch.cuda.synchronize()
    out = enqueue_gather(r, g, d_rec, d)
    torch.cuda.synchronize()
    got = gathered(out)
    assert not got["reserved"].any()
    return got


def accumulate(r, a, b):
    da, db = records_on_device(a), records_on_device(b)
    torch.cuda.synchronize()
    assert r.accumulate_probes(da, db) is da
    torch.cuda.synchronize()
    assert same_bits(records(db), b)  # (`add` is read only)
    return records(da)


@pytest.fixture(scope="module")
def synthetic():
    """the inputs of tests/probe_volume_ref.py with their float64 references, computed once and left unchanged"""
    out = {}
    for dims in PV.DIMS:
        g = PV.gpu_grid(dims)
        rec = PV.random_records(g)
        sets = {(n, kind): PV.points(g, kind, n) for n in PV.COUNTS for kind in PV.KINDS}
        out[dims] = dict(grid=g, records=rec, points=sets, want={k: PV.gather64(g, rec, pts) for k, pts in sets.items()})
    return out


# ------------------------------------------------------------------------------------------------
# 1: the grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", PV.DIMS)
def test_probe_grid_is_the_reference_bit_for_bit(bare, dims):
    for g, tmin, tmax in ((PV.gpu_grid(dims), 0.0, np.inf), (PV.grid(ODD_GRID["origin"], ODD_GRID["spacing"], dims, 0.5), 1e-3, 7.5)):
        grid, probes = bare.probe_grid(g["origin"], g["spacing"], dims, tmin=tmin, tmax=tmax, backface_limit=float(g["backface_limit"]))
        torch.cuda.synchronize()
        assert isinstance(grid, _lib.ProbeGrid) and bytes(grid) == g.tobytes() and probes.shape == (PV.count(g), 8)
        assert same_bits(probes.cpu().numpy(), PV.grid_probes(g, tmin, tmax)), (dims, tmin)
    assert bytes(bare.probe_grid((0, 0, 0), 0.5, dims)[0]) == PV.grid((0, 0, 0), (0.5, 0.5, 0.5), dims, 0.25).tobytes()  # (one spacing for all)


def room_grid(sc, dims=(5, 4, 3)):
    """a grid over the inner 80 % of the room's box"""
    lo, hi = Q.scene_box(sc)
    c, h = 0.5 * (lo + hi), 0.4 * (hi - lo)
    return PV.grid(c - h, 2.0 * h / np.maximum(np.array(dims) - 1, 1), dims, 0.25)


def test_the_grid_from_the_device_bakes_as_the_same_tensor_built_on_the_host(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    g = room_grid(case["scene"])
    _, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    host = on_device(PV.grid_probes(g, tmin=1e-3))
    torch.cuda.synchronize()
    c = P.constants(3)
    a, b = enqueue_bake(r, d_probes, 64, "sh", c), enqueue_bake(r, host, 64, "sh", c)
    torch.cuda.synchronize()
    a, b = records(a), records(b)
    assert same_bits(a, b) and (a["samples"] == 64).all() and (a["hits"] > 0).all()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: the accumulation
# ------------------------------------------------------------------------------------------------
def test_accumulation_stays_inside_the_derived_bound(bare):
    worst = 0.0
    for n in (1, 3, 65):
        a, b = PV.random_bakes(n, 2, seed=n)
        worst = max(worst, PV.judge_accumulation(accumulate(bare, a, b), *PV.accumulate64(a, b), f"n = {n}"))
        lightmap = [x.copy() for x in (a, b)]
        for x in lightmap:
            x["sh"][:, 1:] = 0  # records of NEB_BAKE_IRRADIANCE: E and 24 zero words, which stay zero
        got = accumulate(bare, *lightmap)
        PV.judge_accumulation(got, *PV.accumulate64(*lightmap), f"irradiance records, n = {n}")
        assert not got["sh"][:, 1:].view(U32).any()
    print(f"[accumulate] largest error {worst:.3f} of the bound")
    assert worst > 0.0  # (the comparison is of blended words, not of copies)


def test_the_special_cases_leave_their_neighbours_alone(bare):
    n = 65
    a, b = PV.random_bakes(n, 2)
    plain = accumulate(bare, a, b)
    not_baked, empty, start, full, counter = 5, 6, 7, 8, 9
    a2, b2 = a.copy(), b.copy()
    b2[not_baked] = np.zeros(1, B.RECORD)
    b2["flags"][not_baked] = _lib.PROBE_NOT_BAKED
    b2[empty] = np.zeros(1, B.RECORD)
    a2[start] = np.zeros(1, B.RECORD)
    a2["flags"][start] = _lib.PROBE_NOT_BAKED  # (what a bake leaves of a probe it could not bake: the first good bake replaces it)
    a2["samples"][full] = 0xFFFFFFFF - 63
    a2["hits"][counter] = 0xFFFFFFFF - 3
    b2["flags"][counter] = _lib.PROBE_SATURATED
    got = accumulate(bare, a2, b2)
    want, value, bound = PV.accumulate64(a2, b2)
    PV.judge_accumulation(got, want, value, bound, "special cases")
    assert same_bits(got[not_baked:empty + 1], a2[not_baked:empty + 1])  # all bits kept
    assert same_bits(got[start:start + 1], b2[start:start + 1])  # all 32 words of `add`
    assert got["flags"][full] == _lib.PROBE_SATURATED and same_bits(got["sh"][full], a2["sh"][full]) and got["samples"][full] == a2["samples"][full]
    assert got["hits"][full] == a2["hits"][full] and got["segments"][full] == a2["segments"][full]
    assert got["hits"][counter] == 0xFFFFFFFF and got["flags"][counter] == _lib.PROBE_SATURATED  # the counter stops, the flag is or-ed in
    others = np.setdiff1d(np.arange(n), (not_baked, empty, start, full, counter))
    assert same_bits(got[others], plain[others])
    assert bare.accumulate_probes(records_on_device(a)[:0], records_on_device(b)[:0]).shape == (0, 32)


def test_four_real_bakes_stay_inside_the_bound_of_the_float64_mean_at_every_step(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    g = room_grid(case["scene"])
    _, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    n = PV.count(g)
    acc = torch.zeros((n, 32), dtype=torch.float32, device="cuda")
    ref = PV.Accumulator64(n)
    torch.cuda.synchronize()
    worst = 0.0
    for k in range(4):
        out = enqueue_bake(r, d_probes, 64, "sh", P.constants(3, frame_index=11 + k))
        r.accumulate_probes(acc, out)  # (straight behind the bake on the same stream)
        torch.cuda.synchronize()
        bake = records(out)
        assert (bake["samples"] == 64).all()
        ref.add(bake)
        got = records(acc)
        worst = max(worst, PV.judge_accumulation(got, ref.records, ref.value, ref.bound, f"step {k}"))
        assert (got["samples"] == 64 * (k + 1)).all()
    assert (got["hits"] > 64).any() and (got["segments"] > 4 * 64).any() and np.abs(ref.value).max() > 0.5
    print(f"[accumulate / room] largest error {worst:.3f} of the carried bound")
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3: the gather on synthetic records
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", PV.DIMS)
def test_gather_matches_the_float64_reference_on_every_wave_shape(bare, synthetic, dims):
    s = synthetic[dims]
    g, d_rec = s["grid"], records_on_device(s["records"])
    worst = 0.0
    for key, pts in s["points"].items():
        got = gather(bare, g, d_rec, pts)
        worst = max(worst, PV.judge_gather(PV.as_dict(got), s["want"][key], f"{dims} / {key}"))
    print(f"[gather / {dims}] largest error {worst:.3e} / {PV.TOL['gather']:.1e}")


@pytest.mark.parametrize("dims", PV.DIMS)
def test_both_arms_any_order_a_second_call_and_a_point_alone_give_the_same_bits(bare, synthetic, dims):
    s = synthetic[dims]
    g, d_rec = s["grid"], records_on_device(s["records"])
    one, scattered, stray = (s["points"][(4097, kind)] for kind in ("one cell", "all cells", "one stray lane"))
    a, b, c = gather(bare, g, d_rec, one), gather(bare, g, d_rec, scattered), gather(bare, g, d_rec, stray)
    assert same_bits(a, gather(bare, g, d_rec, one))  # a second call
    # `one` fills whole waves with one cell (the wave-uniform arm); in `stray` lane 17 of every wave lies in another cell, which sends the
    # other 63 lanes down the per-lane arm; mixed and permuted, every point meets other neighbours and, mostly, the other arm
    both = np.concatenate([one, scattered, stray])
    order = np.random.default_rng(8).permutation(len(both))
    mixed = gather(bare, g, d_rec, both[order])
    back = np.empty_like(mixed)
    back[order] = mixed
    assert same_bits(back, np.concatenate([a, b, c]))  # pixel-like order and a permutation: the same bits per point
    for i in (0, 17, 64, 4096):
        assert same_bits(gather(bare, g, d_rec, scattered[i:i + 1]), b[i:i + 1])  # a point alone
        assert same_bits(gather(bare, g, d_rec, stray[i:i + 1]), c[i:i + 1])


def test_unusable_points_say_so_and_leave_their_neighbours_alone(bare, synthetic):
    s = synthetic[(5, 4, 3)]
    g, d_rec = s["grid"], records_on_device(s["records"])
    blank = np.zeros(1, PV.GATHER)
    blank["flags"] = NOT_GATHERED
    spoils = {"nan position": lambda p: p.__setitem__(1, np.nan), "infinite position": lambda p: p.__setitem__(2, -np.inf),
              "position whose square overflows": lambda p: p.__setitem__(0, 2e19), "zero normal": lambda p: p.__setitem__(slice(4, 7), 0.0),
              "normal whose square underflows": lambda p: p.__setitem__(slice(4, 7), 1e-23), "nan normal": lambda p: p.__setitem__(5, np.nan),
              "infinite normal": lambda p: p.__setitem__(6, np.inf), "normal whose square overflows": lambda p: p.__setitem__(4, 3e19)}
    for kind in ("one cell", "all cells"):
        pts = PV.points(g, kind, 129)
        base = gather(bare, g, d_rec, pts)
        rows = np.array([0, 64, 128])  # first, middle (the first lane of a wave) and last
        others = np.setdiff1d(np.arange(129), rows)
        for name, spoil in spoils.items():
            bad = pts.copy()
            for i in rows:
                spoil(bad[i])
            assert not PV.usable(bad)[rows].any() and PV.usable(bad)[others].all(), name
            got = gather(bare, g, d_rec, bad)
            for i in rows:
                assert same_bits(got[i:i + 1], blank), (kind, name, i, got[i])
            assert same_bits(got[others], base[others]), (kind, name)
        alone = pts[:64].copy()
        for i in range(64):
            spoils["nan position"](alone[i])
        assert same_bits(gather(bare, g, d_rec, alone), np.repeat(blank, 64))  # a wave without a usable point


def test_no_valid_probe_gives_no_probe_and_nan_words_reach_nothing(bare, synthetic):
    s = synthetic[(5, 4, 3)]
    g = s["grid"]
    dead = s["records"].copy()
    dead["sh"] = np.nan
    dead["samples"][0::3] = 0
    dead["flags"][1::3] = _lib.PROBE_NOT_BAKED
    dead["backfaces"][2::3] = dead["samples"][2::3]
    d_dead = records_on_device(dead)
    for kind in PV.KINDS:
        got = gather(bare, g, d_dead, s["points"][(65, kind)])
        assert ((got["flags"] & NO_PROBE) != 0).all() and not (got["flags"] & NOT_GATHERED).any()
        assert not got["irradiance"].view(U32).any() and not got["weight"].view(U32).any() and not got["corners"].any()
        assert np.array_equal(got["cell"], s["want"][(65, kind)]["cell"]) and np.array_equal(got["flags"] & CLAMPED, s["want"][(65, kind)]["flags"] & CLAMPED)
    # the limit itself: backfaces == limit * samples is still valid, one more is not
    edge = PV.random_records(g, seed=3)
    edge["samples"], edge["flags"], edge["backfaces"] = 64, 0, 16
    edge["backfaces"][1::2] = 17
    edge["sh"] = np.random.default_rng(3).standard_normal((60, 9, 3)).astype(F)  # (every word finite: every probe may count now)
    pts = s["points"][(4097, "all cells")]
    PV.judge_gather(PV.as_dict(gather(bare, g, records_on_device(edge), pts)), PV.gather64(g, edge, pts), "at the backface limit")


def test_a_point_copied_from_a_probe_coincides_with_it(bare):
    """the rule "the same bits as neb_gi_probe_grid": on a grid that is no power of two a gather that formed the position in any other
    way would see a probe a few ulp away in an arbitrary direction, and w_n -- so the weight -- anywhere in 0.2 .. 1.2 instead of 0.45"""
    dims = (5, 4, 3)
    g = PV.grid(ODD_GRID["origin"], ODD_GRID["spacing"], dims, 0.25)
    _, d_probes = bare.probe_grid(g["origin"], g["spacing"], dims)
    rec = PV.random_records(g, seed=6)
    rec["samples"], rec["flags"], rec["backfaces"] = 64, 0, 0
    rec["sh"] = np.random.default_rng(6).standard_normal((60, 9, 3)).astype(F)
    pts = d_probes.clone()
    pts[:, 4:7] = on_device(np.random.default_rng(7).standard_normal((60, 3)))
    torch.cuda.synchronize()
    got = gathered(enqueue_gather(bare, g, records_on_device(rec), pts))
    torch.cuda.synchronize()
    # (float64 may put such a point an ulp to the other side of the probe's plane: another cell, the same blend but for weights of 1e-7)
    want = PV.gather64(g, rec, pts.cpu().numpy())
    assert np.abs(got["weight"].astype(np.float64) - 0.45).max() <= PV.TOL["gather"], got["weight"]
    for k in ("irradiance", "weight"):
        assert (np.abs(got[k].astype(np.float64) - want[k]) <= PV.TOL["gather"] * np.maximum(1.0, np.abs(want[k]))).all(), k
    assert not (got["flags"] & ~U32(CLAMPED)).any()  # (a probe on the box's faces may sit an ulp outside it)


# ------------------------------------------------------------------------------------------------
# 4: end to end on the room
# ------------------------------------------------------------------------------------------------
def interior_points(g, n, seed=12):
    rng = np.random.default_rng(seed)
    cells = np.maximum(np.array([int(d) for d in g["dims"]]) - 1, 1)
    t = np.floor(rng.uniform(0, 1, (n, 3)) * cells) + rng.uniform(0.01, 0.99, (n, 3))
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = (g["origin"].astype(np.float64) + t * g["spacing"].astype(np.float64)).astype(F)
    pts[:, 4:7] = rng.standard_normal((n, 3)) * rng.uniform(0.5, 3.0, (n, 1))
    return pts


def test_bake_accumulate_gather_on_the_room(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    g = room_grid(case["scene"])
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    torch.cuda.synchronize()
    acc = enqueue_bake(r, d_probes, 64, "sh", P.constants(3, frame_index=21))
    for k in (1, 2):
        r.accumulate_probes(acc, enqueue_bake(r, d_probes, 64, "sh", P.constants(3, frame_index=21 + k)))
    pts = interior_points(g, 300)
    d_pts = on_device(pts)
    res = r.gather_probes(grid, acc, d_pts)  # (behind the three bakes and the two accumulations, no host wait in between)
    torch.cuda.synchronize()
    rec = records(acc)
    assert (rec["samples"] == 192).all() and not rec["flags"].any()
    got = gathered(res["records"])
    worst = PV.judge_gather(PV.as_dict(got), PV.gather64(g, rec, pts), "room")
    lit = got["irradiance"].max(-1) > 0.05
    print(f"[room] largest error {worst:.3e} / {PV.TOL['gather']:.1e}; {int(lit.sum())} of 300 points lit; {int((got['corners'] != 255).sum())} with an ignored corner")
    assert lit.sum() > 150
    r.destroy()


def test_free_space_records_gather_to_pi_times_the_sky(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    h = 2.0 ** -14
    g = PV.grid(np.array(FREE_POINT) - 0.5 * h, (h, h, h), (2, 2, 2), 0.25)  # eight probes within 0.06 mm of a point with a free millimetre
    c = P.constants(5)
    sky = np.array(list(c.skyColor), np.float64)
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=0.0, tmax=9e-4)
    out = enqueue_bake(r, d_probes, 4096, "sh", c)
    pts = interior_points(g, 257)
    res = r.gather_probes(grid, out, on_device(pts))
    torch.cuda.synchronize()
    rec, got = records(out), gathered(res["records"])
    assert (rec["hits"] == 0).all() and (rec["samples"] == 4096).all() and sky.max() > 0
    assert (got["corners"] == 255).all() and not got["flags"].any()
    # The bar, from the downloaded words: the blend is a convex combination of the eight records, so band 0 is off from 4 pi Y00 sky by at
    # most what the worst record is, and every higher band -- Monte-Carlo noise around 0 -- is at most the worst record's word in size;
    # E adds them with |A_l Y_lm(N)|.  The clamp moves nothing away from a positive target.  The device's own rounding is TOL.
    sh = rec["sh"].astype(np.float64)
    k00 = float(B.K00)
    off = np.abs(sh - np.concatenate([(4.0 * np.pi * k00 * sky)[None], np.zeros((8, 3))])[None]).max(0)  # [9, 3]
    nrm = pts[:, 4:7].astype(np.float64)
    Y = np.abs(B.sh_basis64(nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)))  # [n, 9]
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    bar = (Y * A) @ off + PV.TOL["gather"] * np.maximum(1.0, np.pi * sky) + np.pi * sky * abs(4.0 * np.pi * k00 * k00 - 1.0)
    err = np.abs(got["irradiance"].astype(np.float64) - np.pi * sky)
    print(f"[sky] largest error {err.max():.3e}; its bar {bar[np.unravel_index(err.argmax(), err.shape)]:.3e}; noise words up to {off[1:].max():.3e}")
    assert (err <= bar).all() and bar.max() < np.pi * sky.max()  # (and the bar is one that a wrong answer would miss)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 5: ordering, the frame, refusals, the mirror
# ------------------------------------------------------------------------------------------------
def test_a_gather_behind_a_bake_on_one_stream_needs_no_host_wait(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    g = room_grid(case["scene"])
    _, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    d_pts = on_device(interior_points(g, 4097))
    c = P.constants(8)
    torch.cuda.synchronize()
    settled = enqueue_bake(r, d_probes, 256, "sh", c)
    torch.cuda.synchronize()
    want = gathered(enqueue_gather(r, g, settled, d_pts))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    out = enqueue_bake(r, d_probes, 256, "sh", c, stream=s)  # (its buffer is full of NaN until the bake has run)
    got = enqueue_gather(r, g, out, d_pts, stream=s)
    torch.cuda.synchronize()
    assert same_bits(gathered(got), want) and (want["irradiance"].max(-1) > 0.05).any()
    r.destroy()


def test_the_frame_its_counters_and_the_sun_table_are_untouched(cases):
    case = cases["room"]
    sc, cam = clone(case["scene"]), cornell_camera()
    r = _renderer(sc, cam, W, H, sun_table=1, hits=True)
    for f in (2, 3):
        frame(r, sc, cam, f)

    def snapshot():
        torch.cuda.synchronize()
        return r.ray_count(), r.traversal_stats(), r.sun_table_stats(), r.svgf.download(PLANE_RADIANCE).copy()
    count, trav, table, plane = snapshot()
    assert count > 0 and table["builds"] == 1 and plane[..., :3].max() > 0.05
    g = PV.gpu_grid((5, 4, 3))
    rec = PV.random_records(g)
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"])
    d_rec = records_on_device(rec)
    r.accumulate_probes(d_rec, records_on_device(PV.random_bakes(60, 1)[0]))
    res = r.gather_probes(grid, d_rec, on_device(PV.points(g, "all cells", 4097)))
    torch.cuda.synchronize()
    assert same_bits(d_probes.cpu().numpy(), PV.grid_probes(g)) and bool((res["weight"] > 0).any())
    count2, trav2, table2, plane2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(plane2, plane)
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05
    r.destroy()


def test_refusals_enqueue_nothing_and_name_the_cause(bare):
    r = bare
    lib, ctx = r._lib, r._ctx
    g = PV.gpu_grid((5, 4, 3))
    n, m = 65, 60
    rec = PV.random_records(g)
    want_grid = PV.grid_probes(g, 0.0, 2.0)
    pts = PV.points(g, "all cells", n)
    want = PV.gather64(g, rec, pts)
    d_rec, d_add, d_pts = records_on_device(rec), records_on_device(PV.random_bakes(m, 1)[0]), on_device(pts)
    probes = torch.full((m + 1, 8), FILL, dtype=torch.float32, device="cuda")
    acc = torch.full((m + 1, 32), FILL, dtype=torch.float32, device="cuda")
    out = torch.full((n + 1, 8), FILL, dtype=torch.float32, device="cuda")
    host_mem = torch.empty((m * 32 + 16,), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    ok = PV.grid_struct(g)

    def spoiled(**k):
        s = PV.grid_struct(g)
        for name, (index, value) in k.items():
            if index is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[index] = value
        return s

    bad_grids = [("dims of 0", spoiled(dims=(1, 0)), b"dims"), ("negative spacing", spoiled(spacing=(0, -0.5)), b"spacing"),
                 ("zero spacing", spoiled(spacing=(2, 0.0)), b"spacing"), ("nan spacing", spoiled(spacing=(1, float("nan"))), b"spacing"),
                 ("infinite spacing", spoiled(spacing=(0, float("inf"))), b"spacing"), ("nan origin", spoiled(origin=(2, float("nan"))), b"origin"),
                 ("too many probes", _lib.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_uint32 * 3)(4096, 4096, 2), 0.25), b"2^24"),
                 ("too many probes on one axis", spoiled(dims=(2, (1 << 24) + 1)), b"2^24"),
                 ("dims whose product wraps", _lib.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_uint32 * 3)(1 << 16, 1 << 16, 1 << 16), 0.25), b"2^24"),
                 ("negative backface_limit", spoiled(backface_limit=(None, -0.01)), b"backface_limit"),
                 ("backface_limit above 1", spoiled(backface_limit=(None, 1.5)), b"backface_limit"),
                 ("nan backface_limit", spoiled(backface_limit=(None, float("nan"))), b"backface_limit")]

    def call_grid(grid, p_probes):
        return lib.neb_gi_probe_grid(ctx, None if grid is None else C.byref(grid), 0.0, 2.0, C.c_void_p(p_probes), None)

    def call_acc(p_acc, p_add, count):
        return lib.neb_gi_accumulate_probes(ctx, C.c_void_p(p_acc), C.c_void_p(p_add), count, None)

    def call_gather(grid, p_rec, p_pts, count, p_out):
        return lib.neb_gi_gather_probes(ctx, None if grid is None else C.byref(grid), C.c_void_p(p_rec), C.c_void_p(p_pts), count, C.c_void_p(p_out), None)

    def error():
        return lib.neb_last_error(ctx)

    PR, AC, AD, RE, PT, OU = probes.data_ptr(), acc.data_ptr(), d_add.data_ptr(), d_rec.data_ptr(), d_pts.data_ptr(), out.data_ptr()
    refused_grid = [(what, (grid, PR), word) for what, grid, word in bad_grids] + [
        ("null grid", (None, PR), b"null grid"), ("null probes", (ok, 0), b"null"), ("misaligned probes", (ok, PR + 8), b"misaligned"),
        ("host-memory probes", (ok, host_ptr), b"probes is not memory"),
        ("probes one short of their allocation", (ok, end - 32 * (m - 1)), b"probes is not memory")]
    refused_acc = [("null acc", (0, AD, m), b"null"), ("null add", (AC, 0, m), b"null"), ("misaligned acc", (AC + 16, AD, m - 1), b"misaligned"),
                   ("misaligned add", (AC, AD + 16, m - 1), b"misaligned"), ("add is acc", (AC, AC, m), b"overlaps"),
                   ("add overlapping acc", (AC, AC + 128, 2), b"overlaps"), ("host-memory acc", (host_ptr, AD, m), b"acc is not memory"),
                   ("host-memory add", (AC, host_ptr, m), b"add is not memory"),
                   ("acc one short of its allocation", (end - 128 * (m - 1), AD, m), b"acc is not memory"),
                   ("add one short of its allocation", (AC, end - 128 * (m - 1), m), b"add is not memory")]
    refused_gather = [(what, (grid, RE, PT, n, OU), word) for what, grid, word in bad_grids] + [
        ("null grid", (None, RE, PT, n, OU), b"null grid"), ("null records", (ok, 0, PT, n, OU), b"null"), ("null points", (ok, RE, 0, n, OU), b"null"),
        ("null out", (ok, RE, PT, n, 0), b"null"), ("misaligned records", (ok, RE + 16, PT, n, OU), b"misaligned"),
        ("misaligned points", (ok, RE, PT + 8, n - 1, OU), b"misaligned"), ("misaligned out", (ok, RE, PT, n, OU + 16), b"misaligned"),
        ("out is points", (ok, RE, OU, n, OU), b"overlaps points"), ("out overlapping points", (ok, RE, OU + 32, 2, OU), b"overlaps points"),
        ("out inside records", (ok, AC, PT, n, AC + 128), b"overlaps records"),
        ("host-memory records", (ok, host_ptr, PT, n, OU), b"records is not memory"), ("host-memory points", (ok, RE, host_ptr, n, OU), b"points is not memory"),
        ("host-memory out", (ok, RE, PT, n, host_ptr), b"out is not memory"),
        ("records one short of their allocation", (ok, end - 128 * (m - 1), PT, n, OU), b"records is not memory"),
        ("points one short of their allocation", (ok, RE, end - 32 * (n - 1), n, OU), b"points is not memory"),
        ("out one short of its allocation", (ok, RE, PT, n, end - 32 * (n - 1)), b"out is not memory")]
    torch.cuda.synchronize()
    for name, call, cases_ in (("neb_gi_probe_grid", call_grid, refused_grid), ("neb_gi_accumulate_probes", call_acc, refused_acc),
                               ("neb_gi_gather_probes", call_gather, refused_gather)):
        for what, args, word in cases_:
            assert call(*args) == -1, (name, what, error())
            assert name.encode() in error() and word in error(), (name, what, error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(probes).all()) and bool(torch.isnan(acc).all()) and bool(torch.isnan(out).all()), "a refused call wrote something"
    # n == 0: a no-op that succeeds and looks at no pointer
    assert call_acc(0, 0, 0) == 0 and call_gather(ok, 0, 0, 0, 0) == 0
    # ... and the same context answers: the ranges that just fit their allocation are accepted
    block[-128 * m:].view(torch.float32).view(m, 32).copy_(d_rec)
    assert call_grid(ok, end - 128 * m - 32 * m) == 0
    assert call_gather(ok, end - 128 * m, PT, n, end - 128 * m - 32 * m - 32 * n) == 0
    assert call_acc(end - 128 * m, AD, m) == 0
    acc[:m].zero_()
    assert call_grid(ok, PR) == 0 and call_gather(ok, RE, PT, n, OU) == 0 and call_acc(AC, AD, m) == 0
    torch.cuda.synchronize()
    assert same_bits(probes[:m].cpu().numpy(), want_grid) and bool(torch.isnan(probes[m]).all())
    PV.judge_gather(PV.as_dict(gathered(out[:n])), want, "after the refusals")
    assert bool(torch.isnan(out[n]).all())
    assert same_bits(acc[:m].cpu().numpy(), d_add.cpu().numpy()) and bool(torch.isnan(acc[m]).all())
    tail = block[-(128 * m + 32 * m + 32 * n):]
    assert same_bits(tail[32 * n:32 * n + 32 * m].cpu().numpy().view(F).reshape(m, 8), want_grid)
    assert same_bits(tail[:32 * n].cpu().numpy().view(PV.GATHER), gathered(out[:n]))


def test_the_python_mirror_checks_its_arguments_and_returns_the_views(bare):
    r = bare
    g = PV.gpu_grid((5, 4, 3))
    grid, probes = r.probe_grid(g["origin"], g["spacing"], g["dims"])
    rec = records_on_device(PV.random_records(g))
    pts = on_device(PV.points(g, "all cells", 10))
    for bad in (dict(dims=(5, 4)), dict(dims=(5, 0, 3)), dict(dims=(4096, 4096, 2)), dict(spacing=(0.5, 0.5)), dict(spacing=0.0), dict(spacing=(1, -1, 1)),
                dict(origin=(0, 0)), dict(origin=(0, np.nan, 0)), dict(backface_limit=1.5), dict(out=torch.empty((60, 8))),
                dict(out=torch.empty((59, 8), device="cuda"))):
        with pytest.raises(NebError):
            r.probe_grid(**{**dict(origin=(0, 0, 0), spacing=1.0, dims=(5, 4, 3)), **bad})
    for a, b in ((rec.cpu(), rec), (rec, rec[:59]), (rec[:, :31], rec[:, :31]), (rec.double(), rec.double()), (rec[::2], rec[::2])):
        with pytest.raises(NebError):
            r.accumulate_probes(a, b)
    for args in ((g, rec, pts), (grid, rec[:59], pts), (grid, rec.cpu(), pts), (grid, rec, pts.cpu()), (grid, rec, pts[:, :7]), (grid, rec, pts.double()),
                 (grid, rec, pts[::2])):
        with pytest.raises(NebError):
            r.gather_probes(*args)
    for out in (torch.empty((10, 8)), torch.empty((9, 8), device="cuda")):
        with pytest.raises(NebError):
            r.gather_probes(grid, rec, pts, out=out)
    res = r.gather_probes(grid, rec, pts)
    views = ("irradiance", "weight", "corners", "cell", "flags")
    assert set(res) == set(views) | {"records"} and res["records"].shape == (10, 8) and res["irradiance"].shape == (10, 3)
    assert [res[k].data_ptr() - res["records"].data_ptr() for k in views] == [PV.GATHER.fields[k][1] for k in views]
    assert all(res[k].dtype == torch.int32 for k in views[2:]) and res["weight"].dtype == torch.float32
    assert r.gather_probes(grid, rec, pts[:0])["records"].shape == (0, 8)
    torch.cuda.synchronize()
    assert bool((res["weight"] > 0).any())
