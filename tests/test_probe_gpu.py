"""neb_gi_probe_rays / neb_gi_bake_probes on the device: the rays against the float64 formulas of tests/probe_ref.py;
the baked records against probe_ref.bake_ref of the device's own trace_paths over the device's own probe_rays, BIT FOR BIT; against the
float64 projection of those paths within the derived bound; closed forms; counters; probes that are not baked; across updates and
streams; beside a frame they must not disturb; and at their refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import path_ref as P
import probe_ref as B
import ray_query_ref as Q
import ray_shade_ref as R
import views_ref as V
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from nebulae_amd.svgf import PLANE_RADIANCE, NebError
from test_path_gpu import to_host as paths_to_host
from test_ray_query_gpu import H, W, on_device, same_bits
from test_ray_shade_gpu import renderer, state_renderer
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
FILL = float("nan")
MODES = tuple(B.WHAT)
TALL_BOX_CENTRE = (0.4, -0.4, -1.6)  # inside submesh 2 of the room; its nearest walls are 0.3 away, the rug below it 0.58
FREE_POINT = (0.2, 0.0, -0.6)        # nothing of the room within a millimetre


# ------------------------------------------------------------------------------------------------
def probe_set(sc, n, seed=5):
    """n probes in the inner 90 % of the scene's box, some inside its boxes, with normals of every kind and a first interval that
    starts a millimetre out"""
    lo, hi = Q.scene_box(sc)
    rng = np.random.default_rng(seed)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pr = B.probes(c + 0.9 * h * rng.uniform(-1.0, 1.0, (n, 3)), tmin=1e-3)
    nrm = rng.standard_normal((n, 3))
    nrm[0::5] = (0.0, 0.0, 1.0)
    nrm[1::5] = (0.0, 1.0, 0.0)
    nrm[2::5] = (0.1, 0.2, -1.0)
    pr[:, 4:7] = nrm * rng.uniform(0.5, 3.0, (n, 1))
    return pr


def device_rays(r, d_probes, S, what, frame_index, stream=None):
    out = torch.full((d_probes.shape[0] * S, 8), FILL, dtype=torch.float32, device="cuda")
    res = r.probe_rays(d_probes, S, what, frame_index=frame_index, out=out, stream=stream)
    assert res is out
    return out


def enqueue_bake(r, d_probes, S, what, c, stream=None):
    """one call into a buffer filled with a pattern no record has -> the output tensor (nothing waits)"""
    out = torch.full((d_probes.shape[0], 32), FILL, dtype=torch.float32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = r.bake_probes(d_probes, S, what, constants=c, out=out, stream=None if stream is None else stream.cuda_stream)
    assert res["records"] is out
    return out


def records(out):
    return np.ascontiguousarray(out.cpu().numpy()).view(B.RECORD).reshape(-1)


def bake(r, pr, S, what, c):
    d = on_device(pr)
    torch.cuda.synchronize()
    out = enqueue_bake(r, d, S, what, c)
    torch.cuda.synchronize()
    return records(out)


def old_route(r, pr, S, what, c):
    """probe_rays, trace_paths, all on the device -> (neb_ray_path [n * S], rays float32 [n * S, 8]) on the host"""
    d = on_device(pr)
    torch.cuda.synchronize()
    rays = device_rays(r, d, S, what, int(c.frameIndex))
    res = r.trace_paths(rays, constants=c)
    torch.cuda.synchronize()
    return paths_to_host((res["records"], None))[0], rays.cpu().numpy()


def check(r, pr, S, what, c, name):
    """the central comparison -> (the device's records, the paths they reduce)"""
    got = bake(r, pr, S, what, c)
    paths, rays = old_route(r, pr, S, what, c)
    want = B.bake_ref(paths, rays, S, what)
    if not same_bits(got, want):
        bad = np.flatnonzero((got.view(U32).reshape(len(got), 32) != want.view(U32).reshape(len(got), 32)).any(-1))
        raise AssertionError(f"{name}: {len(bad)} of {len(got)} records differ from reduce(trace_paths(probe_rays)); first: probe {bad[0]}\n"
                             f"{got[bad[0]]}\n{want[bad[0]]}")
    ratio = B.inside_bound(got, *B.project64(paths, rays, S, what))
    assert ratio <= 1.0, f"{name}: a word is {ratio:.2f} bounds away from the float64 projection"
    return got, paths


@pytest.fixture(scope="module")
def cases():
    return {name: dict(scene=sc, hidden=hidden) for name, (sc, hidden) in R.states().items()}


# ------------------------------------------------------------------------------------------------
# 1: the rays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", MODES)
def test_rays_follow_the_formulas_and_are_the_probes_own_bits(cases, what):
    r = DeferredRenderer()
    r.init(W, H)  # (no scene: the call needs none)
    sc = cases["room, extras"]["scene"]
    worst = 0.0
    for n in (1, 3, 65):
        for S in (64, 192):
            pr = probe_set(sc, n)
            d = on_device(pr)
            torch.cuda.synchronize()
            a, b, other = device_rays(r, d, S, what, 3), device_rays(r, d, S, what, 3), device_rays(r, d, S, what, 4)
            torch.cuda.synchronize()
            a, b, other = a.cpu().numpy(), b.cpu().numpy(), other.cpu().numpy()
            worst = max(worst, B.judge_rays(pr, S, what, 3, a, f"{what} / {n} x {S}"))
            assert same_bits(a, b)
            assert same_bits(a[:, [0, 1, 2, 3, 7]], other[:, [0, 1, 2, 3, 7]]) and (a[:, 4:7] != other[:, 4:7]).any(-1).mean() > 0.99
    print(f"[rays / {what}] largest direction error {worst:.3e} / {B.TOL['direction']:.1e}")
    assert r.info is None and torch.equal(r.probe_rays(d, 64, what).view(torch.int32), r.probe_rays(d, 64, what, frame_index=0).view(torch.int32))  # (no frame: 0)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: bake == reduce(trace_paths(probe_rays)), bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("what", MODES)
def test_bake_is_the_reduction_of_trace_paths_over_probe_rays_bit_for_bit(cases, what, exact):
    case = cases["room, extras"]
    r = state_renderer(case, bool(exact))
    lit = 0
    for n in (1, 3, 65):
        pr = probe_set(case["scene"], n)
        for S in (64, 128, 192):
            for K in (2, 3, 8):
                got, paths = check(r, pr, S, what, P.constants(K), f"{what} / exact {exact} / {n} x {S} / K {K}")
                assert (got["samples"] == S).all() and not got["flags"].any()
                lit += int((got["sh"][:, 0].max(-1) > 0).sum())
    assert lit > 9 * 60  # (the comparison is of lit records, not of zeroes)
    r.destroy()


@pytest.mark.parametrize("what", MODES)
@pytest.mark.parametrize("state", list(R.states()))
def test_every_scene_state_bakes_the_same_bits(cases, state, what):
    case = cases[state]
    r = state_renderer(case, exact=False)
    got, paths = check(r, probe_set(case["scene"], 65), 128, what, P.constants(3), f"{state} / {what}")
    assert (got["hits"] > 0).all()
    if case["hidden"]:
        assert not np.isin(paths["geometry"], list(case["hidden"])).any()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3: determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", MODES)
def test_a_second_call_and_a_probe_baked_alone_give_the_same_bits(cases, what):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    pr, c = probe_set(case["scene"], 65), P.constants(5)
    a, b = bake(r, pr, 192, what, c), bake(r, pr, 192, what, c)
    assert same_bits(a, b)
    alone = bake(r, pr[:1], 192, what, c)  # (probe 0: a sample's index i depends on the probe's place in the call)
    assert same_bits(alone, a[:1])
    shuffled = pr.copy()
    shuffled[1:] = pr[:0:-1]
    assert same_bits(bake(r, shuffled, 192, what, c)[:1], a[:1])
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 4, 5: physics and closed forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", MODES)
def test_records_are_inside_the_bound_of_the_float64_projection(cases, what):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    pr, S = probe_set(case["scene"], 65), 192
    got = bake(r, pr, S, what, P.constants(8))
    paths, rays = old_route(r, pr, S, what, P.constants(8))
    value, bound = B.project64(paths, rays, S, what)
    ratio = B.inside_bound(got, value, bound)
    print(f"[physics / {what}] largest error {ratio:.3f} of the bound; largest word {float(np.abs(value).max()):.3f}")
    assert ratio <= 1.0 and np.abs(value).max() > 1.0
    r.destroy()


def test_free_space_gives_the_sky_in_closed_form_and_no_light_gives_zero(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    S = 256
    pr = B.probes([FREE_POINT, FREE_POINT], normal=[(0.0, 1.0, 0.0), (0.3, -0.2, 0.9)], tmin=0.0, tmax=1e-3)
    c = P.constants(5)
    sky = np.array(list(c.skyColor), np.float64)
    assert sky.max() > 0
    for what, factor in (("sh", 4.0 * np.pi * float(B.K00)), ("irradiance", np.pi)):
        got = bake(r, pr, S, what, c)
        paths, rays = old_route(r, pr, S, what, c)
        _, bound = B.project64(paths, rays, S, what)
        assert (got["hits"] == 0).all() and (got["backfaces"] == 0).all() and (got["segments"] == S).all() and (got["samples"] == S).all()
        err = np.abs(got["sh"][:, 0].astype(np.float64) - factor * sky)
        # (the bound is around the float scale; the scale's own rounding, 2^-24 relative, is added)
        assert (err <= bound[:, 0:3] + 2.0 ** -24 * factor * sky).all(), (what, err, bound[:, 0:3])
    dark = P.constants(5)
    dark.sunLightRadiance[:] = (0.0, 0.0, 0.0)
    dark.skyColor[:] = (0.0, 0.0, 0.0)
    inside = probe_set(case["scene"], 65)
    for what in MODES:
        got = bake(r, inside, 64, what, dark)
        assert not got["sh"].view(U32).any() and (got["hits"] > 0).all() and (got["samples"] == 64).all()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 6: counters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", MODES)
def test_counters_are_the_sums_over_the_path_records(cases, what):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    S, c = 128, P.constants(4)
    pr = probe_set(case["scene"], 65)
    pr[7] = B.probes([TALL_BOX_CENTRE], normal=(1.0, 0.0, 0.0), tmin=0.0, tmax=0.5)[0]  # inside the tall box, short of the rug below it
    got = bake(r, pr, S, what, c)
    paths, _ = old_route(r, pr, S, what, c)
    flags = paths["flags"].reshape(65, S)
    found = (flags & _lib.HIT_FOUND) != 0
    assert np.array_equal(got["hits"], found.sum(-1))
    assert np.array_equal(got["backfaces"], (found & ((flags & _lib.HIT_BACKFACE) != 0)).sum(-1))
    assert np.array_equal(got["segments"], paths["segments"].reshape(65, S).sum(-1))
    assert got["backfaces"][7] == got["hits"][7] > 0, (got["hits"][7], got["backfaces"][7])
    assert set(np.unique(paths["geometry"].reshape(65, S)[7][found[7]]).tolist()) == {2}
    assert (got["segments"] > S).any() and (got["hits"] < S).any()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 7: probes that are not baked
# ------------------------------------------------------------------------------------------------
ANY_MODE = {"nan position": lambda p: p.__setitem__(1, np.nan), "infinite position": lambda p: p.__setitem__(2, np.inf),
            "position whose square overflows": lambda p: p.__setitem__(0, -2e19), "tmin < 0": lambda p: p.__setitem__(3, -1e-3),
            "tmax == tmin": lambda p: p.__setitem__(slice(3, 8, 4), 0.25), "tmax < tmin": lambda p: p.__setitem__(7, 0.0),
            "nan tmin": lambda p: p.__setitem__(3, np.nan), "nan tmax": lambda p: p.__setitem__(7, np.nan)}
NORMAL_ONLY = {"zero normal": lambda p: p.__setitem__(slice(4, 7), 0.0), "normal whose square underflows": lambda p: p.__setitem__(slice(4, 7), 1e-23),
               "nan normal": lambda p: p.__setitem__(5, np.nan), "infinite normal": lambda p: p.__setitem__(6, -np.inf),
               "normal whose square overflows": lambda p: p.__setitem__(4, 3e19)}


@pytest.mark.parametrize("what", MODES)
def test_probes_that_cannot_be_baked_say_so_and_leave_their_neighbours_alone(cases, what):
    """every kind in both modes: the position and interval kinds are refused in both, the normal kinds under "irradiance" alone -- under
    "sh" such a probe is baked, and its record is the one it has with a good normal"""
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    S, c = 64, P.constants(3)
    good = probe_set(case["scene"], 65)
    rows = np.array([0, 31, 64])
    others = np.setdiff1d(np.arange(65), rows)
    blank = np.zeros(1, B.RECORD)
    blank["flags"] = _lib.PROBE_NOT_BAKED
    base = bake(r, good, S, what, c)
    for kind, spoil in {**ANY_MODE, **NORMAL_ONLY}.items():
        bad = good.copy()
        for i in rows:
            spoil(bad[i])
        refused = kind in ANY_MODE or what == "irradiance"
        assert B.baked(bad, what)[rows].any() != refused and B.baked(bad, what)[others].all(), kind
        got = bake(r, bad, S, what, c)
        if refused:
            for i in rows:
                assert same_bits(got[i:i + 1], blank), (kind, i, got[i])
            assert same_bits(got[others], base[others]), kind
        else:
            assert same_bits(got, base), kind
        paths, rays = old_route(r, bad, S, what, c)
        if refused:
            assert not rays.reshape(65, S * 8)[rows].view(U32).any() and (paths["flags"].reshape(65, S)[rows] == _lib.HIT_NOT_WALKED).all(), kind
        assert same_bits(got, B.bake_ref(paths, rays, S, what)), kind
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 8: the scene as the updates have left it
# ------------------------------------------------------------------------------------------------
def test_a_hidden_submesh_is_absent_from_every_sample(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    S, c = 128, P.constants(3)
    pr = probe_set(case["scene"], 65)
    for what in MODES:
        before, paths0 = check(r, pr, S, what, c, f"visible / {what}")
        assert (paths0["geometry"] == V.POST).any()
        d = on_device(pr)
        torch.cuda.synchronize()
        r.set_visible([V.POST], False)
        out = enqueue_bake(r, d, S, what, c)  # (enqueued straight behind the update)
        torch.cuda.synchronize()
        behind = records(out)
        after, paths1 = check(r, pr, S, what, c, f"hidden / {what}")
        assert same_bits(behind, after) and not same_bits(after, before) and not (paths1["geometry"] == V.POST).any()
        r.set_visible([V.POST], True)
    r.destroy()


def test_a_bake_runs_behind_an_update_on_another_stream_and_a_later_update_waits_for_it():
    sc0, updates = V.room_updates()
    _, _, (indices, moved), s1 = updates[0]  # the boxes rotated
    orig = np.stack([sc0.geometries[i]["M"] for i in indices])
    pr = probe_set(sc0, 1024)  # (a bake long enough for an update to overtake, if it could)
    S, c = 128, P.constants(8)
    r = renderer(clone(sc0), exact=False)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    d = on_device(pr)
    for what in MODES:
        still = records(enqueue_bake(r, d, S, what, c))  # the scene before the move
        torch.cuda.synchronize()
        r.update_transforms(indices, moved, stream=a.cuda_stream)
        out1 = enqueue_bake(r, d, S, what, c, stream=b)  # no host synchronisation in between
        torch.cuda.synchronize()
        h1 = records(out1)
        settled = records(enqueue_bake(r, d, S, what, c))
        torch.cuda.synchronize()
        # the opposite order: the bake on b, then an update on a that moves the boxes back
        out2 = enqueue_bake(r, d, S, what, c, stream=b)
        r.update_transforms(indices, orig, stream=a.cuda_stream)
        torch.cuda.synchronize()
        h2 = records(out2)
        back = records(enqueue_bake(r, d, S, what, c))
        torch.cuda.synchronize()
        assert same_bits(h1, settled) and same_bits(h1, h2) and same_bits(back, still) and not same_bits(still, h1), what
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 9: the frame is untouched
# ------------------------------------------------------------------------------------------------
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
    other_sun = P.constants(8, frame_index=9)
    other_sun.sunLightDirection[:] = (-0.3, -1.0, 0.4)  # (a sun the table was not built for: the call must not make it chase)
    pr = probe_set(sc, 65)
    for what in MODES:
        for c in (P.constants(8), other_sun, P.constants(2)):
            got = bake(r, pr, 128, what, c)
            assert (got["hits"] > 0).all()
            torch.cuda.synchronize()
            device_rays(r, on_device(pr), 128, what, 9)
    count2, trav2, table2, plane2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(plane2, plane)
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05  # the table still serves its own sun
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 10: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_name_the_cause(cases):
    case = cases["room"]
    n, S = 65, 64
    pr = probe_set(case["scene"], n)
    d = on_device(pr)
    r = DeferredRenderer()
    r.init(W, H)
    lib, ctx = r._lib, r._ctx
    out = torch.full((n + 1, 32), FILL, dtype=torch.float32, device="cuda")
    rays = torch.full((n * S + 1, 8), FILL, dtype=torch.float32, device="cuda")
    k3, k1, k9 = P.constants(3), P.constants(3), P.constants(3)
    k1.maxPathVertices, k9.maxPathVertices = 1, 9
    cp = C.byref(k3)
    SH, IRR = _lib.BAKE_SH, _lib.BAKE_IRRADIANCE

    def call_bake(p_probes, count, samples, what, flags, c, p_out):
        return lib.neb_gi_bake_probes(ctx, C.c_void_p(p_probes), count, samples, what, flags, c, C.c_void_p(p_out), None)

    def call_rays(p_probes, count, samples, what, frame_index, p_rays):
        return lib.neb_gi_probe_rays(ctx, C.c_void_p(p_probes), count, samples, what, frame_index, C.c_void_p(p_rays), None)

    def error():
        return lib.neb_last_error(ctx)

    D, O, RY = d.data_ptr(), out.data_ptr(), rays.data_ptr()
    assert call_bake(D, n, S, SH, 0, cp, O) == -4 and b"neb_gi_bake_probes" in error()  # no scene
    assert call_rays(D, n, S, SH, 3, RY) == 0  # ... which the rays do not need
    torch.cuda.synchronize()
    B.judge_rays(pr, S, "sh", 3, rays[:n * S].cpu().numpy(), "without a scene")
    assert bool(torch.isnan(rays[n * S]).all())
    rays.fill_(FILL)
    sc = clone(case["scene"])
    G, ng, M, nm, T, nt = sc.descs()
    assert lib.neb_gi_set_scene(ctx, G, ng, M, nm, T, nt) == 0
    assert call_bake(D, n, S, SH, 0, cp, O) == -4 and b"not ready" in error()  # a scene, no tree
    assert lib.neb_gi_build_bvh(ctx, None) == 0
    host_mem = torch.empty((n * S + 2, 8), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    refused_bake = [("samples not a multiple of 64", (D, n, 96, SH, 0, cp, O), -1, b"samples"),
                    ("no samples", (D, n, 0, IRR, 0, cp, O), -1, b"samples"),
                    ("too many samples", (D, n, 4160, SH, 0, cp, O), -1, b"samples"),
                    ("too many rays", (D, (1 << 22) + 1, 64, SH, 0, cp, O), -5, b"2^28"),
                    ("too many rays, large S", (D, (1 << 16) + 1, 4096, IRR, 0, cp, O), -5, b"2^28"),
                    ("unknown what", (D, n, S, 2, 0, cp, O), -1, b"what"),
                    ("unknown flag", (D, n, S, SH, 4, cp, O), -1, b"flag"),
                    ("any hit", (D, n, S, SH, _lib.RAYS_ANY_HIT, cp, O), -1, b"flag"),
                    ("sorted", (D, n, S, IRR, _lib.RAYS_SORT, cp, O), -1, b"NEB_RAYS_SORT"),
                    ("one path vertex", (D, n, S, SH, 0, C.byref(k1), O), -1, b"maxPathVertices"),
                    ("nine path vertices", (D, n, S, IRR, 0, C.byref(k9), O), -1, b"maxPathVertices"),
                    ("null constants", (D, n, S, SH, 0, None, O), -1, b"constants"),
                    ("null probes", (0, n, S, SH, 0, cp, O), -1, b"null"),
                    ("null out", (D, n, S, IRR, 0, cp, 0), -1, b"null"),
                    ("misaligned probes", (D + 8, n - 1, S, SH, 0, cp, O), -1, b"misaligned"),
                    ("misaligned out", (D, n, S, SH, 0, cp, O + 16), -1, b"misaligned"),
                    ("out overlapping probes", (D, n, S, SH, 0, cp, D + 32 * (n - 1)), -1, b"overlaps"),
                    ("out is probes", (D, n, S, IRR, 0, cp, D), -1, b"overlaps"),
                    ("host-memory probes", (host_ptr, n, S, SH, 0, cp, O), -1, b"probes is not memory"),
                    ("host-memory out", (D, n, S, SH, 0, cp, host_ptr), -1, b"out is not memory"),
                    ("out one record short of its allocation", (D, n, S, SH, 0, cp, end - 128 * (n - 1)), -1, b"out is not memory"),
                    ("probes one record short of their allocation", (end - 32 * (n - 1), n, S, IRR, 0, cp, O), -1, b"probes is not memory")]
    refused_rays = [("samples not a multiple of 64", (D, n, 100, SH, 3, RY), -1, b"samples"),
                    ("no samples", (D, n, 0, SH, 3, RY), -1, b"samples"),
                    ("too many samples", (D, n, 8192, IRR, 3, RY), -1, b"samples"),
                    ("too many rays", (D, (1 << 22) + 1, 64, SH, 3, RY), -5, b"2^28"),
                    ("unknown what", (D, n, S, 7, 3, RY), -1, b"what"),
                    ("null probes", (0, n, S, SH, 3, RY), -1, b"null"),
                    ("null rays", (D, n, S, IRR, 3, 0), -1, b"null"),
                    ("misaligned probes", (D + 8, n - 1, S, SH, 3, RY), -1, b"misaligned"),
                    ("misaligned rays", (D, n, S, SH, 3, RY + 8), -1, b"misaligned"),
                    ("rays overlapping probes", (D, n, S, SH, 3, D + 32 * (n - 1)), -1, b"overlaps"),
                    ("host-memory probes", (host_ptr, n, S, SH, 3, RY), -1, b"probes is not memory"),
                    ("host-memory rays", (D, n, S, IRR, 3, host_ptr), -1, b"rays is not memory"),
                    ("rays one record short of their allocation", (D, n, S, SH, 3, end - 32 * (n * S - 1)), -1, b"rays is not memory")]
    torch.cuda.synchronize()
    for name, call, cases_ in (("neb_gi_bake_probes", call_bake, refused_bake), ("neb_gi_probe_rays", call_rays, refused_rays)):
        for what, args, want, word in cases_:
            assert call(*args) == want, (name, what, error())
            assert name.encode() in error() and word in error(), (name, what, error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(rays).all()), "a refused call wrote something"
    # n == 0: a no-op that succeeds and looks at no pointer
    assert call_bake(0, 0, S, SH, 0, cp, 0) == 0 and call_bake(0, 0, S, IRR, 0, None, 0) == 0 and call_rays(0, 0, S, SH, 3, 0) == 0
    # ... and the same context answers: the ranges that just fit their allocation are accepted
    assert call_bake(D, n, S, SH, 0, cp, end - 128 * n) == 0
    assert call_rays(D, n, S, SH, int(k3.frameIndex), end - 128 * n - 32 * n * S) == 0
    assert call_bake(D, n, S, SH, 0, cp, O) == 0 and call_rays(D, n, S, SH, int(k3.frameIndex), RY) == 0
    torch.cuda.synchronize()
    res = r.trace_paths(rays[:n * S], constants=k3)
    torch.cuda.synchronize()
    want = B.bake_ref(paths_to_host((res["records"], None))[0], rays[:n * S].cpu().numpy(), S, "sh")
    assert same_bits(records(out[:n]), want)
    assert bool(torch.isnan(out[n]).all()) and bool(torch.isnan(rays[n * S]).all())
    r.destroy()


def test_the_python_mirror_checks_its_arguments_and_returns_the_views(cases):
    r = state_renderer(cases["room"])
    d = on_device(probe_set(cases["room"]["scene"], 10))
    for call in (r.probe_rays, r.bake_probes):
        for bad in (d.cpu(), d[:, :7], d.double(), d[::2]):
            with pytest.raises(NebError):
                call(bad)
        for samples in (0, 32, 100, 4160):
            with pytest.raises(NebError):
                call(d, samples)
        with pytest.raises(NebError):
            call(d, 64, "radiance")
    with pytest.raises(NebError):
        r.bake_probes(d, out=torch.empty((10, 32), dtype=torch.float32))
    with pytest.raises(NebError):
        r.probe_rays(d, 128, out=torch.empty((640, 8), dtype=torch.float32, device="cuda"))
    for K in (1, 9):
        with pytest.raises(NebError):
            r.bake_probes(d, max_path_vertices=K)
    c = P.constants(3)
    res = r.bake_probes(d, 128, "irradiance", constants=c, max_path_vertices=6)
    assert c.maxPathVertices == 3  # the caller's constants are left alone
    views = ("sh", "samples", "hits", "backfaces", "segments", "flags")
    assert set(res) == set(views) | {"irradiance", "records"} and res["records"].shape == (10, 32) and res["sh"].shape == (10, 9, 3)
    assert [res[k].data_ptr() - res["records"].data_ptr() for k in views] == [B.RECORD.fields[k][1] for k in views]
    assert res["irradiance"].data_ptr() == res["records"].data_ptr() and res["irradiance"].shape == (10, 3)
    assert all(res[k].dtype == torch.int32 for k in views[1:])
    torch.cuda.synchronize()
    assert bool((res["samples"] == 128).all()) and bool((res["segments"] > 128).any())
    assert r.probe_rays(d, 64, "irradiance").shape == (640, 8) and r.bake_probes(d)["records"].shape == (10, 32)  # (the frame's own constants)
    assert r.probe_rays(d[:0]).shape == (0, 8) and r.bake_probes(d[:0], 4096, max_path_vertices=8)["records"].shape == (0, 32)
    torch.cuda.synchronize()
    r.destroy()
