"""neb_gi_bake_visibility / neb_gi_accumulate_visibility / neb_gi_gather_probes_visible / neb_gi_probe_indirect_visible
on the device: the bake against tests/probe_visibility_ref.py's float32 reduction of the device's own cast_rays over its own probe_rays,
BIT FOR BIT; free space and a floor; the visible gather against float64 on synthetic maps (every wave shape, both arms, any order, a
point alone, maps that see everything); the lookup at the map's edges; the accumulation inside its bound; the fused frame call bit for
bit; the leak behind a thin wall; refusals, the Python mirror, and the frame left alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import probe_frame_ref as PF
import probe_visibility_ref as R
import probe_volume_ref as PV
import views_ref as V
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from nebulae_amd.svgf import PLANE_RADIANCE, NebError
from test_probe_frame_gpu import H as FH
from test_probe_frame_gpu import W as FW
from test_probe_frame_gpu import gbuffers, lit, radiance_of, room, seed, synthetic, upload_gbuffer  # noqa: F401  (room, synthetic: fixtures)
from test_probe_gpu import FREE_POINT, cases, probe_set  # noqa: F401  (cases: the room fixture of the bake's tests)
from test_probe_volume_gpu import gathered, records_on_device
from test_ray_query_gpu import H, W, on_device, same_bits
from test_ray_query_gpu import to_host as hits_to_host
from test_ray_shade_gpu import state_renderer
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, F64, U32 = np.float32, np.float64, np.uint32
FILL = float("nan")
FRAME_INDEX = 7


@pytest.fixture(scope="module")
def scene_less():
    """a renderer without a scene: only the bake needs one"""
    r = DeferredRenderer()
    r.init(W, H)
    yield r
    r.destroy()


def maps_on_device(maps):
    return torch.from_numpy(np.ascontiguousarray(maps).view(F).reshape(len(maps), 192)).cuda()


def maps_of(out):
    return np.ascontiguousarray(out.cpu().numpy()).view(R.VISIBILITY).reshape(-1)


def frame_constants(frame_index=FRAME_INDEX):
    import path_ref as P
    return P.constants(2, frame_index=frame_index)


def bake(r, pr, S, max_distance, frame_index=FRAME_INDEX):
    d = on_device(pr)
    out = torch.full((len(pr), 192), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res = r.bake_visibility(d, S, max_distance=max_distance, constants=frame_constants(frame_index), out=out)
    torch.cuda.synchronize()
    assert res["records"] is out
    return maps_of(out)


def walked(r, pr, S, frame_index=FRAME_INDEX):
    """probe_rays and cast_rays on the device -> (directions float32 [n, S, 3], t [n, S], hit [n, S]) on the host"""
    d = on_device(pr)
    torch.cuda.synchronize()
    rays = r.probe_rays(d, S, "sh", frame_index=frame_index)
    res = r.cast_rays(rays)
    torch.cuda.synchronize()
    hits = hits_to_host(res["records"])
    n = len(pr)
    return rays.cpu().numpy()[:, 4:7].reshape(n, S, 3), hits["t"].reshape(n, S), np.isfinite(hits["t"]).reshape(n, S)


def bake_want(r, pr, S, max_distance, T=F, frame_index=FRAME_INDEX):
    d, t, hit = walked(r, pr, S, frame_index)
    return R.bake_reduce(d, t, hit, max_distance, T, is_baked=R.baked(pr)), hit


def gather_visible(r, g, d_rec, d_maps, pts, bias=R.NORMAL_BIAS):
    d = on_device(pts)
    out = torch.full((len(pts), 8), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res = r.gather_probes(PV.grid_struct(g), d_rec, d, out=out, visibility=d_maps, normal_bias=bias)
    torch.cuda.synchronize()
    assert res["records"] is out
    got = gathered(out)
    assert not got["reserved"].any()
    return got


def gather_plain(r, g, d_rec, pts):
    res = r.gather_probes(PV.grid_struct(g), d_rec, on_device(pts))
    torch.cuda.synchronize()
    return gathered(res["records"])


# ------------------------------------------------------------------------------------------------
# 1: bake == reduce(cast_rays(probe_rays)), bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("S", [64, 256])
def test_bake_is_the_reduction_of_cast_rays_over_probe_rays_bit_for_bit(cases, S, exact):
    case = cases["room, extras"]
    r = state_renderer(case, bool(exact))
    pr = probe_set(case["scene"], 10)
    D = 1.5
    got = bake(r, pr, S, D)
    want, hit = bake_want(r, pr, S, D)
    want = R.as_array(want)
    if not same_bits(got, want):
        bad = np.argwhere(got["moments"].view(U32) != want["moments"].view(U32))
        raise AssertionError(f"S {S} / exact {exact}: {len(bad)} moments differ from reduce(cast_rays(probe_rays)); first: probe, texel, moment {bad[0]}: "
                             f"{got['moments'][tuple(bad[0])]} != {want['moments'][tuple(bad[0])]}")
    assert hit.mean() > 0.5 and not hit.all() and (got["weight"] > 0).all()  # (a room open in front; 64 stratified samples fill every texel)
    assert (got["moments"][..., 0] < D).mean() > 0.25 and (got["moments"][..., 0] <= D * (1 + 2.0 ** -21)).all()  # (distances, not max_distance; a rounded mean may pass its largest term by an ulp or two)
    worst = R.judge_bake(got, bake_want(r, pr, S, D, F64)[0], f"S {S}")
    print(f"[bake / S {S} / exact {exact}] largest error against float64 {worst:.3e} / {R.TOL['bake']:.1e}")
    # a second call, and a probe baked alone (probe 0: a sample's index depends on the probe's place in the call)
    assert same_bits(bake(r, pr, S, D), got) and same_bits(bake(r, pr[:1], S, D), got[:1])
    assert not same_bits(bake(r, pr, S, D, frame_index=FRAME_INDEX + 1), got)
    # probes that cannot be baked get max_distance everywhere and leave their neighbours alone
    spoiled = pr.copy()
    spoiled[3, 1], spoiled[6, 7] = np.nan, spoiled[6, 3]
    again = bake(r, spoiled, S, D)
    keep = np.ones(10, bool)
    keep[[3, 6]] = False
    assert same_bits(again[keep], got[keep])
    assert (again["moments"][~keep] == (F(D), F(D) * F(D))).all() and not again["weight"][~keep].any()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: free space and a closed form
# ------------------------------------------------------------------------------------------------
def test_free_space_and_a_floor(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    sc = case["scene"]
    assert not case["hidden"]
    free = PV.grid_probes(PV.grid(FREE_POINT, (1.0, 1.0, 1.0), (1, 1, 1)), tmin=0.0, tmax=1e4)
    # max_distance below the nearest surface: every texel is (max_distance, max_distance^2) EXACTLY, with its filter weight.  (The
    # contract's quotient (sum of g * D) / (sum of g) is D to the bit where D is a power of two -- the products and the sums then scale
    # exactly --, and within an ulp or two of it otherwise.)
    D = 2.0 ** -11
    got = bake(r, free, 64, D)
    assert (got["moments"] == (F(D), F(D) * F(D))).all() and (got["weight"] > 0).all()
    got = bake(r, free, 64, 9e-4)
    assert np.abs(got["moments"].astype(F64) / (F(9e-4), F(9e-4) * F(9e-4)) - 1.0).max() < 4 * 2.0 ** -23
    # a probe 0.25 above the floor (y = -1): the device is within the tolerance of the float64 reduction of the float64 brute-force cast
    # along the same directions, and the texels that look down hold a mean distance between the nearest surface and max_distance
    h = 0.25
    pr = PV.grid_probes(PV.grid((FREE_POINT[0], -1.0 + h, FREE_POINT[2]), (1.0, 1.0, 1.0), (1, 1, 1)), tmin=0.0, tmax=1e4)
    S, D = 256, 2.0
    got = bake(r, pr, S, D)
    dirs, t_dev, hit_dev = walked(r, pr, S)
    ref = V.cast(V.triangles(sc), pr[0, 0:3].astype(F64), dirs.reshape(-1, 3).astype(F64), 0.0, 1e4)
    want = R.bake_reduce(dirs, ref["t"].reshape(1, S), np.isfinite(ref["t"]).reshape(1, S), D)
    # (the walk's float32 t comes out of a dozen float32 operations: 16 ulp on t at most, twice that on t * t, at the largest moment D * D)
    worst = R.judge_bake(got, want, "floor, against the float64 caster", tol=R.TOL["bake"] + 32 * 2.0 ** -24 * D * D)
    down = np.flatnonzero(R.texel_directions()[:, 1] < -0.95)
    m1 = got["moments"][0, down, 0]
    print(f"[floor] largest error against the float64 caster's maps {worst:.3e}; mean distance in the {len(down)} texels that look down: {m1}")
    nearest = float(ref["t"].min())
    assert len(down) >= 2 and 0.0 < nearest <= h and (m1 >= nearest).all() and (m1 < 2.0 * h).all()  # (the room's extras lie nearer than the floor)
    # the whole scene hidden: max_distance everywhere, whatever it is
    r.set_visible(list(range(len(sc.geometries))), False)
    got = bake(r, free, 64, 4.0)
    assert (got["moments"] == (F(4.0), F(16.0))).all() and (got["weight"] > 0).all()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3: the gather on synthetic maps (no scene)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", PV.DIMS)
def test_the_visible_gather_matches_float64_on_every_wave_shape(scene_less, dims):
    r = scene_less
    g = PV.gpu_grid(dims)
    rec, maps = PV.random_records(g), R.random_maps(g)
    d_rec, d_maps = records_on_device(rec), maps_on_device(maps)
    d_clear = maps_on_device(R.all_visible(PV.count(g), 64.0))
    worst, branches = 0.0, []
    for n in PV.COUNTS:
        for kind in R.KINDS:
            pts = PV.points(g, kind, n)
            parts = {}
            want = R.gather64(g, rec, maps, R.NORMAL_BIAS, pts, parts=parts)
            got = gather_visible(r, g, d_rec, d_maps, pts)
            worst = max(worst, R.judge_gather(PV.as_dict(got), want, f"{dims} / {n} / {kind}"))
            branches.append(parts["branch"])
            # maps that see everything: the plain gather's bits
            assert same_bits(gather_visible(r, g, d_rec, d_clear, pts), gather_plain(r, g, d_rec, pts)), (dims, n, kind)
            if n == 4097 and kind == "one cell":
                plain = gather_plain(r, g, d_rec, pts)
                assert dims == (1, 1, 1) or not same_bits(got["irradiance"], plain["irradiance"])  # (the maps act; the one probe of (1, 1, 1) sees every point)
                # both arms, any order, a point alone: mixed with points of other cells the same points take the per-lane arm
                other = PV.points(g, "all cells", n)
                order = np.random.default_rng(1).permutation(2 * n)
                mixed = gather_visible(r, g, d_rec, d_maps, np.concatenate([pts, other])[order])
                back = np.empty_like(mixed)
                back[order] = mixed
                assert same_bits(back[:n], got)
                for i in (0, 17, 4096):
                    assert same_bits(gather_visible(r, g, d_rec, d_maps, pts[i:i + 1]), got[i:i + 1])
    shares = R.branch_shares(dict(branch=np.concatenate(branches, 1)))
    print(f"[gather / {dims}] largest error {worst:.3e} / {R.TOL['gather']:.1e}; corners r <= m1 {shares[0]:.2f}, Chebyshev {shares[1]:.2f}, floor {shares[2]:.2f}")
    if dims != (1, 1, 1):  # (one probe, and every point on its plane close by: r <= m1 throughout)
        assert min(shares) >= 0.1, shares


# ------------------------------------------------------------------------------------------------
# 4: the lookup at the edges of the map
# ------------------------------------------------------------------------------------------------
def test_the_lookup_at_the_edges_of_the_map(scene_less):
    """One probe whose map holds the texel's index as m1 (and a variance that keeps the factor off its floor), points all around it at
    one distance: in the map's rows and columns -1 and 7, on uz = 0 and below it.  The weight of the one corner is w_n * vis."""
    r = scene_less
    g = PV.grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1))
    rec = PV.random_records(g)
    maps = np.zeros(1, R.VISIBILITY)
    m1 = (1.0 + np.arange(64) / 128.0).astype(F)  # (with r = 1.6 and var = m1 m1 / 2 the factor runs from 0.2 to 1: off its floor)
    maps["moments"][0, :, 0], maps["moments"][0, :, 1], maps["weight"] = m1, (m1 * m1 * F(1.5)).astype(F), 1.0
    rng = np.random.default_rng(4)
    u = rng.standard_normal((4096, 3))
    u[0:512, 2] = 0.0                                                    # on the fold
    u[512:1024, 2] = -np.abs(u[512:1024, 2])                             # below it
    u[1024:1536, 0], u[1024:1536, 2] = 1e-6 * u[1024:1536, 0], -np.abs(u[1024:1536, 2])  # along the edges ux = 0 ...
    u[1536:2048, 1], u[1536:2048, 2] = 1e-6 * u[1536:2048, 1], -np.abs(u[1536:2048, 2])  # ... and uy = 0
    u[2048:2304] = 1e-3 * u[2048:2304] + (0.0, 0.0, -1.0)                # the four corners: the pole -z
    u = 1.6 * u / np.linalg.norm(u, axis=-1, keepdims=True)
    pts = np.zeros((len(u), 8), F)
    pts[:, 0:3], pts[:, 4:7], pts[:, 7] = u, rng.standard_normal((len(u), 3)), 1.0
    taps, fx, fy = R.lookup(pts[:, 0:3].astype(F64), F64)
    rim = (taps[0] != taps[1] - 1) | (taps[2] != taps[0] + 8)  # a tap of the four was wrapped
    assert rim[1024:2304].mean() > 0.9 and rim.sum() > 1500 and len(np.unique(taps)) == 64
    d_rec, d_maps = records_on_device(rec), maps_on_device(maps)
    want = R.gather64(g, rec, maps, 0.0, pts)
    got = gather_visible(r, g, d_rec, d_maps, pts, bias=0.0)
    worst = R.judge_gather(PV.as_dict(got), want, "edges")
    clamp = R.gather64(g, rec, maps, 0.0, pts, corrupt="wrap replaced by clamp")
    no_fold = R.gather64(g, rec, maps, 0.0, pts, corrupt="fold sign dropped")
    for name, bad in (("clamp", clamp), ("no fold sign", no_fold)):
        off = np.abs(got["weight"].astype(F64) - bad["weight"])
        assert (off > 10 * R.TOL["gather"]).sum() > 100, name  # (the device does not follow the corrupted lookups)
    print(f"[edges] largest error {worst:.3e}; {int(rim.sum())} of {len(pts)} points tap across an edge")


# ------------------------------------------------------------------------------------------------
# 5: the accumulation
# ------------------------------------------------------------------------------------------------
def test_accumulation_from_a_zeroed_start_stays_inside_the_carried_bound(scene_less):
    r = scene_less
    g = PV.gpu_grid((5, 4, 3))
    n = PV.count(g)
    rng = np.random.default_rng(6)
    bakes = []
    for q in range(3):
        m = R.random_maps(g, seed=30 + q)
        m["weight"][rng.uniform(size=m["weight"].shape) < 0.15] = 0.0
        m["moments"][m["weight"] == 0] = np.nan  # (a texel that was never filled is never read)
        bakes.append(m)
    acc = torch.zeros((n, 192), dtype=torch.float32, device="cuda")
    ref = R.Accumulator64(n)
    for k, m in enumerate(bakes):
        d = maps_on_device(m)
        assert r.accumulate_visibility(acc, d) is acc
        torch.cuda.synchronize()
        assert same_bits(maps_of(d), m)  # (`add` is read only)
        ref.add(m)
        got = maps_of(acc)
        filled = ref.weight > 0
        worst = R.judge_accumulation(got, ref.records, ref.value, ref.bound, f"fold {k}")
        if k == 0:  # a zeroed start takes `add`, bit for bit where it has weight
            assert same_bits(got["moments"][filled], m["moments"][filled]) and same_bits(got["weight"], m["weight"])
    print(f"[accumulate] largest error after three folds {worst:.3f} of the bound")
    assert worst > 0.0 and ref.folds.max() == 2
    before = maps_of(acc)
    empty = bakes[0].copy()
    empty["weight"][...] = 0.0
    r.accumulate_visibility(acc, maps_on_device(empty))
    torch.cuda.synchronize()
    assert same_bits(maps_of(acc), before)  # (an `add` without weight keeps every bit)


# ------------------------------------------------------------------------------------------------
# 6: the fused frame call
# ------------------------------------------------------------------------------------------------
def lit_visible(r, g, d_rec, d_maps, radiance, bias=R.NORMAL_BIAS, frame_weight=False, rows=None):
    seed(r, radiance)
    r.submit_commands_gi_probes(PV.grid_struct(g), d_rec, frame_weight=frame_weight, rows=rows, visibility=d_maps, normal_bias=bias)
    return radiance_of(r)


@pytest.mark.parametrize("kind", ("room",) + PF.KINDS)
def test_the_fused_frame_call_is_the_visible_gather_of_the_frames_points_bit_for_bit(room, synthetic, kind):
    rad = PF.random_radiance(FW, FH)
    for dims in PF.GRIDS:
        r, g, planes = gbuffers(room, synthetic, kind, dims)
        rec = PV.random_records(g)
        maps = R.random_maps(g)
        d_rec, d_maps = records_on_device(rec), maps_on_device(maps)
        pts = r.gbuffer_points()
        res = r.gather_probes(PV.grid_struct(g), d_rec, pts, visibility=d_maps, normal_bias=R.NORMAL_BIAS)
        torch.cuda.synchronize()
        res = PV.as_dict(gathered(res["records"]))
        got = lit_visible(r, g, d_rec, d_maps, rad)
        n = PF.judge_identity(got, rad, planes, res, f"{kind} / {dims}")  # (every bit, the pixels not stored to -- sky among them -- included)
        sky = PF.sky(planes)
        assert n > 300 and same_bits(got[sky], rad[sky]) and not same_bits(got, rad)
        plain = lit(r, g, d_rec, rad)
        assert dims == (1, 1, 1) or not same_bits(plain, got)  # (the maps act)
        weighted = lit_visible(r, g, d_rec, d_maps, rad, frame_weight=True)
        PF.judge_weighted(weighted, rad, planes, res, tuple(r.info.camera.eye), f"{kind} / {dims}, weighted")
        # maps that see everything: the bits of the existing call, with and without the weight, and over a row range
        d_clear = maps_on_device(R.all_visible(PV.count(g), 64.0))
        assert same_bits(lit_visible(r, g, d_rec, d_clear, rad), plain)
        assert same_bits(lit_visible(r, g, d_rec, d_clear, rad, frame_weight=True), lit(r, g, d_rec, rad, frame_weight=True))
        part = lit_visible(r, g, d_rec, d_maps, rad, rows=(3, 21))
        assert same_bits(part[3:21], got[3:21]) and same_bits(part[:3], rad[:3]) and same_bits(part[21:], rad[21:])


# ------------------------------------------------------------------------------------------------
# 7: the leak
# ------------------------------------------------------------------------------------------------
def test_a_lit_room_no_longer_leaks_through_a_thin_wall():
    """tests/probe_visibility_ref.py's leak fixture: the maps baked on the device, the SH records synthetic (radiance 1 on the probes of
    the lit half, 0 on the others), 200 points on the floor and a wall of the dark half inside the cell layer that straddles the divider.
    The float64 reference's ratio sum(E_visible) / sum(E_plain), from maps built with the float64 brute-force caster, is 0.0620
    (test_probe_visibility_cpu); the device may show at most twice that."""
    sc, g = R.leak_scene(), R.leak_grid()
    r = _renderer(sc, cornell_camera(), W, H, sun_table=0, hits=False, exact=False)
    pr = PV.grid_probes(g, tmin=0.0, tmax=1e4)
    n, S = len(pr), R.LEAK_SAMPLES
    maps = bake(r, pr, S, R.LEAK_MAX_DISTANCE, frame_index=1)
    want_maps, hit = bake_want(r, pr, S, R.LEAK_MAX_DISTANCE, frame_index=1)
    assert same_bits(maps, R.as_array(want_maps))
    rec, pts = R.leak_records(g), R.leak_points()
    d_rec, d_maps = records_on_device(rec), maps_on_device(maps)
    visible = gather_visible(r, g, d_rec, d_maps, pts, bias=R.LEAK_BIAS)
    plain = gather_plain(r, g, d_rec, pts)
    want = R.gather64(g, rec, maps, R.LEAK_BIAS, pts)  # (the reference fed the device's maps)
    R.judge_gather(PV.as_dict(visible), want, "leak")
    Ev, Ep = visible["irradiance"][:, 0].astype(F64), plain["irradiance"][:, 0].astype(F64)
    assert (Ep > 0).all() and (Ev < Ep).all()
    # the float64 reference from end to end: the float64 directions, the brute-force caster, the float64 reduction and gather
    dirs = R.probe_directions64(pr, S, 1)
    ref = V.cast(V.triangles(sc), np.repeat(pr[:, 0:3].astype(F64), S, 0), dirs.reshape(-1, 3), 0.0, 1e4)
    t = ref["t"].reshape(n, S)
    maps64 = R.bake_reduce(dirs, t, np.isfinite(t), R.LEAK_MAX_DISTANCE)
    vis64 = R.as_array({k: v.astype(F) for k, v in maps64.items()})
    ref_ratio = float(R.gather64(g, rec, vis64, R.LEAK_BIAS, pts)["irradiance"][:, 0].sum() / PV.gather64(g, rec, pts)["irradiance"][:, 0].sum())
    ratio = float(Ev.sum() / Ep.sum())
    print(f"[leak] sum(E_visible) / sum(E_plain): device {ratio:.4f}, float64 reference {ref_ratio:.4f}")
    assert ref_ratio < 0.5 and ratio <= 2.0 * ref_ratio
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 8: refusals and the Python mirror
# ------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_name_the_cause(cases, synthetic):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    fr = synthetic[(FW, FH)]
    lib = r._lib
    g = PV.gpu_grid((5, 4, 3))
    m, n = 60, 65
    rec, maps, pts = PV.random_records(g), R.random_maps(g), PV.points(g, "all cells", n)
    d_rec, d_maps, d_pts, d_probes = records_on_device(rec), maps_on_device(maps), on_device(pts), on_device(PV.grid_probes(g, 0.0, 5.0))
    out_maps = torch.full((m + 1, 192), FILL, dtype=torch.float32, device="cuda")
    acc = torch.full((m + 1, 192), FILL, dtype=torch.float32, device="cuda")
    out = torch.full((n + 1, 8), FILL, dtype=torch.float32, device="cuda")
    host_mem = torch.empty((m * 192 + 16,), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    ok = PV.grid_struct(g)
    planes = PF.synthetic_gbuffer(g, "permuted", FW, FH)
    rad = PF.random_radiance(FW, FH)
    upload_gbuffer(fr, planes)
    seed(fr, rad)
    radiance_ptr = fr.svgf.get_plane(PLANE_RADIANCE)[0]
    c = fr.global_constants()
    nan, inf = float("nan"), float("inf")

    def call_bake(x, p_probes, count, S, D, p_out):
        return lib.neb_gi_bake_visibility(x._ctx, C.c_void_p(p_probes), count, S, FRAME_INDEX, D, C.c_void_p(p_out), None)

    def call_acc(x, p_acc, p_add, count):
        return lib.neb_gi_accumulate_visibility(x._ctx, C.c_void_p(p_acc), C.c_void_p(p_add), count, None)

    def call_gather(x, grid, p_rec, p_vis, bias, p_pts, count, p_out):
        return lib.neb_gi_gather_probes_visible(x._ctx, None if grid is None else C.byref(grid), C.c_void_p(p_rec), C.c_void_p(p_vis), bias, C.c_void_p(p_pts),
                                                count, C.c_void_p(p_out), None)

    def call_indirect(x, grid, p_rec, p_vis, bias, constants, flags, rows=None):
        a = (x._ctx, None if grid is None else C.byref(grid), C.c_void_p(p_rec), C.c_void_p(p_vis), bias, None if constants is None else C.byref(constants), flags)
        return lib.neb_gi_probe_indirect_visible(*a, None) if rows is None else lib.neb_gi_probe_indirect_visible_rows(*a, rows[0], rows[1], None)

    bad_grid = PV.grid_struct(g)
    bad_grid.dims[1] = 0
    PR, OM, AC, AD, RE, VI, PT, OU = (t.data_ptr() for t in (d_probes, out_maps, acc, d_maps, d_rec, d_maps, d_pts, out))
    refused = [
        ("neb_gi_bake_visibility", call_bake, [
            ("no scene", (fr, PR, m, 64, 1.0, OM), -4, b"not ready"), ("samples of 0", (r, PR, m, 0, 1.0, OM), -1, b"samples"),
            ("samples of 96", (r, PR, m, 96, 1.0, OM), -1, b"samples"), ("samples above 4096", (r, PR, m, 4160, 1.0, OM), -1, b"samples"),
            ("too many samples", (r, PR, 1 << 20, 4096, 1.0, OM), -5, b"2^28"), ("max_distance of 0", (r, PR, m, 64, 0.0, OM), -1, b"max_distance"),
            ("negative max_distance", (r, PR, m, 64, -1.0, OM), -1, b"max_distance"), ("nan max_distance", (r, PR, m, 64, nan, OM), -1, b"max_distance"),
            ("infinite max_distance", (r, PR, m, 64, inf, OM), -1, b"max_distance"), ("null probes", (r, 0, m, 64, 1.0, OM), -1, b"null"),
            ("null out", (r, PR, m, 64, 1.0, 0), -1, b"null"), ("misaligned probes", (r, PR + 8, m - 1, 64, 1.0, OM), -1, b"misaligned"),
            ("misaligned out", (r, PR, m, 64, 1.0, OM + 16), -1, b"misaligned"), ("out is probes", (r, OM, 2, 64, 1.0, OM), -1, b"overlaps"),
            ("host-memory out", (r, PR, m, 64, 1.0, host_ptr), -1, b"out is not memory"),
            ("out one short of its allocation", (r, PR, m, 64, 1.0, end - 768 * (m - 1)), -1, b"out is not memory")]),
        ("neb_gi_accumulate_visibility", call_acc, [
            ("null acc", (fr, 0, AD, m), -1, b"null"), ("null add", (fr, AC, 0, m), -1, b"null"), ("misaligned acc", (fr, AC + 16, AD, m - 1), -1, b"misaligned"),
            ("misaligned add", (fr, AC, AD + 16, m - 1), -1, b"misaligned"), ("add is acc", (fr, AC, AC, m), -1, b"overlaps"),
            ("add overlapping acc", (fr, AC, AC + 768, 2), -1, b"overlaps"), ("host-memory acc", (fr, host_ptr, AD, m), -1, b"acc is not memory"),
            ("host-memory add", (fr, AC, host_ptr, m), -1, b"add is not memory"),
            ("acc one short of its allocation", (fr, end - 768 * (m - 1), AD, m), -1, b"acc is not memory")]),
        ("neb_gi_gather_probes_visible", call_gather, [
            ("a dims of 0", (fr, bad_grid, RE, VI, 0.0, PT, n, OU), -1, b"dims"), ("null grid", (fr, None, RE, VI, 0.0, PT, n, OU), -1, b"null grid"),
            ("negative bias", (fr, ok, RE, VI, -0.1, PT, n, OU), -1, b"normal_bias"), ("nan bias", (fr, ok, RE, VI, nan, PT, n, OU), -1, b"normal_bias"),
            ("infinite bias", (fr, ok, RE, VI, inf, PT, n, OU), -1, b"normal_bias"), ("null visibility", (fr, ok, RE, 0, 0.0, PT, n, OU), -1, b"null visibility"),
            ("null records", (fr, ok, 0, VI, 0.0, PT, n, OU), -1, b"null"), ("misaligned visibility", (fr, ok, RE, VI + 16, 0.0, PT, n, OU), -1, b"misaligned"),
            ("host-memory visibility", (fr, ok, RE, host_ptr, 0.0, PT, n, OU), -1, b"visibility is not memory"),
            ("visibility one short of its allocation", (fr, ok, RE, end - 768 * (m - 1), 0.0, PT, n, OU), -1, b"visibility is not memory"),
            ("out inside visibility", (fr, ok, RE, AC, 0.0, PT, n, AC + 768), -1, b"overlaps visibility"),
            ("out is points", (fr, ok, RE, VI, 0.0, OU, n, OU), -1, b"overlaps points")]),
        ("neb_gi_probe_indirect_visible", call_indirect, [
            ("a dims of 0", (fr, bad_grid, RE, VI, 0.0, c, 0), -1, b"dims"), ("an unknown flag bit", (fr, ok, RE, VI, 0.0, c, 2), -1, b"flags"),
            ("the frame weight without constants", (fr, ok, RE, VI, 0.0, None, 1), -1, b"null constants"),
            ("negative bias", (fr, ok, RE, VI, -0.1, c, 0), -1, b"normal_bias"), ("nan bias", (fr, ok, RE, VI, nan, c, 0), -1, b"normal_bias"),
            ("null visibility", (fr, ok, RE, 0, 0.0, c, 0), -1, b"null visibility"), ("null records", (fr, ok, 0, VI, 0.0, c, 0), -1, b"null records"),
            ("misaligned visibility", (fr, ok, RE, VI + 16, 0.0, c, 0), -1, b"misaligned"),
            ("host-memory visibility", (fr, ok, RE, host_ptr, 0.0, c, 0), -1, b"visibility is not memory"),
            ("visibility one short of its allocation", (fr, ok, RE, end - 768 * (m - 1), 0.0, c, 0), -1, b"visibility is not memory"),
            ("visibility inside the radiance plane", (fr, ok, RE, radiance_ptr + 768, 0.0, c, 0), -1, b"overlaps the radiance plane"),
            ("rows past the frame", (fr, ok, RE, VI, 0.0, c, 0, (40, FH + 1)), -5, b"rows"), ("no rows", (fr, ok, RE, VI, 0.0, c, 0, (9, 9)), -5, b"rows")])]
    torch.cuda.synchronize()
    for name, call, cases_ in refused:
        for what, args, code, word in cases_:
            assert call(*args) == code, (name, what, lib.neb_last_error(args[0]._ctx))
            error = lib.neb_last_error(args[0]._ctx)
            assert name.encode() in error and word in error, (name, what, error)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_maps).all()) and bool(torch.isnan(acc).all()) and bool(torch.isnan(out).all()), "a refused call wrote something"
    assert same_bits(radiance_of(fr), rad)
    # n == 0 succeeds and looks at no pointer; ranges that just fit their allocation are accepted, and the same contexts answer
    assert call_bake(r, 0, 0, 64, 1.0, 0) == 0 and call_acc(fr, 0, 0, 0) == 0 and call_gather(fr, ok, 0, 0, 0.0, 0, 0, 0) == 0
    block[-768 * m:].view(torch.float32).view(m, 192).copy_(d_maps)
    torch.cuda.synchronize()
    assert call_gather(fr, ok, RE, end - 768 * m, R.NORMAL_BIAS, PT, n, OU) == 0
    assert call_bake(r, PR, m, 64, 1.0, OM) == 0 and call_acc(fr, end - 768 * m, AD, m) == 0
    torch.cuda.synchronize()
    R.judge_gather(PV.as_dict(gathered(out[:n])), R.gather64(g, rec, maps, R.NORMAL_BIAS, pts), "after the refusals")
    assert bool(torch.isnan(out[n]).all()) and bool(torch.isnan(out_maps[m]).all()) and bool(torch.isfinite(out_maps[:m]).all())
    r.destroy()


def test_the_python_mirror_checks_its_arguments_and_returns_the_views(cases, synthetic):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    fr = synthetic[(FW, FH)]
    g = PV.gpu_grid((5, 4, 3))
    grid = PV.grid_struct(g)
    rec, maps = records_on_device(PV.random_records(g)), maps_on_device(R.random_maps(g))
    pts, probes = on_device(PV.points(g, "all cells", 10)), on_device(PV.grid_probes(g, 0.0, 5.0))
    c = frame_constants()
    for kw in (dict(samples=96), dict(samples=0), dict(max_distance=None), dict(max_distance=0.0), dict(max_distance=float("nan")),
               dict(out=torch.empty((60, 192))), dict(out=torch.empty((59, 192), device="cuda")), dict(out=torch.empty((60, 128), device="cuda"))):
        with pytest.raises(NebError):
            r.bake_visibility(probes, **{**dict(samples=64, max_distance=1.0, constants=c), **kw})
    with pytest.raises(NebError):
        r.bake_visibility(probes.cpu(), 64, max_distance=1.0, constants=c)
    for a, b in ((maps.cpu(), maps), (maps, maps[:59]), (maps[:, :191], maps[:, :191]), (maps.double(), maps.double()), (maps[::2], maps[::2])):
        with pytest.raises(NebError):
            fr.accumulate_visibility(a, b)
    for kw in (dict(visibility=maps[:59]), dict(visibility=maps.cpu()), dict(visibility=maps.double()), dict(visibility=maps[:, :128]),
               dict(visibility=maps, normal_bias=-0.1), dict(visibility=maps, normal_bias=float("nan")), dict(normal_bias=0.1)):
        with pytest.raises(NebError):
            fr.gather_probes(grid, rec, pts, **kw)
        with pytest.raises(NebError):
            fr.submit_commands_gi_probes(grid, rec, frame_weight=False, **kw)
    res = r.bake_visibility(probes, 64, max_distance=1.0, constants=c)
    views = ("moments", "weight")
    assert set(res) == set(views) | {"records"} and res["records"].shape == (60, 192) and res["moments"].shape == (60, 64, 2) and res["weight"].shape == (60, 64)
    assert [res[k].data_ptr() - res["records"].data_ptr() for k in views] == [R.VISIBILITY.fields[k][1] for k in views]
    assert r.bake_visibility(probes[:0], 64, max_distance=1.0, constants=c)["records"].shape == (0, 192)
    acc = torch.zeros_like(res["records"])
    assert fr.accumulate_visibility(acc, res["records"]) is acc
    out = fr.gather_probes(grid, rec, pts, visibility=acc, normal_bias=0.01)
    assert fr.submit_commands_gi_probes(grid, rec, frame_weight=False, visibility=acc, normal_bias=0.01) is None
    torch.cuda.synchronize()
    assert same_bits(acc.cpu().numpy(), res["records"].cpu().numpy()) and bool((out["weight"] > 0).any())
    assert sorted(n for n in _lib.exported_symbols() if "visib" in n and n.startswith("neb_gi_") and "set_" not in n and "get_" not in n) == [
        "neb_gi_accumulate_visibility", "neb_gi_bake_visibility", "neb_gi_gather_probes_visible", "neb_gi_probe_indirect_visible",
        "neb_gi_probe_indirect_visible_rows"]
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 9: the frame left alone
# ------------------------------------------------------------------------------------------------
def test_the_bake_and_the_gather_leave_the_frame_its_counter_and_the_sun_table_alone(cases):
    case = cases["room, extras"]
    sc, cam = clone(case["scene"]), cornell_camera()
    r = _renderer(sc, cam, 64, 48, sun_table=1, hits=True)
    for f in (2, 3):
        frame(r, sc, cam, f)

    def snapshot():
        torch.cuda.synchronize()
        return r.ray_count(), r.traversal_stats(), r.sun_table_stats(), r.svgf.download(PLANE_RADIANCE).copy()
    count, trav, table, plane = snapshot()
    assert count > 0 and table["builds"] == 1 and plane[..., :3].max() > 0.05
    g = PV.gpu_grid((5, 4, 3))
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    maps = r.bake_visibility(d_probes, 128, max_distance=1.5)
    acc = torch.zeros_like(maps["records"])
    r.accumulate_visibility(acc, maps["records"])
    res = r.gather_probes(grid, records_on_device(PV.random_records(g)), on_device(PV.points(g, "all cells", 4097)), visibility=acc, normal_bias=0.01)
    torch.cuda.synchronize()
    assert bool((res["weight"] > 0).any()) and bool((maps["weight"] > 0).any())
    count2, trav2, table2, plane2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(plane2, plane)
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05
    r.destroy()
