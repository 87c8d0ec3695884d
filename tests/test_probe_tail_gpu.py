"""neb_gi_trace_paths_tail / neb_gi_bake_probes_tail on the device: tail=None and an empty grid against the plain calls bit
for bit; a closed form; the general case under the judge of tests/probe_tail_ref.py with the library's own shade_rays and gather_probes as
its queries (every K, policy, weight, gather and wave shape, on the wave-uniform and the per-lane route); the bake as the reduction of the
path query; determinism; monotonicity; the convergence of the feedback loop toward the library's own deep paths; stream ordering; the
frame left alone; refusals and the Python mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

import path_ref as P
import probe_ref as B
import probe_tail_ref as T
import probe_volume_ref as PV
import ray_query_ref as Q
import ray_shade_ref as R
import views_ref as V
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer, ProbeTail, RenderInfo
from nebulae_amd.svgf import PLANE_RADIANCE, NebError
from test_path_gpu import to_host as paths_to_host
from test_probe_gpu import cases, enqueue_bake, probe_set, records  # noqa: F401  (cases: the room fixture of the bake's tests)
from test_probe_volume_gpu import gathered, records_on_device, room_grid
from test_ray_query_gpu import H, W, on_device, same_bits
from test_ray_shade_gpu import renderer, state_renderer
from test_ray_shade_gpu import shade as shade_rays
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, F64, U32 = np.float32, np.float64, np.uint32
FILL = float("nan")
BIAS = 0.02
COUNTS = (1, 63, 64, 65, 4097)


# ------------------------------------------------------------------------------------------------
def enqueue_trace(r, d_rays, c, tail=None, sort=False, vertices=True, stream=None):
    """one call into buffers filled with a pattern no record has -> (out, vertices or None) tensors (nothing waits)"""
    n, K = d_rays.shape[0], int(c.maxPathVertices)
    out = torch.full((n, 8), FILL, dtype=torch.float32, device="cuda")
    vert = torch.full((n, K - 1, 24), FILL, dtype=torch.float32, device="cuda") if vertices else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = r.trace_paths(d_rays, constants=c, sort=sort, vertices=vert if vertices else False, out=out, stream=None if stream is None else stream.cuda_stream,
                        tail=tail)
    assert res["records"] is out
    return out, vert


def trace(r, rays, c, tail=None, sort=False, vertices=True):
    d = rays if isinstance(rays, torch.Tensor) else on_device(rays)
    torch.cuda.synchronize()
    pair = enqueue_trace(r, d, c, tail, sort, vertices)
    torch.cuda.synchronize()
    return paths_to_host(pair)


def tail_bake(r, d_probes, S, what, c, tail, stream=None):
    out = torch.full((d_probes.shape[0], 32), FILL, dtype=torch.float32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = r.bake_probes(d_probes, S, what, constants=c, out=out, stream=None if stream is None else stream.cuda_stream, tail=tail)
    assert res["records"] is out
    return out


def baked(r, d_probes, S, what, c, tail=None):
    torch.cuda.synchronize()
    out = tail_bake(r, d_probes, S, what, c, tail)
    torch.cuda.synchronize()
    return records(out)


def gather_on(r, tail):
    def gather(points):
        res = r.gather_probes(tail.grid, tail.records, on_device(points), visibility=tail.visibility, normal_bias=tail.normal_bias)
        torch.cuda.synchronize()
        return gathered(res["records"])
    return gather


def pd64_on(case):
    tris = Q.triangles(case["scene"], case["hidden"])

    def pd64(rays, surface):
        ref = R.reading64(case["scene"], tris, rays, surface["geometry"], surface["primitive"])
        V64, SN64 = R._unit(-rays[:, 4:7].astype(F64)), R._unit(ref["SN"])
        f0 = 0.04 + ref["metalness"][:, None] * (ref["albedo"] - 0.04)
        return 1.0 - P._specular_probability64(np.sum(V64 * SN64, -1), f0, ref["albedo"])
    return pd64


def room_volume(r, sc, dims, S=64, K=2, frame_index=11, visibility=True):
    """a grid over the room baked on the device -> dict(grid, probes, records, maps): device tensors"""
    g = room_grid(sc, dims)
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    rec = enqueue_bake(r, d_probes, S, "sh", P.constants(K, frame_index=frame_index))
    maps = None
    if visibility:
        reach = 1.5 * float(np.linalg.norm(g["spacing"]))
        maps = r.bake_visibility(d_probes, 64, max_distance=reach, constants=P.constants(2, frame_index=frame_index))["records"]
    torch.cuda.synchronize()
    return dict(g=g, grid=grid, probes=d_probes, records=rec, maps=maps)


def tail_of(vol, visible=False, frame_weight=True, records=None):
    return ProbeTail(vol["grid"], vol["records"] if records is None else records, vol["maps"] if visible else None, BIAS if visible else 0.0, frame_weight)


def pool(sc, n=4097, seed=7):
    return Q.scattered_rays(*Q.scene_box(sc), n, np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------
# 1, 2: tail=None and a grid without a valid probe are the plain call, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
def test_no_tail_and_an_empty_grid_are_the_plain_call_bit_for_bit(cases, exact):
    case = cases["room, extras"]
    r = state_renderer(case, bool(exact))
    lib, ctx = r._lib, r._ctx
    c = P.constants(3)
    d_rays = on_device(pool(case["scene"], 65))
    plain = trace(r, d_rays, c)
    # the C entry point with tail == NULL
    out = torch.full((65, 8), FILL, dtype=torch.float32, device="cuda")
    vert = torch.full((65, 2, 24), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.neb_gi_trace_paths_tail(ctx, C.c_void_p(d_rays.data_ptr()), 65, 0, C.byref(c), None, C.c_void_p(out.data_ptr()), C.c_void_p(vert.data_ptr()), None) == 0
    torch.cuda.synchronize()
    null = paths_to_host((out, vert))
    assert same_bits(null[0].view(U32), plain[0].view(U32)) and same_bits(null[1].view(U32), plain[1].view(U32))
    assert (plain[0]["segments"] == 2).sum() > 20
    d_probes = on_device(probe_set(case["scene"], 3))
    plain_bake = baked(r, d_probes, 64, "sh", c)
    rec = torch.full((3, 32), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.neb_gi_bake_probes_tail(ctx, C.c_void_p(d_probes.data_ptr()), 3, 64, _lib.BAKE_SH, 0, C.byref(c), None, C.c_void_p(rec.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert same_bits(records(rec).view(U32), plain_bake.view(U32)) and (plain_bake["sh"][:, 0].max(-1) > 0).all()
    # a grid whose records are all zero: no valid corner anywhere, every gather says NO_PROBE
    g = room_grid(case["scene"], (4, 4, 4))
    empty = ProbeTail(PV.grid_struct(g), torch.zeros((64, 32), dtype=torch.float32, device="cuda"))
    for tail in (empty, ProbeTail(empty.grid, empty.records, torch.zeros((64, 192), dtype=torch.float32, device="cuda"), BIAS, True)):
        got = trace(r, d_rays, c, tail)
        assert same_bits(got[0].view(U32), plain[0].view(U32)) and same_bits(got[1].view(U32), plain[1].view(U32))
        assert not (got[0]["flags"] & T.TAIL).any() and not (got[1]["flags"] & T.TAIL).any()
        assert same_bits(baked(r, d_probes, 64, "sh", c, tail).view(U32), plain_bake.view(U32))
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3: closed form
# ------------------------------------------------------------------------------------------------
def test_without_light_the_radiance_is_the_tail_of_a_constant_grid_in_closed_form(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    rays = Q.scattered_rays(*Q.scene_box(case["scene"]), Q.N_RAYS, np.random.default_rng(7))  # (the `scattered` set of tests/ray_query_ref.py)
    c = P.constants(2)
    c.sunLightRadiance[:] = (0.0, 0.0, 0.0)
    c.skyColor[:] = (0.0, 0.0, 0.0)
    g = room_grid(case["scene"], (4, 4, 4))
    rec = np.zeros(64, B.RECORD)
    rec["sh"][:, 0], rec["samples"], rec["hits"] = (1.0, 0.5, 0.25), 64, 64
    tail = ProbeTail(PV.grid_struct(g), records_on_device(rec), frame_weight=False)
    paths, vert = trace(r, rays, c, tail)
    surf = shade_rays(r, rays, "surface")
    gat = gather_on(r, tail)(T.points(surf, rays[:, 4:7]))
    material = (surf["flags"] & _lib.HIT_MATERIAL) != 0
    assert not (gat["flags"][material] & T.UNANSWERED).any()
    vertex = np.zeros(len(rays), P.VERTEX)
    vertex["throughput"] = 1.0
    want = T.tail32(vertex, surf, gat["irradiance"])[0]
    assert same_bits(paths["radiance"][material].view(U32), want[material].view(U32))
    assert np.array_equal((paths["flags"] & T.TAIL) != 0, material) and np.array_equal((vert["flags"][:, 0] & T.TAIL) != 0, material)
    assert not paths["radiance"][~material].view(U32).any()
    lit = paths["radiance"][material]
    # E of a constant grid is A_0 Y_00 sh[0] = pi * 0.282095 * (1, 0.5, 0.25) for every normal; the tail is albedo (1 - metalness) E / pi
    k = surf["albedo"][material].astype(F64) * (1.0 - surf["metalness"][material].astype(F64))[:, None]
    assert np.abs(lit - k * 0.282095 * np.array([1.0, 0.5, 0.25])).max() < 1e-5 and lit.max() > 0.05 and material.sum() > 2000
    backface = material & ((surf["flags"] & _lib.HIT_BACKFACE) != 0)
    print(f"[closed form] {int(material.sum())} of {len(rays)} rays end in the grid, {int(backface.sum())} of them on a back face; largest tail {lit.max():.3f}")
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 4: the general case
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("dims", [(2, 2, 2), (4, 4, 4)])
def test_the_general_case_under_the_judge(cases, dims, exact):
    case = cases["room, extras"]
    r = state_renderer(case, bool(exact))
    vol = room_volume(r, case["scene"], dims)
    rays = pool(case["scene"])
    shade, pd64 = (lambda x: shade_rays(r, x, "surface")), pd64_on(case)
    flagged = worst = turned = 0
    for K in (2, 3, 8):
        c = P.constants(K)
        for n in COUNTS:
            d_rays = on_device(rays[:n])
            plain = trace(r, d_rays, c)
            for visible in (False, True):
                for weight in (False, True):
                    tail = tail_of(vol, visible, weight)
                    got = trace(r, d_rays, c, tail)
                    name = f"dims {dims} / exact {exact} / K {K} / n {n} / visible {visible} / weight {weight}"
                    verdict = T.judge(plain, got, K, weight, shade, gather_on(r, tail), name, pd64 if weight and n == 4097 else None)  # (rays[:n] are prefixes of that set)
                    assert same_bits(got[0].view(U32), trace(r, d_rays, c, tail, vertices=False)[0].view(U32)), name  # (`out` does not depend on `vertices`)
                    if n == 4097:
                        assert verdict["flagged"] > (400 if K < 8 else 100), name
                        flagged += verdict["flagged"]
                        worst = max(worst, verdict["pdiff"])
                        a = verdict["answered"]
                        turned += int(((verdict["surface"]["flags"][a] & _lib.HIT_BACKFACE) != 0).sum())
                        cells = np.unique(verdict["gather"]["cell"][a])
                        assert len(cells) == 1 if dims == (2, 2, 2) else len(cells) > 8, name  # (the wave-uniform route / the per-lane route)
    print(f"[general / dims {dims} / exact {exact}] {flagged} flagged vertices at n = 4097, {turned} on a back face; largest pdiff error {worst:.3e} / {T.PDIFF_TOL:.1e}")
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 5: the bake is the reduction of the path query
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("what", tuple(B.WHAT))
def test_bake_is_the_reduction_of_trace_paths_with_the_tail_bit_for_bit(cases, what, exact):
    case = cases["room, extras"]
    r = state_renderer(case, bool(exact))
    vol = room_volume(r, case["scene"], (4, 4, 4))
    pr = probe_set(case["scene"], 5)
    d_probes = on_device(pr)
    for S in (64, 256):
        for K, visible, weight in ((2, False, True), (2, True, True), (3, True, False), (8, False, True)):
            c, tail = P.constants(K), tail_of(vol, visible, weight)
            got = baked(r, d_probes, S, what, c, tail)
            d_rays = r.probe_rays(d_probes, S, what, frame_index=int(c.frameIndex))
            paths = trace(r, d_rays, c, tail, vertices=False)[0]
            want = B.bake_ref(paths, d_rays.cpu().numpy(), S, what)
            assert same_bits(got.view(U32), want.view(U32)), (what, exact, S, K, visible, weight)
            plain = baked(r, d_probes, S, what, c)
            for f in ("samples", "hits", "backfaces", "segments", "flags"):
                assert np.array_equal(got[f], plain[f]), f
            assert (paths["flags"] & T.TAIL).mean() > (0.3 if K < 8 else 0.02) and not same_bits(got.view(U32), plain.view(U32))
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 6, 7: determinism and monotonicity
# ------------------------------------------------------------------------------------------------
def test_sorted_a_second_call_and_a_probe_alone_give_the_same_bits(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    vol = room_volume(r, case["scene"], (4, 4, 4))
    rays = pool(case["scene"])
    for K, visible in ((2, True), (8, False)):
        c, tail = P.constants(K), tail_of(vol, visible)
        for n in COUNTS:
            a, av = trace(r, rays[:n], c, tail)
            b, bv = trace(r, rays[:n], c, tail, sort=True)
            again, againv = trace(r, rays[:n], c, tail)
            assert same_bits(a.view(U32), b.view(U32)) and same_bits(av.view(U32), bv.view(U32)) and same_bits(a.view(U32), again.view(U32)) \
                and same_bits(av.view(U32), againv.view(U32)), (K, n)
        assert (a["flags"] & T.TAIL).any()
    pr = probe_set(case["scene"], 9)
    c, tail = P.constants(3), tail_of(vol, True)
    whole = baked(r, on_device(pr), 128, "sh", c, tail)
    assert same_bits(whole.view(U32), baked(r, on_device(pr), 128, "sh", c, tail).view(U32))
    assert same_bits(whole[:1].view(U32), baked(r, on_device(pr[:1]), 128, "sh", c, tail).view(U32))  # (probe 0: a sample's index depends on the probe's place)
    r.destroy()


@pytest.mark.parametrize("what", tuple(B.WHAT))
def test_a_tail_only_adds_light(cases, what):
    """With the same frameIndex the paths are the plain bake's; every tail is >= 0 (k >= 0, E >= 0) and float addition is monotone in
    each operand, in the path's sum, in the butterfly and in the running total; the basis word Y00 and `scale` are positive constants.
    So band 0 -- under "irradiance" the irradiance itself -- cannot fall."""
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    vol = room_volume(r, case["scene"], (4, 4, 4))
    pr = probe_set(case["scene"], 12)
    pr[4, 0], pr[9, 7] = np.nan, 0.0  # two probes that are not baked
    d = on_device(pr)
    for K in (2, 3):
        plain = baked(r, d, 128, what, P.constants(K))
        for visible in (False, True):
            got = baked(r, d, 128, what, P.constants(K), tail_of(vol, visible))
            assert (got["sh"][:, 0] >= plain["sh"][:, 0]).all() and (got["sh"][:, 0] > plain["sh"][:, 0]).any(-1).sum() >= 6
            assert same_bits(got[[4, 9]].view(U32), plain[[4, 9]].view(U32)) and (got["flags"][[4, 9]] == _lib.PROBE_NOT_BAKED).all()
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 8: the feedback loop converges toward the library's own deep paths
# ------------------------------------------------------------------------------------------------
def test_six_rounds_of_feedback_move_a_two_vertex_bake_toward_eight_vertices(cases):
    case = cases["room, extras"]
    sc = clone(case["scene"])
    r = _renderer(sc, cornell_camera(), 64, 64, sun_table=0, hits=False, exact=False)
    r.begin_frame(RenderInfo(scene=sc, camera=cornell_camera(), frame_index=2))
    r.submit_commands_gbuffer()
    pts = r.gbuffer_points()
    vol = room_volume(r, sc, (4, 4, 4))
    S = 1024
    rounds = [enqueue_bake(r, vol["probes"], S, "sh", P.constants(2, frame_index=21))]
    for j in range(6):  # (no host wait anywhere in the loop: every call is ordered on the stream)
        rounds.append(tail_bake(r, vol["probes"], S, "sh", P.constants(2, frame_index=21), tail_of(vol, True, True, records=rounds[-1])))
    deep = enqueue_bake(r, vol["probes"], S, "sh", P.constants(8, frame_index=21))
    deep2 = enqueue_bake(r, vol["probes"], S, "sh", P.constants(8, frame_index=22))

    def E(rec):
        res = r.gather_probes(vol["grid"], rec, pts, visibility=vol["maps"], normal_bias=BIAS)
        torch.cuda.synchronize()
        return gathered(res["records"])
    ref = E(deep)
    ok = (ref["flags"] & T.UNANSWERED) == 0
    d = lambda rec: float(np.linalg.norm(E(rec)["irradiance"][ok].astype(F64) - ref["irradiance"][ok]) / np.linalg.norm(ref["irradiance"][ok].astype(F64)))  # noqa: E731
    dist, floor = [d(x) for x in rounds], d(deep2)
    print("[convergence] relative L2 against the K = 8 bake over", int(ok.sum()), "pixels: " + " ".join(f"R{j} {v:.4f}" for j, v in enumerate(dist))
          + f"; noise floor (another frameIndex) {floor:.4f}")
    assert ok.sum() > 1000 and dist[6] < dist[0]
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 9: ordering, and the frame left alone
# ------------------------------------------------------------------------------------------------
def test_bake_accumulate_tail_bake_back_to_back_on_one_stream(cases):
    case = cases["room, extras"]
    r = state_renderer(case, exact=False)
    vol = room_volume(r, case["scene"], (4, 4, 4))
    c1, c2, c3 = (P.constants(2, frame_index=f) for f in (31, 32, 33))

    def loop(stream, wait):
        sync = torch.cuda.synchronize if wait else (lambda: None)
        acc = enqueue_bake(r, vol["probes"], 256, "sh", c1, stream=stream)
        sync()
        add = enqueue_bake(r, vol["probes"], 256, "sh", c2, stream=stream)
        sync()
        r.accumulate_probes(acc, add, stream=None if stream is None else stream.cuda_stream)
        sync()
        out = tail_bake(r, vol["probes"], 256, "sh", c3, tail_of(vol, True, True, records=acc), stream=stream)
        torch.cuda.synchronize()
        return records(out)
    want = loop(None, True)
    got = loop(torch.cuda.Stream(), False)
    assert same_bits(got.view(U32), want.view(U32)) and (want["sh"][:, 0].max(-1) > 0).all()
    r.destroy()


def test_a_tail_bake_runs_behind_an_update_on_another_stream():
    sc0, updates = V.room_updates()
    _, _, (indices, moved), s1 = updates[0]  # the boxes rotated
    r = renderer(clone(sc0), exact=False)
    vol = room_volume(r, sc0, (4, 4, 4))
    pr = on_device(np.tile(probe_set(sc0, 16), (8, 1)))  # (a bake long enough for an update to overtake, if it could)
    c, tail = P.constants(3), tail_of(vol, True)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    still = baked(r, pr, 256, "sh", c, tail)
    r.update_transforms(indices, moved, stream=a.cuda_stream)
    out = tail_bake(r, pr, 256, "sh", c, tail, stream=b)  # no host synchronisation in between
    torch.cuda.synchronize()
    settled = baked(r, pr, 256, "sh", c, tail)
    assert same_bits(records(out).view(U32), settled.view(U32)) and not same_bits(settled.view(U32), still.view(U32))
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
    vol = room_volume(r, sc, (4, 4, 4))
    count, trav, table, plane = snapshot()  # (the plain bakes above are known to leave them alone; the tail calls are what is asked)
    rays = on_device(pool(sc, 4097))
    for visible in (False, True):
        tail = tail_of(vol, visible)
        paths = trace(r, rays, P.constants(8, frame_index=9), tail, sort=visible)[0]
        rec = baked(r, vol["probes"], 64, "sh", P.constants(2), tail)
        assert (paths["flags"] & T.TAIL).any() and (rec["sh"][:, 0].max(-1) > 0).all()
    count2, trav2, table2, plane2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(plane2, plane)
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 10: refusals and the mirror
# ------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_name_the_cause(cases):
    case = cases["room"]
    r = state_renderer(case, exact=False)
    lib, ctx = r._lib, r._ctx
    g = room_grid(case["scene"], (4, 4, 4))
    m, n, S, K = 64, 65, 64, 3
    c = P.constants(K)
    d_rec = records_on_device(PV.random_records(g))
    d_maps = torch.ones((m, 192), dtype=torch.float32, device="cuda")
    # the call's own buffers 64 KiB apart in one allocation: a grid's records (8 KiB) or maps (48 KiB) laid over one of them reach no other
    arena = torch.full((5 * 16384,), FILL, dtype=torch.float32, device="cuda")

    def carve(k, *shape):
        return arena[k * 16384:k * 16384 + int(np.prod(shape))].view(*shape)
    out, vert = carve(0, n + 1, 8), carve(1, n + 1, K - 1, 24)
    rec_out = carve(2, m, 32)  # (as large as a grid's records: a bake in place is one of the cases)
    d_rays, d_probes = carve(3, n, 8), carve(4, 5, 8)
    d_rays.copy_(on_device(pool(case["scene"], n)))
    d_probes.copy_(on_device(probe_set(case["scene"], 5)))
    host_mem = torch.empty((m * 192 + 16,), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    end = block.data_ptr() + block.numel()
    RE, MA, RA, PR, OU, VE, RO = (t.data_ptr() for t in (d_rec, d_maps, d_rays, d_probes, out, vert, rec_out))

    def desc(grid=None, records=RE, visibility=None, bias=0.0, flags=1):
        return _lib.ProbeTailDesc(PV.grid_struct(g) if grid is None else grid, records, visibility, bias, flags)

    def spoiled(name, index, value):
        s = PV.grid_struct(g)
        if index is None:
            setattr(s, name, value)
        else:
            getattr(s, name)[index] = value
        return s

    def call_trace(d, p_rays=RA, p_out=OU, p_vert=VE):
        return lib.neb_gi_trace_paths_tail(ctx, C.c_void_p(p_rays), n, 0, C.byref(c), C.byref(d), C.c_void_p(p_out), C.c_void_p(p_vert), None)

    def call_bake(d, p_probes=PR, p_out=RO, count=5):
        return lib.neb_gi_bake_probes_tail(ctx, C.c_void_p(p_probes), count, S, _lib.BAKE_SH, 0, C.byref(c), C.byref(d), C.c_void_p(p_out), None)

    def error():
        return lib.neb_last_error(ctx)

    nan, inf = float("nan"), float("inf")
    shared = [("dims of 0", desc(grid=spoiled("dims", 1, 0)), b"dims"), ("negative spacing", desc(grid=spoiled("spacing", 0, -0.5)), b"spacing"),
              ("nan origin", desc(grid=spoiled("origin", 2, nan)), b"origin"), ("backface_limit above 1", desc(grid=spoiled("backface_limit", None, 1.5)), b"backface_limit"),
              ("too many probes", desc(grid=spoiled("dims", 2, 1 << 24)), b"2^24"),
              ("unknown tail flags", desc(flags=2), b"tail flag"), ("unknown tail flags beside a known one", desc(flags=3), b"tail flag"),
              ("null records", desc(records=None), b"null tail records"), ("misaligned records", desc(records=RE + 16), b"misaligned"),
              ("host-memory records", desc(records=host_ptr), b"tail records is not memory"),
              ("records one short of their allocation", desc(records=end - 128 * (m - 1)), b"tail records is not memory"),
              ("misaligned visibility", desc(visibility=MA + 16), b"misaligned"), ("host-memory visibility", desc(visibility=host_ptr), b"tail visibility is not memory"),
              ("visibility one short of its allocation", desc(visibility=end - 768 * (m - 1)), b"tail visibility is not memory"),
              ("nan normal_bias", desc(visibility=MA, bias=nan), b"normal_bias"), ("negative normal_bias", desc(visibility=MA, bias=-0.01), b"normal_bias"),
              ("infinite normal_bias", desc(visibility=MA, bias=inf), b"normal_bias")]
    refused_trace = [(what, (d,), word) for what, d, word in shared] + [
        ("records are out", (desc(records=OU),), b"tail records overlap out"), ("records inside vertices", (desc(records=VE + 96),), b"tail records overlap vertices"),
        ("records are the rays", (desc(records=RA),), b"tail records overlap rays"), ("visibility is out", (desc(visibility=OU),), b"tail visibility overlaps out"),
        ("visibility inside vertices", (desc(visibility=VE + 96),), b"tail visibility overlaps vertices"),
        ("visibility is the rays", (desc(visibility=RA),), b"tail visibility overlaps rays")]
    refused_bake = [(what, (d,), word) for what, d, word in shared] + [
        ("a bake in place", (desc(records=RO), PR, RO, m), b"tail records overlap out"), ("records are the probes", (desc(records=PR),), b"tail records overlap probes"),
        ("out ends inside the records", (desc(), PR, RE - 128, 2), b"tail records overlap out"), ("visibility is out", (desc(visibility=RO),), b"tail visibility overlaps out"),
        ("visibility is the probes", (desc(visibility=PR),), b"tail visibility overlaps probes")]
    torch.cuda.synchronize()
    for name, call, cases_ in (("neb_gi_trace_paths_tail", call_trace, refused_trace), ("neb_gi_bake_probes_tail", call_bake, refused_bake)):
        for what, args, word in cases_:
            assert call(*args) == -1, (name, what, error())
            assert name.encode() in error() and word in error(), (name, what, error())
    # the plain call's refusals come first, under the plain call's name
    bad = P.constants(9)
    assert lib.neb_gi_trace_paths_tail(ctx, C.c_void_p(RA), n, 0, C.byref(bad), C.byref(desc()), C.c_void_p(OU), C.c_void_p(VE), None) == -1
    assert b"neb_gi_trace_paths:" in error() and b"maxPathVertices" in error()
    assert lib.neb_gi_bake_probes_tail(ctx, C.c_void_p(PR), 5, 65, _lib.BAKE_SH, 0, C.byref(c), C.byref(desc()), C.c_void_p(RO), None) == -1
    assert b"neb_gi_bake_probes:" in error() and b"samples" in error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(vert).all()) and bool(torch.isnan(rec_out).all()), "a refused call wrote something"
    # n == 0 succeeds and looks at nothing of the tail; and the same context answers
    assert lib.neb_gi_trace_paths_tail(ctx, None, 0, 0, C.byref(c), C.byref(desc(records=None)), None, None, None) == 0
    assert call_trace(desc(visibility=MA, bias=BIAS)) == 0 and call_bake(desc(visibility=MA, bias=BIAS)) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:n, 0:4]).any()) and bool(torch.isnan(out[n]).all()) and bool(torch.isnan(vert[n]).all())  # (radiance and t: a miss's ids are all ones)
    assert not bool(torch.isnan(rec_out[:5, 0:27]).any()) and bool(torch.isnan(rec_out[5:]).all())
    assert (paths_to_host((out[:n], None))[0]["flags"] & T.TAIL).any()
    r.destroy()


def test_the_python_mirror_checks_its_arguments(cases):
    case = cases["room"]
    r = state_renderer(case, exact=False)
    g = room_grid(case["scene"], (4, 4, 4))
    grid = PV.grid_struct(g)
    rec, maps = records_on_device(PV.random_records(g)), torch.ones((64, 192), dtype=torch.float32, device="cuda")
    rays, probes = on_device(pool(case["scene"], 10)), on_device(probe_set(case["scene"], 64))
    out = torch.empty((64, 32), dtype=torch.float32, device="cuda")
    bad_tails = (g, (grid, rec), ProbeTail(g, rec), ProbeTail(grid, rec[:63]), ProbeTail(grid, rec.cpu()), ProbeTail(grid, rec.double()), ProbeTail(grid, rec, maps[:63]),
                 ProbeTail(grid, rec, maps.cpu()), ProbeTail(grid, rec, maps, -1.0), ProbeTail(grid, rec, maps, float("nan")), ProbeTail(grid, rec, None, 0.5))
    for tail in bad_tails:
        with pytest.raises(NebError):
            r.trace_paths(rays, constants=P.constants(3), tail=tail)
        with pytest.raises(NebError):
            r.bake_probes(probes, 64, "sh", constants=P.constants(2), tail=tail)
    with pytest.raises(NebError, match="overlaps out"):
        r.bake_probes(probes, 64, "sh", constants=P.constants(2), out=out, tail=ProbeTail(grid, out))  # the in-place hazard of a feedback loop
    with pytest.raises(NebError, match="overlaps out"):
        r.bake_probes(probes, 64, "sh", constants=P.constants(2), out=out, tail=ProbeTail(grid, out, maps, BIAS))
    res = r.trace_paths(rays, constants=P.constants(3), vertices=True, tail=ProbeTail(grid, rec, maps, BIAS, frame_weight=False))
    torch.cuda.synchronize()
    assert bool((res["flags"] & _lib.PATH_TAIL).any()) and bool((res["vertex_flags"][:, 1] & _lib.PATH_TAIL).any()) and not bool((res["vertex_flags"][:, 0] & _lib.PATH_TAIL).any())
    assert not bool(res["pdiff"][:, 1].any())  # (no frame weight: the terminal vertex records no pdiff)
    res = r.bake_probes(probes, 64, "sh", constants=P.constants(2), out=out, tail=ProbeTail(grid, rec))
    torch.cuda.synchronize()
    assert res["records"] is out and bool((res["samples"] == 64).all())
    r.destroy()
