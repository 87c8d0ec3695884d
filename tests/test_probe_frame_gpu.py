"""neb_gbuffer_points / neb_gi_probe_indirect on the device: the points against the host's decode bit for bit; the
indirect term against tests/probe_frame_ref.py bit for bit, E being the device's own gather of those points, on the room's G-buffer
and on synthetic planes of every wave shape; row ranges and a row-strip context; the frame weight against float64; the closed form; a
probe-lit frame against traced ones; the frame left alone, stream order, refusals and the Python mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

import path_ref as P
import probe_frame_ref as PF
import probe_ref as B
import probe_volume_ref as PV
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer, RenderInfo
from nebulae_amd.svgf import (PLANE_ALBEDO, PLANE_DEPTH, PLANE_GEOMETRY, PLANE_LDR, PLANE_MOMENTS, PLANE_NORMAL, PLANE_RADIANCE, PLANE_ROUGH_METAL,
                              PLANE_SCRATCH, PLANE_VARIANCE, PLANE_WORLDPOS, NebError)
from oracle import gi_np
from test_probe_gpu import FREE_POINT, cases, enqueue_bake, records  # noqa: F401  (cases: the room fixture of the bake's tests)
from test_probe_volume_gpu import gathered, records_on_device, room_grid
from test_ray_query_gpu import same_bits
from test_refit_gpu import _renderer, clone, cornell_camera, frame

pytestmark = pytest.mark.gpu

F, F64, U32 = np.float32, np.float64, np.uint32
W, H = PF.SIZES[0]
LIT = dict({kind: 1000 for kind in PF.KINDS}, room=600)  # pixels that are no sky pixels, at least (the room fills a third of its frame)
GBUFFER = (("depth", PLANE_DEPTH, -1), ("normal", PLANE_NORMAL, -1), ("world_pos", PLANE_WORLDPOS, 0), ("albedo", PLANE_ALBEDO, 0),
           ("rough_metal", PLANE_ROUGH_METAL, 0))


def camera():
    cam = cornell_camera()
    cam.eye[:] = PF.CAMERA
    return cam


def bare(w, h, **init):
    """a renderer without a scene, inside a frame: neither call needs a scene"""
    r = DeferredRenderer()
    r.init(w, h, **init)
    r.begin_frame(RenderInfo(scene=None, camera=camera(), frame_index=1))
    return r


def upload_gbuffer(r, planes):
    lo, hi = r.svgf.row_begin, r.svgf.row_end
    for name, plane, slot in GBUFFER:
        r.svgf.upload(plane, slot, planes[name][lo:hi])


def download_gbuffer(r):
    return {name: r.svgf.download(plane, slot) for name, plane, slot in GBUFFER}


def seed(r, radiance):
    r.svgf.upload(PLANE_RADIANCE, -1, radiance[r.svgf.row_begin:r.svgf.row_end])


def radiance_of(r):
    torch.cuda.synchronize()
    return r.svgf.download(PLANE_RADIANCE)


def device_gather(r, g, d_rec, rows=None):
    """the gather of the frame's own points, both calls on the device -> (points [n, 8] float32 on the host, the GATHER-like dict)"""
    pts = r.gbuffer_points(rows=rows)
    res = r.gather_probes(PV.grid_struct(g), d_rec, pts)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), PV.as_dict(gathered(res["records"]))


def lit(r, g, d_rec, radiance, frame_weight=False, rows=None, stream=None):
    seed(r, radiance)
    r.submit_commands_gi_probes(PV.grid_struct(g), d_rec, frame_weight=frame_weight, rows=rows, stream=stream)
    return radiance_of(r)


@pytest.fixture(scope="module")
def room(cases):
    """the room's G-buffer through neb_gbuffer_raycast at 70 x 45, with its planes on the host"""
    sc = clone(cases["room, extras"]["scene"])
    r = _renderer(sc, cornell_camera(), W, H, sun_table=0, hits=False, exact=False)
    r.begin_frame(RenderInfo(scene=sc, camera=cornell_camera(), frame_index=2))
    r.submit_commands_gbuffer()
    torch.cuda.synchronize()
    yield dict(r=r, scene=sc, planes=download_gbuffer(r))
    r.destroy()


@pytest.fixture(scope="module")
def synthetic():
    """a scene-less renderer per frame size, shared by the tests that upload their planes"""
    out = {size: bare(*size) for size in PF.SIZES}
    yield out
    for r in out.values():
        r.destroy()


def gbuffers(room, synthetic, kind, dims):
    """-> (renderer, grid, planes on the host) with the planes in place on the device"""
    if kind == "room":
        return room["r"], room_grid(room["scene"], dims), room["planes"]
    g = PV.gpu_grid(dims)
    planes = PF.synthetic_gbuffer(g, kind, W, H)
    upload_gbuffer(synthetic[(W, H)], planes)
    return synthetic[(W, H)], g, planes


# ------------------------------------------------------------------------------------------------
# 1: the points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("room",) + PF.KINDS)
def test_points_are_the_hosts_decode_bit_for_bit(room, synthetic, kind):
    r, g, planes = gbuffers(room, synthetic, kind, (5, 4, 3))
    pts = r.gbuffer_points()
    torch.cuda.synchronize()
    got = pts.cpu().numpy().reshape(H, W, 8)
    sky = PF.sky(planes)
    assert same_bits(got[~sky][:, 0:3], planes["world_pos"][~sky][:, 0:3].astype(F))  # the three fp16 words, converted
    with np.errstate(all="ignore"):
        want_n = gi_np.oct16_fast_unpack(planes["normal"][..., 2:4].astype(F))  # the oracle's restatement of oct_unpack
    assert same_bits(got[~sky][:, 4:7], want_n[~sky])
    assert not got[sky][:, [0, 1, 2, 4, 5, 6]].view(U32).any()  # sky: position 0, normal 0 -- all bits
    assert same_bits(got[..., 3], np.full((H, W), 0.01, F)) and same_bits(got[..., 7], np.full((H, W), np.inf, F))
    assert same_bits(got.reshape(-1, 8), PF.points32(planes))
    assert (~sky).sum() > LIT[kind] and (kind != "special" or sky.sum() > 100)
    rows = r.gbuffer_points(rows=(3, 21))  # begins and ends in mid-tile
    torch.cuda.synchronize()
    assert rows.shape == (18 * W, 8) and same_bits(rows.cpu().numpy(), got[3:21].reshape(-1, 8))
    # ... and the buffer is what the gather takes: a sky pixel is NOT_GATHERED with no special case anywhere
    _, res = device_gather(r, g, records_on_device(PV.random_records(g)))
    assert ((res["flags"].reshape(H, W)[sky] == _lib.GATHER_NOT_GATHERED)).all() and PF.stored(res).sum() > LIT[kind] // 2


# ------------------------------------------------------------------------------------------------
# 2: the identity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("room",) + PF.KINDS)
def test_the_indirect_term_is_the_float32_statement_bit_for_bit(room, synthetic, kind):
    rad = PF.random_radiance(W, H)
    for dims in PF.GRIDS:
        r, g, planes = gbuffers(room, synthetic, kind, dims)
        d_rec = records_on_device(PV.random_records(g))
        _, res = device_gather(r, g, d_rec)
        got = lit(r, g, d_rec, rad)
        n = PF.judge_identity(got, rad, planes, res, f"{kind} / {dims}")
        flags = res["flags"]
        print(f"[identity / {kind} / {dims}] {n} of {W * H} pixels stored to; {int(((flags & _lib.GATHER_NO_PROBE) != 0).sum())} without a probe, "
              f"{int(((flags & _lib.GATHER_NOT_GATHERED) != 0).sum())} not gathered, {int(((flags & _lib.GATHER_CLAMPED) != 0).sum())} clamped")
        assert n > LIT[kind] // 2 and not same_bits(got, rad)
        if kind == "special":
            assert ((flags & _lib.GATHER_NOT_GATHERED) != 0).sum() > 300 and (dims == (1, 1, 1) or ((flags & _lib.GATHER_NO_PROBE) != 0).sum() > 100)
        assert same_bits(lit(r, g, d_rec, rad), got)  # a second call on the re-seeded plane


@pytest.mark.parametrize("size", PF.SIZES[1:])
def test_one_tile_and_one_pixel(synthetic, size):
    w, h = size
    r = synthetic[size]
    rad = PF.random_radiance(w, h)
    for dims in PF.GRIDS:
        g = PV.gpu_grid(dims)
        d_rec = records_on_device(PV.random_records(g))
        for kind in PF.KINDS:
            planes = PF.synthetic_gbuffer(g, kind, w, h)
            if size == (1, 1):
                planes["depth"] |= U32(1 << 24)  # (the one pixel is no sky pixel)
            upload_gbuffer(r, planes)
            pts, res = device_gather(r, g, d_rec)
            assert same_bits(pts, PF.points32(planes))
            PF.judge_identity(lit(r, g, d_rec, rad), rad, planes, res, f"{size} / {kind} / {dims}")
            got = lit(r, g, d_rec, rad, frame_weight=True)
            PF.judge_weighted(got, rad, planes, res, PF.CAMERA, f"{size} / {kind} / {dims}, weighted")
    sky = PF.synthetic_gbuffer(g, "uniform", w, h)
    sky["depth"] &= U32(0x00FFFFFF)
    upload_gbuffer(r, sky)
    assert same_bits(lit(r, g, d_rec, rad, frame_weight=True), rad)  # a frame of sky: nothing is stored


# ------------------------------------------------------------------------------------------------
# 3: rows
# ------------------------------------------------------------------------------------------------
def test_row_ranges_and_a_row_strip_context(synthetic):
    r = synthetic[(W, H)]
    g = PV.gpu_grid((5, 4, 3))
    d_rec = records_on_device(PV.random_records(g))
    planes = PF.synthetic_gbuffer(g, "special", W, H)
    upload_gbuffer(r, planes)
    rad = PF.random_radiance(W, H)
    grid = PV.grid_struct(g)
    for weight in (False, True):
        whole = lit(r, g, d_rec, rad, frame_weight=weight)
        seed(r, rad)
        for rows in ((21, H), (0, 3), (3, 21)):  # complementary ranges that begin and end in mid-tile, in any order
            r.submit_commands_gi_probes(grid, d_rec, frame_weight=weight, rows=rows)
        assert same_bits(radiance_of(r), whole)
        part = lit(r, g, d_rec, rad, frame_weight=weight, rows=(3, 21))
        assert same_bits(part[3:21], whole[3:21]) and same_bits(part[:3], rad[:3]) and same_bits(part[21:], rad[21:])
        one = lit(r, g, d_rec, rad, frame_weight=weight, rows=(H - 1, H))
        assert same_bits(one[H - 1:], whole[H - 1:]) and same_bits(one[:H - 1], rad[:H - 1])
        strip = bare(W, H, row_begin=5, row_end=30)  # a row-strip context: rows 5 .. 29 are all it holds
        upload_gbuffer(strip, planes)
        assert same_bits(lit(strip, g, d_rec, rad, frame_weight=weight), whole[5:30])
        half = lit(strip, g, d_rec, rad, frame_weight=weight, rows=(9, 22))
        assert same_bits(half[4:17], whole[9:22]) and same_bits(half[:4], rad[5:9]) and same_bits(half[17:], rad[22:30])
        pts = strip.gbuffer_points(rows=(9, 22))
        torch.cuda.synchronize()
        assert same_bits(pts.cpu().numpy(), PF.points32(planes).reshape(H, W, 8)[9:22].reshape(-1, 8))
        strip.destroy()


# ------------------------------------------------------------------------------------------------
# 4: the frame weight
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("room",) + PF.KINDS)
def test_the_frame_weight_matches_the_float64_statement(room, synthetic, kind):
    rad = PF.random_radiance(W, H)
    worst = 0.0
    for dims in PF.GRIDS:
        r, g, planes = gbuffers(room, synthetic, kind, dims)
        eye = tuple(r.info.camera.eye)
        d_rec = records_on_device(PV.random_records(g))
        _, res = device_gather(r, g, d_rec)
        got = lit(r, g, d_rec, rad, frame_weight=True)
        worst = max(worst, PF.judge_weighted(got, rad, planes, res, eye, f"{kind} / {dims}"))
        plain = lit(r, g, d_rec, rad)
        metal = (planes["rough_metal"][..., 1] == 1.0) & PF.stored(res).reshape(H, W)
        assert np.array_equal(got[metal], rad[metal]) and (kind == "room" or metal.sum() > 100)  # metalness 1 adds 0
        gain, gain0 = got[..., 0:3].astype(F64) - rad[..., 0:3], plain[..., 0:3].astype(F64) - rad[..., 0:3]
        assert (gain >= gain0 - 1e-5).all() and gain.sum() > 1.05 * gain0.sum()  # the factor lies in 1.1 .. 1.9
    print(f"[frame weight / {kind}] largest error {worst:.3e} / {PF.TOL['frame_weight']:.1e}")


# ------------------------------------------------------------------------------------------------
# 5: the closed form
# ------------------------------------------------------------------------------------------------
def test_free_space_records_light_every_pixel_with_its_albedo_times_the_sky(cases, synthetic):
    """the records test_free_space_records_gather_to_pi_times_the_sky gathers to pi * sky: every pixel that is no sky pixel gains
    albedo * (1 - metalness) * sky, within that test's bar on E carried through k / pi.  A lost 1 / pi or (1 - metalness) misses it."""
    case = cases["room, extras"]
    baker = _renderer(clone(case["scene"]), cornell_camera(), 64, 48, sun_table=0, hits=False, exact=False)
    h = 2.0 ** -14
    g = PV.grid(np.array(FREE_POINT) - 0.5 * h, (h, h, h), (2, 2, 2), 0.25)
    c = P.constants(5)
    sky_color = np.array(list(c.skyColor), F64)
    _, d_probes = baker.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=0.0, tmax=9e-4)
    out = enqueue_bake(baker, d_probes, 4096, "sh", c)
    torch.cuda.synchronize()
    rec = records(out)
    assert (rec["hits"] == 0).all() and (rec["samples"] == 4096).all() and sky_color.max() > 0
    r = synthetic[(W, H)]
    planes = PF.synthetic_gbuffer(PV.gpu_grid((5, 4, 3)), "permuted", W, H)  # (any finite positions: outside this grid they are clamped to it)
    planes["depth"][::7, ::5] &= U32(0x00FFFFFF)
    upload_gbuffer(r, planes)
    pts, res = device_gather(r, g, out)
    zero = np.zeros((H, W, 4), F)
    got = lit(r, g, out, zero)
    use = ~PF.sky(planes)
    assert np.array_equal(PF.stored(res).reshape(H, W), use) and not got[~use].view(U32).any() and not got[..., 3].view(U32).any()
    sh = rec["sh"].astype(F64)
    k00 = float(B.K00)
    off = np.abs(sh - np.concatenate([(4.0 * np.pi * k00 * sky_color)[None], np.zeros((8, 3))])[None]).max(0)  # [9, 3]
    Y = np.abs(B.sh_basis64(pts[:, 4:7].astype(F64)[use.reshape(-1)]))
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    bar_E = (Y * A) @ off + PV.TOL["gather"] * np.maximum(1.0, np.pi * sky_color) + np.pi * sky_color * abs(4.0 * np.pi * k00 * k00 - 1.0)
    k = PF.diffuse_k(planes, F64)[use]
    want = k * sky_color
    bar = k * bar_E / np.pi + 4.0 * 2.0 ** -24 * want  # (and the three roundings of the term, with one to spare)
    err = np.abs(got[use][:, 0:3].astype(F64) - want)
    print(f"[closed form] largest error {err.max():.3e}; its bar {bar[np.unravel_index(err.argmax(), err.shape)]:.3e}; gains up to {want.max():.3f}")
    assert (err <= bar).all() and (bar.max(-1) < 0.5 * want.max(-1))[k.min(-1) > 0.05].all()  # (a bar a lost 1 / pi would miss)
    baker.destroy()


# ------------------------------------------------------------------------------------------------
# 6: a probe-lit frame
# ------------------------------------------------------------------------------------------------
def test_a_probe_lit_frame_is_nearer_to_the_converged_traced_frame_than_one_sample_is(cases):
    """Measured on MI355X: see the numbers there.  A sanity ordering, not a tuned bar."""
    sc = clone(cases["room, extras"]["scene"])
    cam = cornell_camera()
    r = _renderer(sc, cam, W, H, sun_table=0, hits=False, exact=False)
    r.gi_ui.max_path_vertices = 3  # (what the probes are baked with)
    g = room_grid(sc)
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    torch.cuda.synchronize()
    acc = enqueue_bake(r, d_probes, 64, "sh", P.constants(3, frame_index=21))
    for k in (1, 2):
        r.accumulate_probes(acc, enqueue_bake(r, d_probes, 64, "sh", P.constants(3, frame_index=21 + k)))

    def begin(f):
        r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
        r.submit_commands_gbuffer()
        r.submit_commands_pbr_lighting()

    traced = []
    for f in range(65):
        begin(100 + f)
        r.submit_commands_gi_pathtrace()
        traced.append(radiance_of(r)[..., 0:3].astype(F64))
        r.end_frame()
    begin(200)
    direct = radiance_of(r)[..., 0:3].astype(F64)
    r.submit_commands_gi_probes(grid, acc)  # frame_weight=True: the stand-in for submit_commands_gi_pathtrace
    probe_lit = radiance_of(r)
    assert r.submit_commands_svgf_denoising() is True
    denoised = radiance_of(r)
    r.end_frame()
    assert np.isfinite(probe_lit).all() and np.isfinite(denoised).all() and (probe_lit[..., 0:3] >= direct - 1e-6).all()
    mean, single = np.mean(traced[:64], axis=0), traced[64]

    def distance(a, ref):
        return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))
    d_probe, d_single = distance(probe_lit[..., 0:3].astype(F64), mean), distance(single, mean)
    i_probe, i_single = distance(probe_lit[..., 0:3] - direct, mean - direct), distance(single - direct, mean - direct)
    print(f"[probe-lit frame] relative L2 to the mean of 64 one-sample frames: probe-lit {d_probe:.4f}, one sample {d_single:.4f}; "
          f"of the indirect term alone: probe-lit {i_probe:.4f}, one sample {i_single:.4f}")
    assert (mean - direct).max() > 0.05 and d_probe < d_single
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 7 - 10: the frame left alone, stream order, refusals, the mirror
# ------------------------------------------------------------------------------------------------
def test_every_other_plane_the_counters_the_hits_and_the_sun_table_are_untouched(cases):
    case = cases["room"]
    sc, cam = clone(case["scene"]), cornell_camera()
    r = _renderer(sc, cam, 64, 48, sun_table=1, hits=True)
    for f in (2, 3):
        frame(r, sc, cam, f)
    cur = r.svgf.get_current_resource_index()
    others = [(PLANE_RADIANCE, cur ^ 1)] + [(p, s) for p in (PLANE_NORMAL, PLANE_DEPTH, PLANE_MOMENTS) for s in (0, 1)] + [
        (p, 0) for p in (PLANE_VARIANCE, PLANE_SCRATCH, PLANE_ALBEDO, PLANE_ROUGH_METAL, PLANE_WORLDPOS, PLANE_LDR, PLANE_GEOMETRY)]

    def snapshot():
        torch.cuda.synchronize()
        return (r.ray_count(), r.traversal_stats(), r.sun_table_stats(), r.download_hits().copy(), [r.svgf.download(p, s).copy() for p, s in others],
                r.svgf.download(PLANE_RADIANCE).copy())
    count, trav, table, hits, planes, radiance = snapshot()
    assert count > 0 and table["builds"] == 1 and radiance[..., :3].max() > 0.05
    g = room_grid(sc)
    d_rec = records_on_device(PV.random_records(g))
    pts = r.gbuffer_points()
    for weight in (False, True):
        r.submit_commands_gi_probes(PV.grid_struct(g), d_rec, frame_weight=weight)
    r.submit_commands_gi_probes(PV.grid_struct(g), d_rec, rows=(3, 21))
    count2, trav2, table2, hits2, planes2, radiance2 = snapshot()
    assert count2 == count and trav2 == trav and table2 == table and same_bits(hits2, hits)
    for (p, s), a, b in zip(others, planes, planes2):
        assert same_bits(a, b), (p, s)
    assert not same_bits(radiance2, radiance) and same_bits(radiance2[..., 3], radiance[..., 3]) and bool(torch.isfinite(pts[:, 0:7]).all())
    a = frame(r, sc, cam, 4)
    assert r.sun_table_stats()["builds"] == 1 and float(a["radiance"][..., :3].max()) > 0.05
    r.destroy()


def test_bake_accumulate_and_the_indirect_term_on_one_stream_need_no_host_wait(room):
    r, sc = room["r"], room["scene"]
    g = room_grid(sc)
    grid, d_probes = r.probe_grid(g["origin"], g["spacing"], g["dims"], tmin=1e-3)
    rad = PF.random_radiance(W, H)
    cs = [P.constants(3, frame_index=31 + k) for k in (0, 1)]

    def run(stream, wait):
        seed(r, rad)
        torch.cuda.synchronize()
        st = None if stream is None else stream.cuda_stream
        acc = torch.zeros((PV.count(g), 32), dtype=torch.float32, device="cuda")
        for c in cs:
            out = enqueue_bake(r, d_probes, 128, "sh", c, stream=stream)  # (its buffer is full of NaN until the bake has run)
            wait()
            r.accumulate_probes(acc, out, stream=st)
            wait()
        r.submit_commands_gi_probes(grid, acc, frame_weight=True, stream=st)
        return radiance_of(r), acc
    want, acc = run(None, torch.cuda.synchronize)
    got, _ = run(torch.cuda.Stream(), lambda: None)
    assert same_bits(got, want) and not same_bits(want, rad) and (records(acc)["samples"] == 256).all()


def test_refusals_enqueue_nothing_and_name_the_cause(synthetic):
    r = synthetic[(W, H)]
    strip = bare(W, H, row_begin=8, row_end=24)
    lib = r._lib
    g = PV.gpu_grid((5, 4, 3))
    m, n = 60, W * H
    planes = PF.synthetic_gbuffer(g, "permuted", W, H)
    rad = PF.random_radiance(W, H)
    for x in (r, strip):
        upload_gbuffer(x, planes)
        seed(x, rad)
    d_rec = records_on_device(PV.random_records(g))
    points = torch.full((n + 1, 8), float("nan"), dtype=torch.float32, device="cuda")
    host_mem = torch.empty((m * 32 + 16,), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    ok, c = PV.grid_struct(g), r.global_constants()
    radiance_ptr = r.svgf.get_plane(PLANE_RADIANCE)[0]
    worldpos_ptr = r.svgf.get_plane(PLANE_WORLDPOS, 0)[0]
    FW = _lib.INDIRECT_FRAME_WEIGHT

    def spoiled(name, index, value):
        s = PV.grid_struct(g)
        if index is None:
            setattr(s, name, value)
        else:
            getattr(s, name)[index] = value
        return s

    def indirect(x, grid, p_rec, constants, flags, rows=None):
        a = (x._ctx, None if grid is None else C.byref(grid), C.c_void_p(p_rec), None if constants is None else C.byref(constants), flags)
        return lib.neb_gi_probe_indirect(*a, None) if rows is None else lib.neb_gi_probe_indirect_rows(*a, rows[0], rows[1], None)

    def make_points(x, rows, p_points):
        return lib.neb_gbuffer_points(x._ctx, rows[0], rows[1], C.c_void_p(p_points), None)

    RE, PT = d_rec.data_ptr(), points.data_ptr()
    refused_indirect = [
        ("dims of 0", (r, spoiled("dims", 1, 0), RE, c, 0), -1, b"dims"), ("negative spacing", (r, spoiled("spacing", 0, -0.5), RE, c, 0), -1, b"spacing"),
        ("nan origin", (r, spoiled("origin", 2, float("nan")), RE, c, 0), -1, b"origin"),
        ("too many probes", (r, spoiled("dims", 2, (1 << 24) + 1), RE, c, 0), -1, b"2^24"),
        ("backface_limit above 1", (r, spoiled("backface_limit", None, 1.5), RE, c, 0), -1, b"backface_limit"),
        ("null grid", (r, None, RE, c, 0), -1, b"null grid"), ("null records", (r, ok, 0, c, 0), -1, b"null records"),
        ("misaligned records", (r, ok, RE + 16, c, 0), -1, b"misaligned"), ("host-memory records", (r, ok, host_ptr, c, 0), -1, b"records is not memory"),
        ("records one short of their allocation", (r, ok, end - 128 * (m - 1), c, 0), -1, b"records is not memory"),
        ("records inside the radiance plane", (r, ok, radiance_ptr + 128, c, 0), -1, b"overlaps the radiance plane"),
        ("records ending inside the radiance plane", (r, ok, radiance_ptr - 128 * (m - 1), None, 0), -1, b"overlaps the radiance plane"),
        ("an unknown flag bit", (r, ok, RE, c, 2), -1, b"flags"), ("an unknown flag bit beside the known", (r, ok, RE, c, FW | 0x80000000), -1, b"flags"),
        ("the frame weight without constants", (r, ok, RE, None, FW), -1, b"null constants"),
        ("rows past the frame", (r, ok, RE, c, 0, (40, H + 1)), -5, b"rows"), ("no rows", (r, ok, RE, c, 0, (9, 9)), -5, b"rows"),
        ("rows reversed", (r, ok, RE, c, FW, (21, 3)), -5, b"rows"), ("rows before the strip", (strip, ok, RE, c, 0, (7, 20)), -5, b"rows"),
        ("rows past the strip", (strip, ok, RE, c, 0, (8, 25)), -5, b"rows"), ("rows outside the strip", (strip, ok, RE, c, 0, (30, 40)), -5, b"rows")]
    refused_points = [
        ("null points", (r, (0, H), 0), -1, b"null points"), ("misaligned points", (r, (0, H), PT + 8), -1, b"misaligned"),
        ("host-memory points", (r, (0, 1), host_ptr), -1, b"points is not memory"),
        ("points one short of their allocation", (r, (0, H), end - 32 * (n - 1)), -1, b"points is not memory"),
        ("points inside a plane the call reads", (r, (0, 1), worldpos_ptr + 64), -1, b"overlaps"),
        ("rows past the frame", (r, (0, H + 1), PT), -5, b"rows"), ("no rows", (r, (5, 5), PT), -5, b"rows"), ("rows reversed", (r, (21, 3), PT), -5, b"rows"),
        ("rows before the strip", (strip, (7, 20), PT), -5, b"rows"), ("rows past the strip", (strip, (8, 25), PT), -5, b"rows")]
    torch.cuda.synchronize()
    for name, call, refused in (("neb_gi_probe_indirect", indirect, refused_indirect), ("neb_gbuffer_points", make_points, refused_points)):
        for what, args, code, word in refused:
            assert call(*args) == code, (name, what, lib.neb_last_error(args[0]._ctx))
            error = lib.neb_last_error(args[0]._ctx)
            assert name.encode() in error and word in error, (name, what, error)
    torch.cuda.synchronize()
    assert same_bits(radiance_of(r), rad) and same_bits(radiance_of(strip), rad[8:24]) and bool(torch.isnan(points).all()), "a refused call wrote something"
    assert same_bits(download_gbuffer(r)["world_pos"], planes["world_pos"])
    # ... and the same contexts answer: ranges that just fit are accepted, null constants without the flag too
    block[-128 * m:].view(torch.float32).view(m, 32).copy_(d_rec)
    torch.cuda.synchronize()
    _, res = device_gather(r, g, d_rec)
    assert indirect(r, ok, end - 128 * m, None, 0) == 0 and make_points(r, (0, H), PT) == 0 and indirect(strip, ok, RE, c, 0, (8, 24)) == 0
    PF.judge_identity(radiance_of(r), rad, planes, res, "after the refusals")
    assert same_bits(points[:n].cpu().numpy(), PF.points32(planes)) and bool(torch.isnan(points[n]).all())
    assert same_bits(radiance_of(strip), radiance_of(r)[8:24])
    assert make_points(r, (0, H), end - 128 * m - 32 * n) == 0
    torch.cuda.synchronize()
    assert same_bits(block[-(128 * m + 32 * n):-128 * m].cpu().numpy().view(F).reshape(n, 8), PF.points32(planes))
    strip.destroy()


def test_the_python_mirror_checks_its_arguments_and_returns_the_views(synthetic):
    r = synthetic[(W, H)]
    g = PV.gpu_grid((5, 4, 3))
    planes = PF.synthetic_gbuffer(g, "uniform", W, H)
    upload_gbuffer(r, planes)
    seed(r, PF.random_radiance(W, H))
    grid, rec = PV.grid_struct(g), records_on_device(PV.random_records(g))
    for rows in ((0, 0), (5, 3), (0, H + 1), (-1, 4), (3,), 7):
        with pytest.raises(NebError):
            r.gbuffer_points(rows=rows)
        with pytest.raises(NebError):
            r.submit_commands_gi_probes(grid, rec, rows=rows)
    for out in (torch.empty((W * H, 8)), torch.empty((W * H - 1, 8), device="cuda"), torch.empty((W * H, 8), dtype=torch.float64, device="cuda"),
                torch.empty((W * H, 16), device="cuda")[:, ::2]):
        with pytest.raises(NebError):
            r.gbuffer_points(out=out)
    for args in ((g, rec), (grid, rec[:59]), (grid, rec.cpu()), (grid, rec.double()), (grid, rec[:, :31]), (grid, rec[::2])):
        with pytest.raises(NebError):
            r.submit_commands_gi_probes(*args)
    fresh = DeferredRenderer()
    fresh.init(8, 8)
    with pytest.raises(NebError, match="frame"):
        fresh.submit_commands_gi_probes(grid, rec)  # frame_weight needs the frame's camera
    fresh.submit_commands_gi_probes(grid, rec, frame_weight=False)
    fresh.destroy()
    out = torch.full((18 * W, 8), float("nan"), dtype=torch.float32, device="cuda")
    pts = r.gbuffer_points(rows=(3, 21), out=out)
    whole = r.gbuffer_points()
    torch.cuda.synchronize()
    assert pts is out and whole.shape == (W * H, 8) and whole.dtype == torch.float32 and whole.is_cuda
    assert same_bits(out.cpu().numpy(), whole.cpu().numpy().reshape(H, W, 8)[3:21].reshape(-1, 8))
    res = r.gather_probes(grid, rec, whole)  # the tensor is the gather's `points` as it is ...
    assert r.submit_commands_gi_probes(grid, rec) is None and r.submit_commands_gi_probes(grid, rec, frame_weight=False, rows=(3, 21)) is None
    torch.cuda.synchronize()
    assert bool((res["weight"] > 0).any()) and bool(torch.isfinite(r.svgf.plane_tensor(PLANE_RADIANCE)).all())
