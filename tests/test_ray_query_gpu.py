"""neb_gi_cast_rays: the caller's rays from device buffers against the scene the context holds, closest hit and any
hit, sorted or not -- judged against the float64 brute-force caster by tests/ray_query_ref.py (whose judge, tolerances and caps
tests/test_ray_query_cpu.py establishes on the CPU), compared with itself bit for bit where the contract says the bits are equal,
across updates, streams, growing sort scratch, and at its refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_query_ref as Q
import views_ref as V
from motion_ref import NO_SUBMESH
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from test_deform_gpu import update as update_vertices
from test_gi_gpu import scenes
from test_refit_gpu import _renderer, clone, cornell_camera

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
HIT = np.dtype([("t", F), ("u", F), ("v", F), ("geometry", U32), ("primitive", U32), ("reserved", U32, (3,))])
MISS = np.array([(np.inf, 0.0, 0.0, NO_SUBMESH, NO_SUBMESH, (0, 0, 0))], HIT)[0]
W, H = 64, 48  # (the frame's planes play no part)


# ------------------------------------------------------------------------------------------------
def on_device(rays):
    return torch.from_numpy(np.ascontiguousarray(rays, F)).cuda()


def enqueue(r, d_rays, any_hit=False, sort=False, stream=None):
    """one call into a buffer filled with a pattern no answer has -> the output tensor (nothing waits)"""
    n = d_rays.shape[0]
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if any_hit else torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    if stream is not None:  # (the fill above ran on the current stream: ordered on the device, the host waits for nothing)
        stream.wait_stream(torch.cuda.current_stream())
    res = r.cast_rays(d_rays, any_hit=any_hit, sort=sort, out=out, stream=None if stream is None else stream.cuda_stream)
    assert (res["occluded"] if any_hit else res["records"]) is out
    return out


def to_host(out):
    a = out.cpu().numpy()
    return a.view(U32) if a.ndim == 1 else np.ascontiguousarray(a).view(HIT).reshape(-1)


def cast(r, rays, any_hit=False, sort=False):
    d = on_device(rays)
    torch.cuda.synchronize()
    out = enqueue(r, d, any_hit, sort)
    torch.cuda.synchronize()
    return to_host(out)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def room_renderer(sc):
    return _renderer(sc, cornell_camera(), W, H, sun_table=0, hits=False)


@pytest.fixture(scope="module")
def cases():
    """the scene states of tests/ray_query_ref.py with their ray sets and float64 references, computed once and left unchanged"""
    out = {}
    for name, (sc, hidden) in Q.states().items():
        tris = Q.triangles(sc, hidden)
        sets = Q.ray_sets(*Q.scene_box(sc), tris)
        wanted = Q.SETS if name == "room" else ("scattered", "outside")
        out[name] = dict(scene=sc, tris=tris, sets=sets, refs={k: Q.reference(tris, sets[k]) for k in wanted})
    return out


def judged(case, name, hits, occluded, what):
    tris, rays, ref = case["tris"], case["sets"][name], case["refs"][name]
    assert not hits["reserved"].any(), what
    Q.check(Q.judge(tris, rays, ref, {k: hits[k] for k in ("t", "u", "v", "geometry", "primitive")}), what)
    Q.check_any_hit(occluded, ref, what)


# ------------------------------------------------------------------------------------------------
# 1: against float64
# ------------------------------------------------------------------------------------------------
def test_every_set_against_float64(cases):
    """The beamed room (1 246 triangles, split references among them), the five sets, closest hit and any hit through the judge.
    `short` reports misses with t = +inf.  Every set sees hits on at least six of the eight submeshes -- for `short`, whose rays all
    end in front of their surface, the submeshes they were cut short of."""
    case = cases["room"]
    r = room_renderer(clone(case["scene"]))
    refs = r.scene_bytes()["triangles"] // 176
    assert refs > case["scene"].num_triangles  # the tree holds split references
    for name in Q.SETS:
        hits, occ = cast(r, case["sets"][name]), cast(r, case["sets"][name], any_hit=True)
        judged(case, name, hits, occ, f"room / {name}")
        found = hits["geometry"] != NO_SUBMESH
        seen = sorted(set(hits["geometry"][found].tolist()))
        if name == "short":
            was_hit = case["refs"]["scattered"]["hit"]
            assert not found[was_hit].any() and np.isposinf(hits["t"][was_hit]).all() and not occ[was_hit].any()
            assert same_bits(hits[was_hit], np.full(int(was_hit.sum()), MISS, HIT))
            seen = Q.submeshes_seen(name, case["sets"], case["refs"][name], case["tris"])
        print(f"[room / {name}] {int(found.sum())} hits on submeshes {seen}")
        assert len(seen) >= 6, (name, seen)
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 2: sorted == unsorted, bit for bit
# ------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 37]


def test_sorted_equals_unsorted_bit_for_bit_on_the_room(cases):
    """wave boundaries and raysort's 4096-pair tiles; the whole output buffer, reserved words included"""
    case = cases["room"]
    r = room_renderer(clone(case["scene"]))
    pool = np.concatenate([case["sets"][k] for k in ("scattered", "outside", "axis")])
    for n in SIZES:
        for any_hit in (False, True):
            a, b = cast(r, pool[:n], any_hit=any_hit), cast(r, pool[:n], any_hit=any_hit, sort=True)
            assert same_bits(a, b), (n, any_hit)
            written = (a != 0x5A5A5A5A).all() if any_hit else not np.isnan(a["t"]).any()  # (every answer replaced the buffer's fill)
            assert written, (n, any_hit)
    r.destroy()


def test_sorted_equals_unsorted_on_a_deeper_tree_and_any_hit_equals_closest_hit_found():
    make, cam, _, _ = scenes()["atrium_small"]
    sc = make()
    r = _renderer(sc, cam, W, H, sun_table=0, hits=False)
    rays = Q.scattered_rays(*Q.scene_box(sc), 8229, np.random.default_rng(11))
    hits, hits_s = cast(r, rays), cast(r, rays, sort=True)
    occ, occ_s = cast(r, rays, any_hit=True), cast(r, rays, any_hit=True, sort=True)
    assert same_bits(hits, hits_s) and same_bits(occ, occ_s)
    found = hits["geometry"] != NO_SUBMESH
    print(f"[atrium_small] {int(found.sum())} of {len(rays)} rays hit; tree depth {r.bvh_depth()}")
    assert 0.5 * len(rays) < found.sum()
    assert np.array_equal(occ != 0, found)  # the same triangle tests on the same intervals: exact
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 3: rays that cannot be walked
# ------------------------------------------------------------------------------------------------
def test_rays_that_cannot_be_walked_report_a_miss_and_disturb_nobody(cases):
    case = cases["room"]
    r = room_renderer(clone(case["scene"]))
    good = case["sets"]["scattered"].copy()
    n = len(good)
    bad = good.copy()
    kinds = ["zero direction", "nan origin", "infinite direction", "tmin -1", "tmin nan", "tmax == tmin"]
    where = {}
    for base in (0, n - 64):  # one of each kind in the first wave and one in the last
        for k, kind in enumerate(kinds):
            i = base + 5 + 9 * k
            where[i] = kind
            if kind == "zero direction":
                bad[i, 4:7] = 0.0
            elif kind == "nan origin":
                bad[i, 1] = np.nan
            elif kind == "infinite direction":
                bad[i, 5] = np.inf
            elif kind == "tmin -1":
                bad[i, 3] = -1.0
            elif kind == "tmin nan":
                bad[i, 3] = np.nan
            else:
                bad[i, 3] = bad[i, 7] = 0.25
    rows = np.array(sorted(where))
    others = np.setdiff1d(np.arange(n), rows)
    assert (case["refs"]["scattered"]["hit"][rows]).sum() >= 6  # (most of them would have hit something)
    for sort in (False, True):
        for any_hit in (False, True):
            a, b = cast(r, good, any_hit=any_hit, sort=sort), cast(r, bad, any_hit=any_hit, sort=sort)
            assert same_bits(a[others], b[others]), (sort, any_hit)
            if any_hit:
                assert not b[rows].any(), (sort, [where[i] for i in rows[b[rows] != 0]])
            else:
                for i in rows:
                    assert same_bits(b[i:i + 1], np.full(1, MISS, HIT)), (sort, where[i], b[i])
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 4: updates are seen
# ------------------------------------------------------------------------------------------------
def test_updates_and_hidden_submeshes_are_seen(cases):
    sc0, updates = V.room_updates()
    sa = clone(sc0)
    r = room_renderer(sa)
    for name, kind, payload, sc in updates:
        if kind == "transforms":
            r.update_transforms(*payload)
        else:
            update_vertices(r, payload)
    shown = cases["updated"]
    before = {k: (cast(r, shown["sets"][k]), cast(r, shown["sets"][k], any_hit=True)) for k in ("scattered", "outside")}
    for k, (hits, occ) in before.items():
        judged(shown, k, hits, occ, f"updated / {k}")
        assert (hits["geometry"] == Q.HIDDEN).any()  # the tall box is there to be seen
    r.set_visible([Q.HIDDEN], False)
    case = cases["updated, 2 hidden"]
    for k in ("scattered", "outside"):
        hits, occ = cast(r, case["sets"][k]), cast(r, case["sets"][k], any_hit=True)
        judged(case, k, hits, occ, f"updated, 2 hidden / {k}")
        assert not (hits["geometry"] == Q.HIDDEN).any(), k
        assert same_bits(hits, cast(r, case["sets"][k], sort=True))
    r.set_visible([Q.HIDDEN], True)
    for k, (hits, occ) in before.items():
        assert same_bits(hits, cast(r, shown["sets"][k])) and same_bits(occ, cast(r, shown["sets"][k], any_hit=True)), k
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 5: ordering across streams
# ------------------------------------------------------------------------------------------------
def test_a_query_runs_behind_an_update_on_another_stream_and_a_later_update_waits_for_it():
    sc0, updates = V.room_updates()
    _, _, (indices, moved), s1 = updates[0]  # the boxes rotated
    orig = np.stack([sc0.geometries[i]["M"] for i in indices])
    tris = Q.triangles(s1)
    one = Q.ray_sets(*Q.scene_box(s1), tris)["scattered"]
    ref = Q.reference(tris, one)
    rays = np.tile(one, (8, 1))  # (a query long enough for an update to overtake, if it could)
    r = room_renderer(clone(sc0))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    d = on_device(rays)
    still = to_host(enqueue(r, d))  # the scene before the move
    torch.cuda.synchronize()
    r.update_transforms(indices, moved, stream=a.cuda_stream)
    out1 = enqueue(r, d, stream=b)  # no host synchronisation in between
    torch.cuda.synchronize()
    h1 = to_host(out1)
    # the opposite order: the query on b, then an update on a that moves the boxes back
    out2 = enqueue(r, d, sort=True, stream=b)
    r.update_transforms(indices, orig, stream=a.cuda_stream)
    torch.cuda.synchronize()
    h2 = to_host(out2)
    back = to_host(enqueue(r, d))
    torch.cuda.synchronize()
    for what, h in (("query behind the update", h1), ("update behind the query", h2)):
        for k in range(8):
            part = h[k * len(one):(k + 1) * len(one)]
            assert same_bits(part, h[:len(one)]), (what, k)
        Q.check(Q.judge(tris, one, ref, {k: h[k][:len(one)] for k in ("t", "u", "v", "geometry", "primitive")}), what)
    assert same_bits(h1, h2)
    assert same_bits(back, still) and not same_bits(still, h1)  # the move changes answers, and moving back restores them
    r.destroy()


# ------------------------------------------------------------------------------------------------
# 6: the sort scratch
# ------------------------------------------------------------------------------------------------
def _free_bytes():  # (tests/test_soak_gpu.py's query)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_sorted_calls_of_growing_size_on_alternating_streams(cases):
    """three sorted queries of growing size on alternating streams, each followed at once by a smaller one on the other stream: every
    one grows the block (host wait, free, allocate) under the call before it, every smaller one reuses it from another stream"""
    case = cases["room"]
    r = room_renderer(clone(case["scene"]))
    pool = np.tile(np.concatenate([case["sets"][k] for k in ("scattered", "outside", "axis", "second")]), (2, 1))
    sizes = [(3001, 1000), (9000, 4097), (len(pool), 8229)]
    d = {n: on_device(pool[-n:] if k % 2 else pool[:n]) for k, n in enumerate(s for pair in sizes for s in pair)}
    plain = {(n, any_hit): to_host(enqueue(r, d[n], any_hit=any_hit)) for n in d for any_hit in (False, True)}
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for any_hit in (False, True):
        outs = []
        for k, (big, small) in enumerate(sizes):
            outs.append((big, enqueue(r, d[big], any_hit=any_hit, sort=True, stream=streams[k % 2])))
            outs.append((small, enqueue(r, d[small], any_hit=any_hit, sort=True, stream=streams[(k + 1) % 2])))
        torch.cuda.synchronize()
        for n, out in outs:
            assert same_bits(to_host(out), plain[(n, any_hit)]), (n, any_hit)
    r.destroy()


def test_contexts_that_sorted_give_their_scratch_back(cases):
    """Three contexts, each with a sorted 8 k-ray query -- and a sorted 2 M-ray one behind it, whose 33 MB block a margin of 32 MB
    cannot hide -- created and destroyed: the free device memory returns to where it started, within test_soak_gpu's margins."""
    sc = cases["room"]["scene"]
    small = on_device(np.tile(cases["room"]["sets"]["scattered"], (2, 1)))
    want = None

    def life():
        nonlocal want
        r = room_renderer(clone(sc))
        big = small.repeat(256, 1)
        out = enqueue(r, small, sort=True)
        out_big = enqueue(r, big, any_hit=True, sort=True)
        torch.cuda.synchronize()
        got = to_host(out)
        want = got if want is None else want
        assert same_bits(got, want) and out_big.shape[0] == 256 * small.shape[0] and not (out_big == 0x5A5A5A5A).any()
        del big, out, out_big
        in_use = _free_bytes()
        r.destroy()
        return in_use

    life()  # (the first context also pays for the process's one-off state)
    start = _free_bytes()
    held = []
    for _ in range(3):
        in_use = start - life()
        held.append(start - _free_bytes())
        assert in_use > 32 << 20, in_use  # (the context did hold its sort block: the measurement sees it)
    print(f"[scratch] device memory still held after each destroy (MB): {[round(h / 2**20, 2) for h in held]}")
    assert max(held) < 32 << 20, held
    assert held[-1] <= held[0] + (8 << 20), held


# ------------------------------------------------------------------------------------------------
# 7: refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_name_the_cause(cases):
    case = cases["room"]
    rays = case["sets"]["scattered"]
    n = len(rays)
    d = on_device(rays)
    r = DeferredRenderer()
    r.init(W, H)
    lib, ctx = r._lib, r._ctx
    out = torch.full((n + 1, 8), float("nan"), dtype=torch.float32, device="cuda")

    def call(p_rays, count, flags, p_out):
        return lib.neb_gi_cast_rays(ctx, C.c_void_p(p_rays), count, flags, C.c_void_p(p_out), None)

    def error():
        return lib.neb_last_error(ctx)

    assert call(d.data_ptr(), n, 0, out.data_ptr()) == -4 and b"neb_gi_cast_rays" in error()  # no scene
    sc = clone(case["scene"])
    G, ng, M, nm, T, nt = sc.descs()
    assert lib.neb_gi_set_scene(ctx, G, ng, M, nm, T, nt) == 0
    assert call(d.data_ptr(), n, 0, out.data_ptr()) == -4 and b"not ready" in error()  # a scene, no tree
    assert lib.neb_gi_build_bvh(ctx, None) == 0
    host_mem = torch.empty((n + 2, 8), dtype=torch.float32)
    host_ptr = (host_mem.data_ptr() + 31) & ~31  # (aligned: refused for where it lies, not for how)
    torch.cuda.empty_cache()
    block = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")  # (an allocation of its own: the caching allocator hands out whole segments at this size)
    end = block.data_ptr() + block.numel()
    refused = [("host-memory rays", (host_ptr, n, 0, out.data_ptr()), -1, b"rays is not memory"),
               ("host-memory out", (d.data_ptr(), n, 0, host_ptr), -1, b"out is not memory"),
               ("misaligned out", (d.data_ptr(), n, 0, out.data_ptr() + 16), -1, b"misaligned"),
               ("misaligned any-hit out", (d.data_ptr(), n, _lib.RAYS_ANY_HIT, out.data_ptr() + 2), -1, b"misaligned"),
               ("misaligned rays", (d.data_ptr() + 8, n - 1, 0, out.data_ptr()), -1, b"misaligned"),
               ("null rays", (0, n, 0, out.data_ptr()), -1, b"null"),
               ("null out", (d.data_ptr(), n, 0, 0), -1, b"null"),
               ("out overlapping rays", (d.data_ptr(), n, 0, d.data_ptr() + 32 * (n - 1)), -1, b"overlaps"),
               ("out is rays", (d.data_ptr(), n, _lib.RAYS_SORT, d.data_ptr()), -1, b"overlaps"),
               ("unknown flag", (d.data_ptr(), n, 4, out.data_ptr()), -1, b"flag"),
               ("out too small for its allocation", (d.data_ptr(), n, 0, end - 32 * (n - 1)), -1, b"out is not memory"),
               ("any-hit out too small for its allocation", (d.data_ptr(), n, _lib.RAYS_ANY_HIT | _lib.RAYS_SORT, end - 4 * (n - 1)), -1, b"out is not memory"),
               ("rays too short for their allocation", (end - 32 * (n - 1), n, 0, out.data_ptr()), -1, b"rays is not memory")]
    torch.cuda.synchronize()
    for what, args, want, word in refused:
        assert call(*args) == want, what
        assert b"neb_gi_cast_rays" in error() and word in error(), (what, error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote something"
    assert call(0, 0, 0, 0) == 0 and call(0, 0, _lib.RAYS_ANY_HIT | _lib.RAYS_SORT, 0) == 0  # n == 0: a no-op that succeeds
    # ... and the same context answers: the range that just fits its allocation is accepted
    assert call(d.data_ptr(), n, 0, end - 32 * n) == 0
    assert call(d.data_ptr(), n, 0, out.data_ptr()) == 0
    torch.cuda.synchronize()
    hits = to_host(out[:n])
    judged(case, "scattered", hits, (hits["geometry"] != NO_SUBMESH).astype(U32), "after the refusals")
    assert bool(torch.isnan(out[n]).all())
    r.destroy()


def test_the_python_mirror_checks_its_arguments(cases):
    r = room_renderer(clone(cases["room"]["scene"]))
    d = on_device(cases["room"]["sets"]["scattered"][:100])
    from nebulae_amd.svgf import NebError
    for bad in (d.cpu(), d[:, :7], d.double(), d[::2]):
        with pytest.raises(NebError):
            r.cast_rays(bad)
    with pytest.raises(NebError):
        r.cast_rays(d, out=torch.empty((100, 8), dtype=torch.float32))
    res = r.cast_rays(d)
    assert set(res) == {"t", "u", "v", "geometry", "primitive", "records"} and res["geometry"].dtype == torch.int32
    assert all(res[k].data_ptr() - res["records"].data_ptr() == 4 * i for i, k in enumerate(("t", "u", "v", "geometry", "primitive")))
    empty = r.cast_rays(d[:0], any_hit=True, sort=True)
    assert empty["occluded"].shape == (0,)
    torch.cuda.synchronize()
    r.destroy()
