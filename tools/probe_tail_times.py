"""Cost of a path that ends in a probe grid beside the paths that walk on, on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8g.

  python tools/probe_tail_times.py [--out profiles/probe_tail_times.json] [--calls 30] [--warmup 5] [--triangles 262267]

Two groups, the arms of a group timed INTERLEAVED in one run and process (a, b, c, ..., a, b, c, ...: whatever the clocks do, they do to
all), device time of one call between two events on the null stream, medians of `calls` after `warmup`:
  bake   neb_gi_bake_probes(_tail) of 4096 probes x 256 samples;
  paths  neb_gi_trace_paths(_tail) over the 1080p camera's primary rays;
each with the arms  plain K = 2,  tail K = 2 with the plain and with the visible gather on a 32 x 16 x 32 grid (2 MB of records) and on a
128 x 64 x 128 grid (134 MB),  plain K = 3  and  plain K = 8.  The comparison that matters is tail K = 2 against plain K = 3: the cheapest
way there was to one more bounce.  The grids' records and maps are random: what they hold does not change what is loaded.
The JSON carries the library's build id.  Needs a GPU; no CPU fallback.
"""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
W, H = 1920, 1080
GRIDS = {"grid_32x16x32": (32, 16, 32), "grid_128x64x128": (128, 64, 128)}
BAKE_PROBES, BAKE_SAMPLES = 4096, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_tail_times.json"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    ap.add_argument("--time-limit", type=int, default=420)
    args = ap.parse_args()
    signal.alarm(args.time_limit)  # (SIGALRM's default action ends the process)

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import _lib
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, ProbeTail, RenderInfo
    from ray_query_times import primary_rays

    if not torch.cuda.is_available():
        raise SystemExit("probe_tail_times: no GPU visible")
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
    torch.cuda.synchronize()
    tris, nodes = r.scene_info()
    lo, hi = (np.asarray(v, np.float64) for v in sc.world_aabb())

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def group(arms):
        """the arms interleaved -> {name: {"us": median, "p10_p90_us": [..]}}"""
        us = {name: [] for name in arms}
        for k in range(args.warmup + args.calls):
            for name, fn in arms.items():
                t = once(fn)
                if k >= args.warmup:
                    us[name].append(t)
        return {k: {"us": float(np.median(v)), "p10_p90_us": [float(np.percentile(v, 10)), float(np.percentile(v, 90))]} for k, v in us.items()}

    def random_records(count, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rec = torch.rand((count, 32), generator=g, device="cuda")
        ints = rec.view(torch.int32)
        ints[:, 27], ints[:, 28], ints[:, 30], ints[:, 31] = 64, 32, 128, 0
        ints[:, 29] = (torch.rand(count, generator=g, device="cuda") < 0.1).int() * 32  # a tenth of the probes see too many backfaces
        return rec

    def random_maps(count, spacing, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        maps = torch.empty((count, 192), dtype=torch.float32, device="cuda")
        m1 = (0.2 + 1.8 * torch.rand((count, 64), generator=g, device="cuda")) * spacing
        maps[:, 0:128:2], maps[:, 1:128:2] = m1, m1 * m1 * (1.01 + 0.49 * torch.rand((count, 64), generator=g, device="cuda"))
        maps[:, 128:] = 1.0
        return maps

    tails = {}
    for name, dims in GRIDS.items():
        count = dims[0] * dims[1] * dims[2]
        spacing = (hi - lo) / (np.array(dims) - 1)
        grid, probes = r.probe_grid(lo, spacing, dims, tmin=1e-3, tmax=1e4)
        del probes
        rec, maps = random_records(count, 3), random_maps(count, float(np.median(spacing)), 4)
        tails[f"tail_K2/{name}/plain_gather"] = ProbeTail(grid, rec)
        tails[f"tail_K2/{name}/visible_gather"] = ProbeTail(grid, rec, maps, 0.05 * float(spacing.min()))

    def constants(K):
        c = r.global_constants()
        c = type(c).from_buffer_copy(c)
        c.maxPathVertices = K
        return c
    c2, c3, c8 = constants(2), constants(3), constants(8)

    # ---- the bake ----
    side = round(BAKE_PROBES ** (1.0 / 3.0))
    bake_dims = (side, side, BAKE_PROBES // (side * side))
    _, bake_probes = r.probe_grid(lo + 0.05 * (hi - lo), 0.9 * (hi - lo) / (np.array(bake_dims) - 1), bake_dims, tmin=1e-3, tmax=1e4)
    rec_out = torch.empty((bake_probes.shape[0], 32), dtype=torch.float32, device="cuda")
    arms = {"plain_K2": lambda: r.bake_probes(bake_probes, BAKE_SAMPLES, "sh", constants=c2, out=rec_out)}
    for name, tail in tails.items():
        arms[name] = lambda tail=tail: r.bake_probes(bake_probes, BAKE_SAMPLES, "sh", constants=c2, out=rec_out, tail=tail)
    arms["plain_K3"] = lambda: r.bake_probes(bake_probes, BAKE_SAMPLES, "sh", constants=c3, out=rec_out)
    arms["plain_K8"] = lambda: r.bake_probes(bake_probes, BAKE_SAMPLES, "sh", constants=c8, out=rec_out)
    bake = group(arms)
    for name in tails:
        bake[name]["over_plain_K3"] = bake[name]["us"] / bake["plain_K3"]["us"]
        bake[name]["over_plain_K2"] = bake[name]["us"] / bake["plain_K2"]["us"]
    bake.update(probes=int(bake_probes.shape[0]), samples=BAKE_SAMPLES)
    print("bake", json.dumps(bake), flush=True)

    # ---- the path query over the primary rays ----
    prim = torch.from_numpy(primary_rays(cam, W, H)).cuda()
    out = torch.empty((prim.shape[0], 8), dtype=torch.float32, device="cuda")
    arms = {"plain_K2": lambda: r.trace_paths(prim, constants=c2, out=out)}
    for name, tail in tails.items():
        arms[name] = lambda tail=tail: r.trace_paths(prim, constants=c2, out=out, tail=tail)
    arms["plain_K3"] = lambda: r.trace_paths(prim, constants=c3, out=out)
    arms["plain_K8"] = lambda: r.trace_paths(prim, constants=c8, out=out)
    paths = group(arms)
    for name in tails:
        paths[name]["over_plain_K3"] = paths[name]["us"] / paths["plain_K3"]["us"]
        paths[name]["over_plain_K2"] = paths[name]["us"] / paths["plain_K2"]["us"]
    res = r.trace_paths(prim, constants=c2, out=out, tail=tails["tail_K2/grid_32x16x32/plain_gather"])
    torch.cuda.synchronize()
    paths.update(rays=int(prim.shape[0]), paths_that_end_in_the_grid=int(((res["flags"] & _lib.PATH_TAIL) != 0).sum()))
    print("paths", json.dumps(paths), flush=True)

    result = {"what": "paths that end in a probe grid beside paths that walk on, the arms of a group interleaved in one run; device times of one call between "
                      "events, medians", "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
              "triangles": tris, "nodes": nodes, "bake": bake, "trace_paths": paths}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
