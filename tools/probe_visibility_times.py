"""Cost of the visibility calls beside the plain ones on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8f.

  python tools/probe_visibility_times.py [--out profiles/probe_visibility_times.json] [--calls 30] [--warmup 5] [--triangles 262267]

Three pairs, the two arms of a pair timed INTERLEAVED in one run and process (a, b, a, b, ...: whatever the clocks do, they do to both),
device time of one call between two events on the null stream, medians of `calls` after `warmup`:
  bake    neb_gi_bake_visibility of 4096 probes x 256 samples  against  neb_gi_cast_rays over the same rays (neb_gi_probe_rays', made once);
  gather  neb_gi_gather_probes_visible  against  neb_gi_gather_probes at the 1080p camera's primary hit points, in pixel order and in a fixed
          random permutation, on a 32 x 16 x 32 grid (2 MB of records, 12.6 MB of maps) and a 128 x 64 x 128 grid (134 MB, 805 MB);
  frame   neb_gi_probe_indirect_visible  against  neb_gi_probe_indirect on the bench frame's 1080p G-buffer, the same two grids.
The maps are baked on the scene for the small grid and random (m1 in 0.2 .. 2 spacings) for the large one, whose bake is not what is timed.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_visibility_times.json"))
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
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo
    from nebulae_amd.svgf import PLANE_RADIANCE
    from ray_query_times import primary_rays

    if not torch.cuda.is_available():
        raise SystemExit("probe_visibility_times: no GPU visible")
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
    r.submit_commands_gbuffer()
    r.submit_commands_pbr_lighting()
    torch.cuda.synchronize()
    tris, nodes = r.scene_info()
    lo, hi = (np.asarray(v, np.float64) for v in sc.world_aabb())
    n = W * H

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def pair(plain, visible):
        """the two arms interleaved -> {"plain": .., "visible": .., "visible_over_plain": ..}"""
        us = {"plain": [], "visible": []}
        for k in range(args.warmup + args.calls):
            for name, fn in (("plain", plain), ("visible", visible)):
                t = once(fn)
                if k >= args.warmup:
                    us[name].append(t)
        row = {k: {"us": float(np.median(v)), "p10_p90_us": [float(np.percentile(v, 10)), float(np.percentile(v, 90))]} for k, v in us.items()}
        row["visible_over_plain"] = row["visible"]["us"] / row["plain"]["us"]
        return row

    def random_records(count, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rec = torch.randn((count, 32), generator=g, device="cuda")
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

    # ---- the bake beside the walk of the same rays ----
    side = round(BAKE_PROBES ** (1.0 / 3.0))
    bake_dims = (side, side, BAKE_PROBES // (side * side))
    bake_grid, bake_probes = r.probe_grid(lo + 0.05 * (hi - lo), 0.9 * (hi - lo) / (np.array(bake_dims) - 1), bake_dims, tmin=1e-3, tmax=1e4)
    count = bake_probes.shape[0]
    max_distance = 1.5 * float(np.linalg.norm(0.9 * (hi - lo) / (np.array(bake_dims) - 1)))
    rays = r.probe_rays(bake_probes, BAKE_SAMPLES, "sh")
    hits = torch.empty((rays.shape[0], 8), dtype=torch.float32, device="cuda")
    maps = torch.empty((count, 192), dtype=torch.float32, device="cuda")
    bake = pair(lambda: r.cast_rays(rays, out=hits), lambda: r.bake_visibility(bake_probes, BAKE_SAMPLES, max_distance=max_distance, out=maps))
    bake.update(probes=count, samples=BAKE_SAMPLES, rays=int(rays.shape[0]), ray_and_hit_bytes_the_bake_does_not_touch=64 * int(rays.shape[0]))
    print("bake", json.dumps(bake), flush=True)
    del rays, hits, maps

    # ---- the gathers at the camera's primary hit points ----
    prim = torch.from_numpy(primary_rays(cam, W, H)).cuda()
    surf = r.shade_rays(prim, "surface")
    torch.cuda.synchronize()
    found = (surf["flags"] & _lib.HIT_FOUND) != 0
    pixel = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    pixel[:, 0:3], pixel[:, 4:7] = surf["position"], surf["shading_normal"]
    pixel[~found] = 0.0
    order = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    inputs = {"pixel_order": pixel, "permuted": pixel[order].contiguous()}
    del prim, surf

    radiance = r.svgf.plane_tensor(PLANE_RADIANCE).view(n, 4)
    direct = radiance.clone()
    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    gather_rows, frame_rows = {}, {}
    for name, dims in GRIDS.items():
        count = dims[0] * dims[1] * dims[2]
        spacing = (hi - lo) / (np.array(dims) - 1)
        grid, probes = r.probe_grid(lo, spacing, dims, tmin=1e-3, tmax=1e4)
        rec = random_records(count, 3)
        bias = 0.05 * float(spacing.min())
        if count <= 1 << 15:
            maps = r.bake_visibility(probes, 64, max_distance=1.5 * float(np.linalg.norm(spacing)))["records"]
        else:
            maps = random_maps(count, float(np.median(spacing)), 4)
        del probes
        for order_name, pts in inputs.items():
            row = pair(lambda: r.gather_probes(grid, rec, pts, out=out), lambda: r.gather_probes(grid, rec, pts, out=out, visibility=maps, normal_bias=bias))
            res = r.gather_probes(grid, rec, pts, out=out, visibility=maps, normal_bias=bias)
            torch.cuda.synchronize()
            row["points"], row["usable_points"] = n, int(((res["flags"] & _lib.GATHER_NOT_GATHERED) == 0).sum())
            row["extra_tap_bytes_per_usable_point"] = 8 * 4 * 8  # eight corners, four 8-byte taps each
            gather_rows[f"{name}/{order_name}"] = row
            print(name, order_name, json.dumps(row), flush=True)
        for weight in (False, True):
            radiance.copy_(direct)
            row = pair(lambda: r.submit_commands_gi_probes(grid, rec, frame_weight=weight),
                       lambda: r.submit_commands_gi_probes(grid, rec, frame_weight=weight, visibility=maps, normal_bias=bias))
            frame_rows[f"{name}/{'frame_weight' if weight else 'plain_weight'}"] = row
            print(name, "frame", weight, json.dumps(row), flush=True)
        radiance.copy_(direct)
        del rec, maps

    result = {"what": "the visibility calls beside the plain ones, the two arms of each pair interleaved in one run; device times of one call between events, "
                      "medians", "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
              "triangles": tris, "nodes": nodes, "bake_against_cast_rays": bake, "gather": gather_rows, "frame": frame_rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
