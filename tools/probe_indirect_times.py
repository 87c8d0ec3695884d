"""Cost of neb_gi_probe_indirect on the bench scene's 1080p G-buffer (sponza stand-in: 262 k triangles), DESIGN.md 3.8e.

  python tools/probe_indirect_times.py [--out profiles/probe_indirect_times.json] [--calls 30] [--warmup 5] [--triangles 262267] [--time-limit 420]

The frame's G-buffer comes from neb_gbuffer_raycast; the grids are those of tools/probe_volume_times.py: 32 x 16 x 32 over the scene box
(2 MB of records) and 128 x 64 x 128 (134 MB), random records, a tenth of the probes invalid.  Per grid, in one run and one process, device
time between two events on the null stream (median of `calls`, after `warmup`) of
  (a) the fused call, without and with NEB_INDIRECT_FRAME_WEIGHT;
  (b) the three steps it replaces: neb_gbuffer_points, neb_gi_gather_probes on those points, and the diffuse weighting as a torch
      expression on the plane tensors (decode of albedo and metalness, k * E / pi, the masked add) -- each alone and the three in a row;
and, for scale, neb_gi_trace on the same frame.  The whole run ends after --time-limit seconds whatever happens.  The JSON carries the
library's build id.  Needs a GPU; no CPU fallback.
"""
import argparse
import json
import math
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
GRIDS = {"grid_32x16x32": (32, 16, 32), "grid_128x64x128": (128, 64, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_indirect_times.json"))
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
    from nebulae_amd.svgf import PLANE_ALBEDO, PLANE_RADIANCE, PLANE_ROUGH_METAL

    if not torch.cuda.is_available():
        raise SystemExit("probe_indirect_times: no GPU visible")
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

    def timed(fn):
        us = []
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                us.append(e0.elapsed_time(e1) * 1e3)
        return {"us": float(np.median(us)), "p10_p90_us": [float(np.percentile(us, 10)), float(np.percentile(us, 90))]}

    def random_records(count, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rec = torch.randn((count, 32), generator=g, device="cuda")
        ints = rec.view(torch.int32)
        ints[:, 27], ints[:, 28], ints[:, 30], ints[:, 31] = 64, 32, 128, 0
        ints[:, 29] = (torch.rand(count, generator=g, device="cuda") < 0.1).int() * 32  # a tenth of the probes see too many backfaces
        return rec

    radiance = r.svgf.plane_tensor(PLANE_RADIANCE).view(n, 4)
    albedo_words = r.svgf.plane_tensor(PLANE_ALBEDO, 0).view(n)
    rough_metal = r.svgf.plane_tensor(PLANE_ROUGH_METAL, 0).view(n, 2)
    direct = radiance.clone()

    def small_float(bits, mbits):
        e, m = bits >> mbits, (bits & ((1 << mbits) - 1)).float() / float(1 << mbits)
        return torch.where(e == 0, m * 2.0 ** -14, (1.0 + m) * torch.exp2(e.float() - 15.0))

    def torch_weighting(gathered):
        """the third step a host had to write: radiance += albedo * (1 - metalness) * E / pi where the gather found a probe"""
        ids = gathered.view(torch.int32)
        lit = (ids[:, 6] & (_lib.GATHER_NOT_GATHERED | _lib.GATHER_NO_PROBE)) == 0
        v = albedo_words
        albedo = torch.stack([small_float(v & 0x7FF, 6), small_float((v >> 11) & 0x7FF, 6), small_float((v >> 22) & 0x3FF, 5)], 1)
        k = albedo * (1.0 - rough_metal[:, 1].float())[:, None]
        radiance[:, 0:3] += torch.where(lit[:, None], k * gathered[:, 0:3] * (1.0 / math.pi), torch.zeros_like(k))

    points = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    gathered = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    rows = {}
    for name, dims in GRIDS.items():
        count = dims[0] * dims[1] * dims[2]
        grid, _ = r.probe_grid(lo, (hi - lo) / (np.array(dims) - 1), dims)
        rec = random_records(count, 3)

        def three_steps():
            r.gbuffer_points(out=points)
            r.gather_probes(grid, rec, points, out=gathered)
            torch_weighting(gathered)

        # the two routes give the same frame: once each from the same start, before anything is timed
        radiance.copy_(direct)
        r.submit_commands_gi_probes(grid, rec, frame_weight=False)
        fused = radiance.clone()
        radiance.copy_(direct)
        three_steps()
        torch.cuda.synchronize()
        res = r.gather_probes(grid, rec, points, out=gathered)
        lit = (res["flags"] & (_lib.GATHER_NOT_GATHERED | _lib.GATHER_NO_PROBE)) == 0
        row = {"largest_difference_fused_minus_three_steps": float((fused - radiance).abs().max()), "largest_gain": float((fused - direct).max()),
               "pixels": n, "pixels_stored_to": int(lit.sum()), "compulsory_bytes_fused": 28 * n + 16 * int(lit.sum()) + 16 * int(lit.sum()),
               "fused": timed(lambda: r.submit_commands_gi_probes(grid, rec, frame_weight=False)),
               "fused_frame_weight": timed(lambda: r.submit_commands_gi_probes(grid, rec, frame_weight=True)),
               "step_points": timed(lambda: r.gbuffer_points(out=points)),
               "step_gather": timed(lambda: r.gather_probes(grid, rec, points, out=gathered)),
               "step_torch_weighting": timed(lambda: torch_weighting(gathered)),
               "three_steps": timed(three_steps)}
        row["fused_over_three_steps"] = row["fused"]["us"] / row["three_steps"]["us"]
        row["fused_over_points_plus_gather"] = row["fused"]["us"] / (row["step_points"]["us"] + row["step_gather"]["us"])
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del rec
    radiance.copy_(direct)
    trace = timed(lambda: r.submit_commands_gi_pathtrace())
    print("neb_gi_trace", json.dumps(trace), flush=True)
    out = {"what": "neb_gi_probe_indirect on the bench scene's 1080p G-buffer beside the three steps it replaces (neb_gbuffer_points, neb_gi_gather_probes, "
                   "a torch expression of the weighting) and beside neb_gi_trace; device times between events, medians", "calls_per_case": args.calls,
           "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0), "triangles": tris, "nodes": nodes,
           "grids": rows, "neb_gi_trace": trace}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
