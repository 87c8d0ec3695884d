"""Cost of neb_gi_bake_probes on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8c.

  python tools/probe_bake_times.py [--out profiles/probe_bake_times.json] [--calls 50] [--warmup 5] [--triangles 262267]

Three setups -- 4096 SH probes on a 16^3 grid in the scene box with S = 64 and with S = 256 samples, and 262 144 irradiance probes on a
512^2 grid just above the floor with S = 64 -- each for maxPathVertices K = 2, 3, 5.  Per setup and K, in the same run and process,
device time of one call between two events on the null stream (median of `calls`, after `warmup`) of
  (a) bake_probes;
  (b) trace_paths alone over the rays probe_rays wrote (the kernel of DESIGN.md 3.8b: the yardstick);
  (c) the route a host had before: probe_rays, then trace_paths, then a torch projection and reduction,
with the device memory each of (a) and (c) needs, the lane utilisation segments / (S (K - 1)) from (a)'s own records and the largest
difference between (a)'s and (c)'s results.  The JSON carries the library's build id.  Needs a GPU; no CPU fallback.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (2, 3, 5)
SH_K = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bake_times.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("probe_bake_times: no GPU visible")
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    r = DeferredRenderer()
    r.init(1920, 1080, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
    tris, nodes = r.scene_info()
    consts = r.global_constants()
    lo, hi = (np.asarray(v, np.float64) for v in sc.world_aabb())

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

    def grid(n_axis):
        t = (np.arange(n_axis) + 0.5) / n_axis
        g = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
        pr = np.zeros((len(g), 8), np.float32)
        pr[:, 0:3], pr[:, 3], pr[:, 4:7], pr[:, 7] = lo + (0.05 + 0.9 * g) * (hi - lo), 1e-3, (0.0, 1.0, 0.0), 1e4
        return pr

    def floor(n_axis):
        t = (np.arange(n_axis) + 0.5) / n_axis
        u, v = (a.reshape(-1) for a in np.meshgrid(t, t, indexing="ij"))
        pr = np.zeros((len(u), 8), np.float32)
        pr[:, 0], pr[:, 1], pr[:, 2] = lo[0] + (0.05 + 0.9 * u) * (hi[0] - lo[0]), lo[1] + 0.01 * (hi[1] - lo[1]), lo[2] + (0.05 + 0.9 * v) * (hi[2] - lo[2])
        pr[:, 3], pr[:, 4:7], pr[:, 7] = 1e-3, (0.0, 1.0, 0.0), 1e4
        return pr

    def project(paths, rays, n, samples, what):
        """the torch projection and reduction a host would write: [n, 27] float32"""
        L = paths[:, 0:3]
        if what == "irradiance":
            return torch.cat([L.view(n, samples, 3).sum(1) * (math.pi / samples), torch.zeros((n, 24), dtype=torch.float32, device=L.device)], 1)
        x, y, z = rays[:, 4], rays[:, 5], rays[:, 6]
        k00, k1, k2a, k20, k22 = SH_K
        Y = torch.stack([torch.full_like(x, k00), k1 * y, k1 * z, k1 * x, k2a * x * y, k2a * y * z, k20 * (3.0 * z * z - 1.0), k2a * x * z, k22 * (x * x - y * y)], 1)
        return (L[:, None, :] * Y[:, :, None]).view(n, samples, 27).sum(1) * (4.0 * math.pi / samples)

    setups = [("grid_4096_s64", grid(16), 64, "sh"), ("grid_4096_s256", grid(16), 256, "sh"), ("floor_262144_s64", floor(512), 64, "irradiance")]
    results = {}
    for name, pr, samples, what in setups:
        n = len(pr)
        d = torch.from_numpy(pr).cuda()
        out = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        rays = torch.empty((n * samples, 8), dtype=torch.float32, device="cuda")
        paths = torch.empty((n * samples, 8), dtype=torch.float32, device="cuda")
        frame_index = int(consts.frameIndex)
        per_k = {}
        for K in KS:
            def bake():
                r.bake_probes(d, samples, what, constants=consts, max_path_vertices=K, out=out)

            def trace():
                r.trace_paths(rays, constants=consts, max_path_vertices=K, out=paths)

            def old_route():
                r.probe_rays(d, samples, what, frame_index=frame_index, out=rays)
                trace()
                return project(paths, rays, n, samples, what)

            r.probe_rays(d, samples, what, frame_index=frame_index, out=rays)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            want = old_route()
            torch.cuda.synchronize()
            old_extra = torch.cuda.max_memory_allocated() - before  # the projection's temporaries and result
            bake()
            torch.cuda.synchronize()
            rec = out.clone()
            seg = rec.view(torch.int32)[:, 30].double()
            case = {"bake": timed(bake), "trace_paths_alone": timed(trace), "old_route": timed(old_route)}
            case["bake_over_trace_paths"] = case["bake"]["us"] / case["trace_paths_alone"]["us"]
            case["bake_over_old_route"] = case["bake"]["us"] / case["old_route"]["us"]
            case["lane_utilisation"] = float(seg.sum() / (n * samples * (K - 1)))
            case["mean_hits_per_sample"] = float(rec.view(torch.int32)[:, 28].double().sum() / (n * samples))
            case["largest_difference_from_torch"] = float((rec[:, :27] - want).abs().max())
            case["largest_word"] = float(want.abs().max())
            case["bytes_bake"] = int(d.numel() * 4 + out.numel() * 4)
            case["bytes_old_route"] = int(d.numel() * 4 + rays.numel() * 4 + paths.numel() * 4 + old_extra)
            per_k[str(K)] = case
            print(name, K, json.dumps(case), flush=True)
        results[name] = {"probes": n, "samples": samples, "what": what, "waves": n, "k": per_k}
        del rays, paths, out

    out = {"what": "neb_gi_bake_probes on the sponza stand-in beside neb_gi_trace_paths over the same rays and the host's old route; device times of one call "
                   "between events, medians", "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(),
           "device": torch.cuda.get_device_name(0), "triangles": tris, "nodes": nodes, "setups": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
