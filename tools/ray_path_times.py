"""Cost of neb_gi_trace_paths on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8b.

  python tools/ray_path_times.py [--out profiles/ray_path_times.json] [--calls 50] [--warmup 5] [--triangles 262267]

Device time of one call between two events on the null stream (median of `calls`, after `warmup`) on the 1080p camera's 2.07 M
primary rays, in pixel order and in a fixed random permutation, unsorted and with NEB_RAYS_SORT, for maxPathVertices K = 2, 3, 5, 8
-- and, in the same run and process, NEB_SHADE_RADIANCE of neb_gi_shade_rays on the same inputs, measured three times (before, between
and after the path calls): the spread of its medians is the yardstick K = 2 is held against (`k2_within_radiance_spread`).  Also K = 2
with the vertex records, the share of paths alive per segment and the mean number of segments (the lane utilisation of the one-lane-
per-ray loop).  The JSON carries the library's build id.  Needs a GPU; no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KS = (2, 3, 5, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_path_times.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo
    from ray_query_times import primary_rays

    if not torch.cuda.is_available():
        raise SystemExit("ray_path_times: no GPU visible")
    W, H = args.width, args.height
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
    tris, nodes = r.scene_info()
    consts = r.global_constants()

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

    n = W * H
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).cuda()
    inputs = {"pixel_order": torch.from_numpy(primary_rays(cam, W, H)).cuda()}
    inputs["shuffled"] = inputs["pixel_order"][perm].contiguous()
    out8 = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    vert = torch.empty((n, 1, 24), dtype=torch.float32, device="cuda")

    # the answers first: K = 2 is NEB_SHADE_RADIANCE's record, sorted == unsorted on the timed inputs
    rad = r.shade_rays(inputs["shuffled"], "radiance", constants=consts)["records"].clone().view(torch.int32)
    k2 = r.trace_paths(inputs["shuffled"], constants=consts, max_path_vertices=2)["records"].clone().view(torch.int32)
    same = bool((k2[:, :6] == rad[:, :6]).all()) and bool(((k2[:, 6] & 0x3F) == rad[:, 6]).all())
    alive, mean_segments = {}, {}
    for K in KS:
        a = r.trace_paths(inputs["shuffled"], constants=consts, max_path_vertices=K)["records"].clone().view(torch.int32)
        b = r.trace_paths(inputs["shuffled"], constants=consts, max_path_vertices=K, sort=True)["records"].clone().view(torch.int32)
        torch.cuda.synchronize()
        same = same and bool((a == b).all())
        seg = a[:, 7]
        alive[str(K)] = [float((seg >= k).float().mean()) for k in range(1, K)]  # the share of paths that walk segment k
        mean_segments[str(K)] = float(seg.float().mean())
    if not same:
        raise SystemExit("ray_path_times: K = 2 is not the radiance record, or sorted and unsorted answers differ")

    def radiance_round(tag):
        return {f"radiance_{name}{'_sorted' if sort else ''}_{tag}": timed(lambda: r.shade_rays(rays, "radiance", constants=consts, sort=sort, out=out8))
                for name, rays in inputs.items() for sort in (False, True)}

    cases = radiance_round("first")
    for K in KS:
        for name, rays in inputs.items():
            for sort in (False, True):
                tag = name + ("_sorted" if sort else "")
                cases[f"paths_k{K}_{tag}"] = timed(lambda: r.trace_paths(rays, constants=consts, max_path_vertices=K, sort=sort, out=out8))
        if K == 2:
            cases.update(radiance_round("second"))
            cases["paths_k2_vertices_pixel_order"] = timed(lambda: r.trace_paths(inputs["pixel_order"], constants=consts, max_path_vertices=2, vertices=vert,
                                                                                 out=out8))
    cases.update(radiance_round("third"))

    verdict = {}
    for name in inputs:
        for sort in (False, True):
            tag = name + ("_sorted" if sort else "")
            rounds = [cases[f"radiance_{tag}_{t}"]["us"] for t in ("first", "second", "third")]
            k2_us = cases[f"paths_k2_{tag}"]["us"]
            verdict[tag] = {"radiance_medians_us": rounds, "paths_k2_us": k2_us, "within": bool(min(rounds) <= k2_us <= max(rounds)),
                            "k2_over_radiance_median": k2_us / float(np.median(rounds))}

    out = {"what": "neb_gi_trace_paths on the sponza stand-in beside NEB_SHADE_RADIANCE of neb_gi_shade_rays; device times of one call between events, medians",
           "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "width": W, "height": H, "rays": n, "k2_equals_radiance_and_sorted_equals_unsorted": same,
           "share_of_paths_walking_segment": alive, "mean_segments": mean_segments, "cases": cases, "k2_within_radiance_spread": verdict}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
