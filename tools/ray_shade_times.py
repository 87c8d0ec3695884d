"""Cost of neb_gi_shade_rays on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8a.

  python tools/ray_shade_times.py [--out profiles/ray_shade_times.json] [--calls 50] [--warmup 5] [--triangles 262267]

Device time of one call between two events on the null stream (median of `calls`, after `warmup`) on the 1080p camera's 2.07 M
primary rays, in pixel order and in a fixed random permutation, unsorted and with NEB_RAYS_SORT, for NEB_SHADE_SURFACE and
NEB_SHADE_RADIANCE -- and, in the same run and process, the two yardsticks: neb_gi_cast_rays on the same four inputs (the floor:
the same walk, 32 bytes out per ray and no shading) and neb_gbuffer_raycast (the same walk over the same rays plus a reconstruction
of the same kind, its 22 bytes per pixel written along memory).  The JSON carries the library's build id.  Needs a GPU; no CPU
fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_shade_times.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import _lib
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo
    from ray_query_times import primary_rays

    if not torch.cuda.is_available():
        raise SystemExit("ray_shade_times: no GPU visible")
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
    outs = {"cast": torch.empty((n, 8), dtype=torch.float32, device="cuda"), "surface": torch.empty((n, 24), dtype=torch.float32, device="cuda"),
            "radiance": torch.empty((n, 8), dtype=torch.float32, device="cuda")}

    # the answers first: sorted == unsorted on the timed inputs, the ids are neb_gi_cast_rays' bits, the permutation only permutes
    hits = r.cast_rays(inputs["pixel_order"])["records"].clone().view(torch.int32)
    same = True
    counts = {}
    for what in ("surface", "radiance"):
        a = r.shade_rays(inputs["shuffled"], what, constants=consts)["records"].clone().view(torch.int32)
        b = r.shade_rays(inputs["shuffled"], what, constants=consts, sort=True)["records"].clone().view(torch.int32)
        torch.cuda.synchronize()
        same = same and bool((a == b).all())
        if what == "surface":  # {t, geometry, primitive, u, v} against the plain query, and the records against the pixel-order call
            p = r.shade_rays(inputs["pixel_order"], what)["records"].clone().view(torch.int32)
            same = same and bool((p[perm] == a).all())
            same = same and bool((p[:, [3, 7, 11, 20, 21]] == hits[:, [0, 3, 4, 1, 2]]).all())
            counts["hits"] = int(((p[:, 22] & _lib.HIT_FOUND) != 0).sum())
            counts["hits_with_material"] = int(((p[:, 22] & _lib.HIT_MATERIAL) != 0).sum())
        else:
            counts["hits_that_see_the_sun"] = int(((a[:, 6] & _lib.HIT_SUN_VISIBLE) != 0).sum())
    if not same:
        raise SystemExit("ray_shade_times: sorted, unsorted and plain-query answers differ")

    cases = {"gbuffer_raycast": timed(lambda: r.submit_commands_gbuffer())}
    for name, rays in inputs.items():
        for sort in (False, True):
            tag = name + ("_sorted" if sort else "")
            cases["cast_" + tag] = timed(lambda: r.cast_rays(rays, sort=sort, out=outs["cast"]))
            cases["surface_" + tag] = timed(lambda: r.shade_rays(rays, "surface", sort=sort, out=outs["surface"]))
            cases["radiance_" + tag] = timed(lambda: r.shade_rays(rays, "radiance", constants=consts, sort=sort, out=outs["radiance"]))
    cases["gbuffer_raycast_again"] = timed(lambda: r.submit_commands_gbuffer())

    out = {"what": "neb_gi_shade_rays on the sponza stand-in, beside neb_gi_cast_rays and neb_gbuffer_raycast; device times of one call between events, medians",
           "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "width": W, "height": H, "rays": n, **counts, "sorted_equals_unsorted": same, "cases": cases,
           "surface_over_cast_pixel_order": cases["surface_pixel_order"]["us"] / cases["cast_pixel_order"]["us"],
           "surface_over_gbuffer_raycast": cases["surface_pixel_order"]["us"] / cases["gbuffer_raycast"]["us"],
           "radiance_minus_surface_pixel_order_us": cases["radiance_pixel_order"]["us"] - cases["surface_pixel_order"]["us"]}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
