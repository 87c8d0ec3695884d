"""Cost of neb_gi_cast_rays on the bench scene (sponza stand-in: 262 k triangles), DESIGN.md 3.8.

  python tools/ray_query_times.py [--out profiles/ray_query_times.json] [--calls 50] [--warmup 5] [--triangles 262267]

Device time of one call between two events on the null stream (median of `calls`, after `warmup`), for
  * primary_pixel_order:      the 1080p camera's 2.07 M primary rays in pixel order, closest hit;
  * primary_shuffled:         the same rays in a fixed random permutation, closest hit, unsorted and with NEB_RAYS_SORT;
  * sun_pixel_order / sun_shuffled: any-hit rays towards the sun from the primary hit points (pixels that see the sky carry a ray that
                              is not walked), unsorted and sorted;
  * sort_share_us:            what NEB_RAYS_SORT adds in front of the walk -- the key kernel and the radix sort -- taken as sorted minus
                              unsorted on the shuffled primary rays with tmax = 1e-30, whose walk ends in the boxes around the origin;
and, as the yardstick, gbuffer_raycast_us: neb_gbuffer_raycast in the same run and process -- the same walk over the same rays plus
shading, without 64 bytes per ray of ray and hit traffic.  The JSON carries the library's build id.  Needs a GPU; no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def primary_rays(cam, W, H):
    """the rays of neb_gbuffer_raycast (camera_basis of neb_internal.h), pixel order -> float32 [H * W, 8], tmin 0, tmax 1e30"""
    import math

    import numpy as np
    F = np.float32
    eye, tgt, up = [np.array(list(v), np.float64) for v in (cam.eye, cam.target, cam.up)]
    z = (eye - tgt) / np.linalg.norm(eye - tgt)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    tan_half = math.tan(math.radians(cam.vfov_deg) * 0.5)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ndc_x = (xs + 0.5) / W * 2.0 - 1.0
    ndc_y = 1.0 - (ys + 0.5) / H * 2.0
    d = x * (ndc_x * (W / H) * tan_half)[..., None] + y * (ndc_y * tan_half)[..., None] - z
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.empty((H * W, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = eye, 0.0, d.reshape(-1, 3), 1e30
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query_times.json"))
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

    if not torch.cuda.is_available():
        raise SystemExit("ray_query_times: no GPU visible")
    W, H = args.width, args.height
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))
    tris, nodes = r.scene_info()

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
    primary = torch.from_numpy(primary_rays(cam, W, H)).cuda()
    shuffled = primary[perm].contiguous()
    hits = r.cast_rays(primary)
    torch.cuda.synchronize()
    found = hits["geometry"] != -1
    # towards the sun from the hit points: the sun of the renderer's UI, tmin 1e-3 (in units of the unit direction), no far end
    to_sun = -torch.tensor(r.sun.direction, dtype=torch.float32, device="cuda")
    to_sun = to_sun / to_sun.norm()
    sun = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    sun[:, 0:3] = primary[:, 0:3] + primary[:, 4:7] * torch.where(found, hits["t"], torch.zeros_like(hits["t"]))[:, None]
    sun[:, 3] = 1e-3
    sun[:, 4:7] = torch.where(found[:, None], to_sun[None, :], torch.zeros(3, device="cuda")[None, :])  # (sky pixels: a zero direction, not walked)
    sun[:, 7] = float("inf")
    sun_shuffled = sun[perm].contiguous()
    stub = shuffled.clone()
    stub[:, 7] = 1e-30
    out_hits = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    out_words = torch.empty((n,), dtype=torch.int32, device="cuda")

    # the answers first: sorted == unsorted on the timed inputs, and the permutation only permutes
    a = r.cast_rays(shuffled)["records"].clone()
    b = r.cast_rays(shuffled, sort=True)["records"].clone()
    oa = r.cast_rays(sun_shuffled, any_hit=True)["occluded"].clone()
    ob = r.cast_rays(sun_shuffled, any_hit=True, sort=True)["occluded"].clone()
    torch.cuda.synchronize()
    same = bool((a.view(torch.int32) == b.view(torch.int32)).all()) and bool((oa == ob).all())
    same = same and bool((a.view(torch.int32) == hits["records"][perm].view(torch.int32)).all())
    if not same:
        raise SystemExit("ray_query_times: sorted and unsorted answers differ")

    cases = {}
    cases["gbuffer_raycast"] = timed(lambda: r.submit_commands_gbuffer())
    cases["primary_pixel_order"] = timed(lambda: r.cast_rays(primary, out=out_hits))
    cases["primary_shuffled"] = timed(lambda: r.cast_rays(shuffled, out=out_hits))
    cases["primary_shuffled_sorted"] = timed(lambda: r.cast_rays(shuffled, sort=True, out=out_hits))
    cases["primary_pixel_order_sorted"] = timed(lambda: r.cast_rays(primary, sort=True, out=out_hits))
    cases["sun_pixel_order"] = timed(lambda: r.cast_rays(sun, any_hit=True, out=out_words))
    cases["sun_pixel_order_sorted"] = timed(lambda: r.cast_rays(sun, any_hit=True, sort=True, out=out_words))
    cases["sun_shuffled"] = timed(lambda: r.cast_rays(sun_shuffled, any_hit=True, out=out_words))
    cases["sun_shuffled_sorted"] = timed(lambda: r.cast_rays(sun_shuffled, any_hit=True, sort=True, out=out_words))
    cases["stub_walk"] = timed(lambda: r.cast_rays(stub, out=out_hits))
    cases["stub_walk_sorted"] = timed(lambda: r.cast_rays(stub, sort=True, out=out_hits))
    cases["gbuffer_raycast_again"] = timed(lambda: r.submit_commands_gbuffer())
    sort_share = cases["stub_walk_sorted"]["us"] - cases["stub_walk"]["us"]

    out = {"what": "neb_gi_cast_rays on the sponza stand-in; device times of one call between events, medians",
           "calls_per_case": args.calls, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "width": W, "height": H, "rays": n, "primary_rays_that_hit": int(found.sum()),
           "sun_rays_occluded": int((oa != 0).sum()), "sorted_equals_unsorted": same, "cases": cases, "sort_share_us": sort_share,
           "gbuffer_raycast_us": cases["gbuffer_raycast"]["us"]}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
