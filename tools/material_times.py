"""Cost of changing what submeshes look like in place -- neb_gi_update_materials, neb_gi_set_geometry_materials, neb_gi_update_textures and
neb_gi_update_textures_device -- on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes, 25 materials, 69 maps of 1024^2),
against what the same change cost before: neb_gi_set_scene + neb_gi_build_bvh, measured in the same run.

  python tools/material_times.py [--out profiles/material_times.json] [--updates 30] [--warmup 5] [--triangles 262267] [--tex-size 1024]

The method of tools/visibility_times.py: device time of one call between two events on the null stream and host time of the call itself (it
only enqueues; the host-sourced texel call also copies its rows into the pinned slot), medians of `updates` calls after `warmup`.  Every
timed call changes something: factor and assignment calls alternate between two states, texel calls between two images.
Cases: the factors of 1 and of all 25 materials; another material for 1 and for all 103 submeshes; all 1024^2 texels of a map that sits in
one bundle, and of the roughness-metalness map three materials share (three bundles); a 64 x 64 rectangle -- the texel cases from host
memory and from device memory.
For a full update of a bundled map the traffic cannot be less than: the source read once (4 B per texel), the bundle read and written
once (32 B each per texel position) per bundle.  The achieved bytes/s over that floor is reported beside each such case -- reported, not gated.
The JSON carries the library's build id (bench.library_build_id).  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_times.json"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    ap.add_argument("--tex-size", type=int, default=1024)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("material_times: no GPU visible")
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles, tex_size=args.tex_size)
    cam = S.sponza_camera()
    n_geoms, n_mats, ts = len(sc.geometries), len(sc.materials), args.tex_size

    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    t0 = time.perf_counter()
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))  # neb_gi_set_scene + neb_gi_build_bvh
    torch.cuda.synchronize()
    rebuild_wall_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    r.init_pathtracer_scene(sc)  # (a second time: the first also paid for the process's one-off state)
    torch.cuda.synchronize()
    rebuild_wall_ms = min(rebuild_wall_ms, (time.perf_counter() - t0) * 1e3)
    build_ms = r.build_ms()
    tris, nodes = r.scene_info()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        h0 = time.perf_counter()
        call()
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, (h1 - h0) * 1e6

    def measure(calls):
        """calls: the two alternating states of one case"""
        dev, host = [], []
        for k in range(args.warmup + args.updates):
            d, h = timed(calls[k % 2])
            if k >= args.warmup:
                dev.append(d)
                host.append(h)
        return {"device_us": float(np.median(dev)), "device_p10_p90_us": [float(np.percentile(dev, 10)), float(np.percentile(dev, 90))],
                "host_us": float(np.median(host)), "device_over_rebuild": float(np.median(dev)) / (rebuild_wall_ms * 1e3)}

    rng = np.random.default_rng(1)
    cases = {}
    for label, mats in (("factors_1_material", [2]), (f"factors_all_{n_mats}_materials", list(range(n_mats)))):
        a = [rng.uniform(0.1, 0.9, (len(mats), 3)).astype(np.float32) for _ in range(2)]
        m = [rng.uniform(0.2, 1.0, (len(mats), 2)).astype(np.float32) for _ in range(2)]
        cases[label] = dict(measure([lambda k=k: r.update_materials(mats, albedo=a[k], rough_metal=m[k], stream=0) for k in range(2)]), materials=len(mats))
    base = [g["material"] for g in sc.geometries]
    for label, geoms in (("reassign_1_submesh", [n_geoms // 2]), (f"reassign_all_{n_geoms}_submeshes", list(range(n_geoms)))):
        to = [[base[g] for g in geoms], [(base[g] + 1) % n_mats for g in geoms]]
        cases[label] = dict(measure([lambda k=k: r.set_geometry_materials(geoms, to[k], stream=0) for k in (1, 0)]), submeshes=len(geoms))

    one_bundle = sc.materials[0]["textures"][0]   # the albedo map of material 0: one bundle
    shared_rm = sc.materials[14]["textures"][2]   # the roughness-metalness map of materials 14-16: three bundles
    n_bundles = {one_bundle: sum(1 for m in sc.materials if one_bundle in m["textures"] and min(m["textures"]) >= 0),
                 shared_rm: sum(1 for m in sc.materials if shared_rm in m["textures"] and min(m["textures"]) >= 0)}
    side = min(64, ts)
    for label, tex, x, y, w, h in ((f"texels_full_{ts}x{ts}_one_bundle", one_bundle, 0, 0, ts, ts), (f"texels_full_{ts}x{ts}_three_bundles", shared_rm, 0, 0, ts, ts),
                                   (f"texels_{side}x{side}_rectangle", one_bundle, ts // 3, ts // 5, side, side)):
        images = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2)]
        tensors = [torch.from_numpy(im).cuda() for im in images]
        torch.cuda.synchronize()
        for src, sources in (("host", images), ("device", tensors)):
            c = measure([lambda k=k: r.update_texture(tex, sources[k], x=x, y=y, stream=0, mirror=False) for k in range(2)])
            c.update(texture=tex, width=w, height=h, bundles=n_bundles[tex], source=src)
            if w == ts and h == ts:  # the floor: the source once, every bundle read and written once
                c["floor_bytes"] = 4 * w * h + n_bundles[tex] * 64 * w * h
                c["achieved_GBps_over_floor_bytes"] = c["floor_bytes"] / (c["device_us"] * 1e-6) / 1e9
            cases[f"{label}_{src}"] = c

    out = {"what": "materials and texels updated in place on the sponza stand-in; device times between events, medians; "
                   "rebuild_wall_ms = neb_gi_set_scene + neb_gi_build_bvh in the same run",
           "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "materials": n_mats, "textures": len(sc.textures), "tex_size": ts,
           "build_ms": build_ms, "rebuild_wall_ms": rebuild_wall_ms, "sun_table_builds": r.sun_table_stats()["builds"], "cases": cases}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
