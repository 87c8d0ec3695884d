"""Cost of moving submeshes with neb_gi_update_transforms on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes).

  python tools/refit_times.py [--out profiles/refit_times.json] [--updates 50] [--warmup 5] [--triangles 262267]

For 1, 10 and all submeshes moved it records
  * update_device_us: device time of one update between two events on the null stream (median of `updates`, after `warmup`);
  * update_host_us:   host time of the call itself (it only enqueues);
  * build_ms:         neb_gi_build_ms of the same scene in the same process, and rebuild_wall_ms: the wall time of
                      neb_gi_set_scene + neb_gi_build_bvh -- what moving a submesh cost before.
And the loss in tree quality: node visits of the bounce rays per traced ray (neb_gi_traversal_stats, one 1080p dispatch) of the refitted tree against a
tree built from the moved scene, after a small move (every tenth submesh by 5 cm) and after a move across the scene (by 8 m).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_times.json"))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("refit_times: no GPU visible")
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    n_geoms = len(sc.geometries)
    base = [g["M"].astype(np.float64) for g in sc.geometries]

    def shifted(indices, shift):
        T = np.eye(4)
        T[3, :3] = shift
        return np.stack([(base[i] @ T).astype(np.float32) for i in indices])

    def scene_with(indices, mats):
        out = S.Scene(sc.name)
        out.materials, out.textures = sc.materials, sc.textures
        out.geometries = [dict(g) for g in sc.geometries]
        for i, m in zip(indices, mats):
            out.geometries[i]["M"] = m
        return out

    def visits_per_ray(r, scene):
        r.begin_frame(RenderInfo(scene=scene, camera=cam, frame_index=7))
        r.set_debug_hits(True)  # (the option belongs to the scene: set once there is one)
        r.submit_commands_gbuffer()
        r.ray_count(reset=True)
        r.submit_commands_gi_pathtrace()
        r.ray_count()
        st = r.traversal_stats()
        r.end_frame()
        r.set_debug_hits(False)
        return st["bounce_nodes"] / max(st["rays"], 1)

    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    mine = scene_with([], [])
    t0 = time.perf_counter()
    r.begin_frame(RenderInfo(scene=mine, camera=cam, frame_index=1))  # neb_gi_set_scene + neb_gi_build_bvh
    torch.cuda.synchronize()
    rebuild_wall_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    r.init_pathtracer_scene(mine)  # (a second time: the first also paid for the process's one-off state)
    torch.cuda.synchronize()
    rebuild_wall_ms = min(rebuild_wall_ms, (time.perf_counter() - t0) * 1e3)
    build_ms = r.build_ms()
    tris, nodes = r.scene_info()

    cases = {}
    for label, indices in (("1", [n_geoms // 2]), ("10", list(range(0, n_geoms, max(1, n_geoms // 10)))[:10]), ("all", list(range(n_geoms)))):
        dev, host = [], []
        for k in range(args.warmup + args.updates):
            mats = shifted(indices, (0.01 * (k % 7 + 1), 0.0, 0.005 * (k % 3)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            h0 = time.perf_counter()
            r.update_transforms(indices, mats, stream=0)
            h1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1) * 1e3)
                host.append((h1 - h0) * 1e6)
        moved_tris = sum(len(sc.geometries[i]["indices"]) // 3 for i in indices)
        cases[label] = {"submeshes": len(indices), "triangles_moved": moved_tris, "update_device_us": float(np.median(dev)),
                        "update_device_p10_p90_us": [float(np.percentile(dev, 10)), float(np.percentile(dev, 90))],
                        "update_host_us": float(np.median(host)), "device_over_build": float(np.median(dev)) / (build_ms * 1e3)}
        r.update_transforms(indices, np.stack([base[i].astype(np.float32) for i in indices]), stream=0)

    quality = {}
    some = list(range(0, n_geoms, 10))
    for label, shift in (("small_move_5cm", (0.05, 0.0, 0.03)), ("across_the_scene_8m", (8.0, 0.0, 3.0))):
        mats = shifted(some, shift)
        r.update_transforms(some, mats, stream=0)
        refit = visits_per_ray(r, mine)
        fresh = DeferredRenderer()
        fresh.init(W, H, atrous_levels=5)
        built_scene = scene_with(some, mats)
        rebuilt = visits_per_ray(fresh, built_scene)
        fresh.destroy()
        quality[label] = {"submeshes": len(some), "bounce_node_visits_per_ray_refit": refit, "bounce_node_visits_per_ray_rebuilt": rebuilt,
                          "ratio": refit / rebuilt}
        r.update_transforms(some, np.stack([base[i].astype(np.float32) for i in some]), stream=0)
    quality["restored"] = {"bounce_node_visits_per_ray_refit": visits_per_ray(r, mine)}

    out = {"what": "neb_gi_update_transforms on the sponza stand-in; device times between events, medians",
           "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "build_ms": build_ms, "rebuild_wall_ms": rebuild_wall_ms,
           "cases": cases, "tree_quality": quality}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
