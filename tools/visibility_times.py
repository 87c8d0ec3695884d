"""Cost of hiding and showing submeshes with neb_gi_set_visibility on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes, six of
them drapes), and what a tree with emptied slots costs the rays against a tree built without the hidden submeshes.

  python tools/visibility_times.py [--out profiles/visibility_times.json] [--updates 50] [--warmup 5] [--triangles 262267]

The method of tools/refit_times.py: device time of one call between two events on the null stream and host time of the call itself (it
only enqueues), medians of `updates` calls after `warmup`, beside neb_gi_build_ms of the same scene in the same process and the wall
time of neb_gi_set_scene + neb_gi_build_bvh -- what making a submesh absent cost before.  Cases: hide one drape, show it again, hide
all six drapes, hide 102 of the 103 submeshes (each case timed as a hide / show pair: every timed call changes flags).
Tree quality: node visits of the bounce rays per traced ray (neb_gi_traversal_stats, one 1080p dispatch) for three trees -- everything
visible, the six drapes hidden, and a tree built from a scene whose drapes have empty index lists.  Reported, not gated.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_times.json"))
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
        raise SystemExit("visibility_times: no GPU visible")
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    n_geoms = len(sc.geometries)
    drapes = [i for i, g in enumerate(sc.geometries) if g["positions"].shape[0] == 49 * 41 and len(g["indices"]) == 6 * 48 * 40]
    if len(drapes) != 6:
        raise SystemExit(f"visibility_times: expected the stand-in's six drapes, found {len(drapes)}")

    def scene_without(indices):
        out = S.Scene(sc.name)
        out.materials, out.textures = sc.materials, sc.textures
        out.geometries = [dict(g) for g in sc.geometries]
        for i in indices:
            out.geometries[i]["indices"] = sc.geometries[i]["indices"][:0].copy()
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
    mine = scene_without([])
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

    def timed(indices, flag):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        h0 = time.perf_counter()
        r.set_visible(indices, flag, stream=0)
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, (h1 - h0) * 1e6

    cases = {}
    keep = n_geoms // 2
    for label, indices in (("one_drape", drapes[:1]), ("six_drapes", drapes), ("all_but_one", [i for i in range(n_geoms) if i != keep])):
        times = {False: ([], []), True: ([], [])}
        for k in range(args.warmup + args.updates):
            for flag in (False, True):
                dev, host = timed(indices, flag)
                if k >= args.warmup:
                    times[flag][0].append(dev)
                    times[flag][1].append(host)
        n_tris = sum(len(sc.geometries[i]["indices"]) // 3 for i in indices)
        for flag, name in ((False, "hide_"), (True, "show_")):
            dev, host = times[flag]
            cases[name + label] = {"submeshes": len(indices), "triangles": n_tris, "device_us": float(np.median(dev)),
                                   "device_p10_p90_us": [float(np.percentile(dev, 10)), float(np.percentile(dev, 90))],
                                   "host_us": float(np.median(host)), "device_over_build": float(np.median(dev)) / (build_ms * 1e3)}
    assert r.visibility().all()

    quality = {"all_visible": visits_per_ray(r, mine)}
    r.set_visible(drapes, False, stream=0)
    quality["six_drapes_hidden"] = visits_per_ray(r, mine)
    r.set_visible(drapes, True, stream=0)
    quality["shown_again"] = visits_per_ray(r, mine)
    fresh = DeferredRenderer()
    fresh.init(W, H, atrous_levels=5)
    quality["built_without_the_drapes"] = visits_per_ray(fresh, scene_without(drapes))
    fresh.destroy()
    quality["hidden_over_built_without"] = quality["six_drapes_hidden"] / quality["built_without_the_drapes"]

    out = {"what": "neb_gi_set_visibility on the sponza stand-in; device times between events, medians; bounce-ray node visits per traced ray",
           "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "drapes": drapes, "build_ms": build_ms, "rebuild_wall_ms": rebuild_wall_ms,
           "cases": cases, "bounce_node_visits_per_ray": quality}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
