"""Cost of deforming submeshes with neb_gi_update_vertices on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes, six of
them drapes), and what a refitted tree loses against a rebuilt one.

  python tools/deform_times.py [--out profiles/deform_times.json] [--device-out profiles/deform_device_times.json] [--updates 50]
                               [--warmup 5] [--triangles 262267]

For one drape, all drapes and every submesh -- one call each, positions + normals, a sine displacement along the normal with the normals
recomputed from the deformed grid -- it records, for both arms of option "gi_deform_stage" (0: the scatter kernel reads the pinned staging,
1: one hipMemcpyAsync to a device buffer first),
  * update_device_us: device time of one update between two events on the null stream (median of `updates`, after `warmup`);
  * update_host_us:   host time of the call itself (it copies the arrays into the staging and enqueues);
  * build_ms:         neb_gi_build_ms of the same scene in the same process, and rebuild_wall_ms: the wall time of
                      neb_gi_set_scene + neb_gi_build_bvh -- what deforming a submesh cost before.
And the loss in tree quality: node visits of the bounce rays per traced ray (neb_gi_traversal_stats, one 1080p dispatch) of the refitted
tree against a tree built from the deformed scene, for a sine wave on the drapes of 3 cm and of 1 m amplitude.  Reported, not gated.
A third arm, written to --device-out: the same three cases through neb_gi_update_vertices_device, the sources resident in device memory
(uploaded once, outside the timed region) -- device interval and host time of the call beside the pinned arm's of this very run and the
figures recorded before the device path existed.  And the all-submesh neb_gi_update_transforms of tools/refit_times.py twice: with the
host's per-vertex box walk, and, after one device-sourced update has made every submesh's host positions stale, with the boxes reduced on
the device.  An empty --out or --device-out writes no file.
The JSON carries the library's build id (bench.library_build_id).  Needs a GPU; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNIT = 0.00800000037997961  # world units per object unit of the stand-in (its node scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_times.json"))
    ap.add_argument("--device-out", default=os.path.join(ROOT, "profiles", "deform_device_times.json"))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import _lib, scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("deform_times: no GPU visible")
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    n_geoms = len(sc.geometries)
    # the drapes: the only submeshes on 48 x 40 grids (scene.atrium_standin)
    drapes = [i for i, g in enumerate(sc.geometries) if g["positions"].shape[0] == 49 * 41 and len(g["indices"]) == 6 * 48 * 40]
    if len(drapes) != 6:
        raise SystemExit(f"deform_times: expected the stand-in's six drapes, found {len(drapes)}")

    def deformed(gi, amplitude, phase):
        """sine displacement along the normal (object units), normals recomputed from the deformed grid"""
        g = sc.geometries[gi]
        P, N0 = g["positions"].astype(np.float64), g["normals"].astype(np.float64)
        d = amplitude * np.sin(2.0 * math.pi / 130.0 * (P @ np.array([0.55, 1.0, 0.35])) + phase)
        P = P + d[:, None] * N0
        tri = g["indices"].reshape(-1, 3).astype(np.int64)
        fn = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
        N = np.zeros_like(P)
        for k in range(3):
            np.add.at(N, tri[:, k], fn)
        N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-30)
        N *= np.where(np.sum(N * N0, axis=1, keepdims=True) < 0.0, -1.0, 1.0)
        return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(N, np.float32)

    def entries(indices, amplitude, phase):
        arrays = [deformed(gi, amplitude, phase) for gi in indices]
        arr = (_lib.VertexUpdate * len(indices))()
        for u, gi, (P, N) in zip(arr, indices, arrays):
            u.geometry, u.firstVertex, u.numVertices = gi, 0, P.shape[0]
            u.positions, u.positionStride, u.normals, u.normalStride = P.ctypes.data, 12, N.ctypes.data, 12
        return arr, arrays

    def original(indices):
        arr = (_lib.VertexUpdate * len(indices))()
        for u, gi in zip(arr, indices):
            g = sc.geometries[gi]
            u.geometry, u.firstVertex, u.numVertices = gi, 0, g["positions"].shape[0]
            u.positions, u.positionStride, u.normals, u.normalStride = g["positions"].ctypes.data, 12, g["normals"].ctypes.data, 12
        return arr

    def send(r, arr):
        r._check(r._lib.neb_gi_update_vertices(r._ctx, arr, len(arr), C.c_void_p(0)), "neb_gi_update_vertices")

    def scene_with(indices, arrays):
        out = S.Scene(sc.name)
        out.materials, out.textures = sc.materials, sc.textures
        out.geometries = [dict(g) for g in sc.geometries]
        for gi, (P, N) in zip(indices, arrays):
            out.geometries[gi]["positions"], out.geometries[gi]["normals"] = P, N
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
    for label, indices in (("one_drape", drapes[:1]), ("all_drapes", drapes), ("every_submesh", list(range(n_geoms)))):
        poses = [entries(indices, 3.0 + k, 0.9 * k) for k in range(2)]
        row = {"submeshes": len(indices), "vertices": int(sum(sc.geometries[i]["positions"].shape[0] for i in indices)),
               "triangles_deformed": int(sum(len(sc.geometries[i]["indices"]) // 3 for i in indices)), "streams": "positions + normals"}
        for arm, name in ((0, "pinned"), (1, "device_copy")):
            r.svgf.set_option("gi_deform_stage", arm)
            dev, host = [], []
            for k in range(args.warmup + args.updates):
                arr = poses[k % 2][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                h0 = time.perf_counter()
                send(r, arr)
                h1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    dev.append(e0.elapsed_time(e1) * 1e3)
                    host.append((h1 - h0) * 1e6)
            row[name] = {"update_device_us": float(np.median(dev)), "update_device_p10_p90_us": [float(np.percentile(dev, 10)), float(np.percentile(dev, 90))],
                         "update_host_us": float(np.median(host)), "device_over_build": float(np.median(dev)) / (build_ms * 1e3)}
        r.svgf.set_option("gi_deform_stage", 0)
        cases[label] = row
        send(r, original(indices))

    quality = {}
    for label, metres in (("drape_sine_3cm", 0.03), ("drape_sine_1m", 1.0)):
        arr, arrays = entries(drapes, metres / UNIT, 0.3)
        send(r, arr)
        refit = visits_per_ray(r, mine)
        fresh = DeferredRenderer()
        fresh.init(W, H, atrous_levels=5)
        rebuilt = visits_per_ray(fresh, scene_with(drapes, arrays))
        fresh.destroy()
        quality[label] = {"submeshes": len(drapes), "amplitude_m": metres, "bounce_node_visits_per_ray_refit": refit,
                          "bounce_node_visits_per_ray_rebuilt": rebuilt, "ratio": refit / rebuilt}
        send(r, original(drapes))
    quality["restored"] = {"bounce_node_visits_per_ray_refit": visits_per_ray(r, mine)}

    # ---- the third arm: sources resident in device memory (a fresh build first: no submesh is stale when an arm starts) ----
    def timed(fn):
        dev, host = [], []
        for k in range(args.warmup + args.updates):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            h0 = time.perf_counter()
            fn(k)
            h1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1) * 1e3)
                host.append((h1 - h0) * 1e6)
        return {"update_device_us": float(np.median(dev)), "update_device_p10_p90_us": [float(np.percentile(dev, 10)), float(np.percentile(dev, 90))],
                "update_host_us": float(np.median(host)), "device_over_build": float(np.median(dev)) / (build_ms * 1e3)}

    def device_entries(indices, amplitude, phase):
        tensors = [tuple(torch.from_numpy(a).cuda() for a in deformed(gi, amplitude, phase)) for gi in indices]
        arr = (_lib.VertexUpdate * len(indices))()
        for u, gi, (P, N) in zip(arr, indices, tensors):
            u.geometry, u.firstVertex, u.numVertices = gi, 0, P.shape[0]
            u.positions, u.positionStride, u.normals, u.normalStride = P.data_ptr(), 12, N.data_ptr(), 12
        return arr, tensors

    def send_device(arr):
        r._check(r._lib.neb_gi_update_vertices_device(r._ctx, arr, len(arr), C.c_void_p(0)), "neb_gi_update_vertices_device")

    recorded = {"one_drape": (116, 87), "all_drapes": (226, 182), "every_submesh": (1541, 1417)}  # profiles/deform_times.json before the device path
    device_cases = {}
    if args.device_out:
        everything = list(range(n_geoms))
        base = [sc.geometries[i]["M"].astype(np.float32) for i in everything]
        idx = np.arange(n_geoms, dtype=np.uint32)
        shift = [np.stack(base) for _ in range(2)]
        for k in range(2):
            shift[k][:, 3, 0] += np.float32(0.01 * (k + 1))  # every submesh 1 / 2 cm along x
        moves = lambda k: r.update_transforms(idx, shift[k % 2], stream=0)
        r.init_pathtracer_scene(mine)
        torch.cuda.synchronize()
        transforms = {"submeshes": n_geoms, "host_box_walk": timed(moves)}
        for label, indices in (("one_drape", drapes[:1]), ("all_drapes", drapes), ("every_submesh", everything)):
            r.init_pathtracer_scene(mine)
            poses = [device_entries(indices, 3.0 + k, 0.9 * k) for k in range(2)]
            torch.cuda.synchronize()
            row = {k: v for k, v in cases[label].items() if k not in ("pinned", "device_copy")}
            row["device_sources"] = timed(lambda k: send_device(poses[k % 2][0]))
            row["host_sources_pinned_same_run"] = cases[label]["pinned"]
            row["host_sources_pinned_recorded_before"] = {"update_device_us": recorded[label][0], "update_host_us": recorded[label][1]}
            device_cases[label] = row
        # (every submesh has just been updated from device memory: all 103 are stale)
        transforms["device_reduced_boxes"] = timed(moves)
        transforms["status"] = r.update_status()
        out_dev = {"what": "neb_gi_update_vertices_device on the sponza stand-in, sources resident in device memory; device times between events, medians; "
                           "beside the host-sourced pinned arm of the same run",
                   "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
                   "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "drapes": drapes, "build_ms": build_ms,
                   "cases": device_cases, "update_transforms_every_submesh": transforms}
        print(json.dumps(out_dev, indent=1))
        os.makedirs(os.path.dirname(os.path.abspath(args.device_out)), exist_ok=True)
        with open(args.device_out, "w") as f:
            json.dump(out_dev, f, indent=1)

    out = {"what": "neb_gi_update_vertices on the sponza stand-in; device times between events, medians; both arms of gi_deform_stage",
           "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "drapes": drapes, "build_ms": build_ms, "rebuild_wall_ms": rebuild_wall_ms,
           "cases": cases, "tree_quality": quality}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
