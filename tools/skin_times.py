"""Cost of skinning submeshes with neb_gi_skin_vertices on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes, six of them
drapes), against the route that existed before it.

  python tools/skin_times.py [--out profiles/skin_times.json] [--updates 50] [--warmup 5] [--triangles 262267]

The method of tools/deform_times.py: 1080p context, medians of `updates` calls between two events on the null stream after `warmup`, in
the same process as the build, the library's build id recorded.  Submeshes are skinned with 4 joints each -- the skins and poses of
the tests (tests/skin_ref.py: overlapping hat weights of the height, four non-zero influences on four joints; rotations of 10 .. 25
degrees plus a translation per joint) --, as one drape, all six drapes, and every submesh.  Per case, two arms:
  (a) skin:        neb_gi_skin_vertices -- the palettes go in, the library blends from the bind pose into the pools;
  (b) torch_route: what a host could do before, done well: ONE batched torch expression over all the case's vertices (the same linear
                   blend: gather four matrices per vertex, weight, sum, transform positions, normals and tangents) writes the skinned
                   arrays to device tensors, then ONE neb_gi_update_vertices_device reads them.  Joints (already offset into the
                   case's concatenated palette), weights and bind pose are resident tensors; the case's palettes are uploaded inside
                   the timed region in one non-blocking copy from pinned memory, as arm (a) uploads its own.
Each arm records the device interval and the host time of the call(s).  Reported, not gated.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # skin_ref: one definition of the skins and poses for the tests and this tool

N_JOINTS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_times.json"))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    args = ap.parse_args()

    import numpy as np
    import torch

    import skin_ref
    from bench import library_build_id
    from nebulae_amd import _lib, scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("skin_times: no GPU visible")
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    n_geoms = len(sc.geometries)
    drapes = [i for i, g in enumerate(sc.geometries) if g["positions"].shape[0] == 49 * 41 and len(g["indices"]) == 6 * 48 * 40]
    if len(drapes) != 6:
        raise SystemExit(f"skin_times: expected the stand-in's six drapes, found {len(drapes)}")

    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))  # neb_gi_set_scene + neb_gi_build_bvh
    torch.cuda.synchronize()
    build_ms = r.build_ms()
    tris, nodes = r.scene_info()

    skins = {gi: skin_ref.hat_skin(g["positions"], N_JOINTS) for gi, g in enumerate(sc.geometries)}
    valid = {gi: all(g[k] is not None for k in ("normals", "uvs", "tangents")) for gi, g in enumerate(sc.geometries)}

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

    cases = {}
    for label, indices in (("one_drape", drapes[:1]), ("all_drapes", drapes), ("every_submesh", list(range(n_geoms)))):
        r.init_pathtracer_scene(sc)  # (a fresh build: no submesh is stale, no skin is bound when a case starts)
        torch.cuda.synchronize()
        palettes = [[skin_ref.pose(sc.geometries[gi]["positions"], N_JOINTS, k) for gi in indices] for k in range(2)]
        row = {"submeshes": len(indices), "vertices": int(sum(sc.geometries[i]["positions"].shape[0] for i in indices)),
               "triangles_skinned": int(sum(len(sc.geometries[i]["indices"]) // 3 for i in indices)), "joints_per_submesh": N_JOINTS}
        # (b) first, on the unskinned context: one batched torch blend, one neb_gi_update_vertices_device
        counts = [sc.geometries[gi]["positions"].shape[0] for gi in indices]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        cat = lambda key, width: np.concatenate([sc.geometries[gi][key] if valid[gi] else np.zeros((n, width), np.float32) for gi, n in zip(indices, counts)])
        q = dict(j=torch.from_numpy(np.concatenate([skins[gi][0].astype(np.int64) + N_JOINTS * k for k, gi in enumerate(indices)])).cuda(),
                 w=torch.from_numpy(np.concatenate([skins[gi][1] for gi in indices])).cuda(),
                 p=torch.from_numpy(np.concatenate([sc.geometries[gi]["positions"] for gi in indices])).cuda(),
                 n=torch.from_numpy(cat("normals", 3)).cuda(), t=torch.from_numpy(cat("tangents", 4)).cuda())
        o = dict(p=torch.empty_like(q["p"]), n=torch.empty_like(q["n"]), t=q["t"].clone())  # (.w of the tangents never changes)
        pinned = [torch.from_numpy(np.concatenate(palettes[k])).pin_memory() for k in range(2)]
        J = torch.empty(tuple(pinned[0].shape), dtype=torch.float32, device="cuda")
        arr = (_lib.VertexUpdate * len(indices))()
        for u, gi, first, n in zip(arr, indices, starts, counts):
            u.geometry, u.firstVertex, u.numVertices = gi, 0, n
            u.positions, u.positionStride = o["p"].data_ptr() + 12 * int(first), 12
            if valid[gi]:
                u.normals, u.normalStride = o["n"].data_ptr() + 12 * int(first), 12
                u.tangents, u.tangentStride = o["t"].data_ptr() + 16 * int(first), 16

        def torch_route(k):
            J.copy_(pinned[k % 2], non_blocking=True)
            Sm = (q["w"][:, :, None, None] * J[q["j"]]).sum(1)  # n x 4 x 4
            R = Sm[:, :3, :3]
            torch.add(torch.einsum("nr,nrc->nc", q["p"], R), Sm[:, 3, :3], out=o["p"])
            o["n"].copy_(torch.einsum("nr,nrc->nc", q["n"], R))
            o["t"][:, :3].copy_(torch.einsum("nr,nrc->nc", q["t"][:, :3], R))
            r._check(r._lib.neb_gi_update_vertices_device(r._ctx, arr, len(arr), C.c_void_p(0)), "neb_gi_update_vertices_device")

        row["torch_route"] = timed(torch_route)
        # (a) the library's skinning, from the bind pose the scene was set with
        r.init_pathtracer_scene(sc)
        descs = (_lib.SkinDesc * len(indices))()
        for d, gi in zip(descs, indices):
            j, w = skins[gi]
            d.geometry, d.numJoints, d.joints, d.jointStride, d.weights, d.weightStride = gi, N_JOINTS, j.ctypes.data, 8, w.ctypes.data, 16
        r._check(r._lib.neb_gi_set_skin(r._ctx, descs, len(indices), C.c_void_p(0)), "neb_gi_set_skin")
        ups = [(_lib.SkinUpdate * len(indices))() for _ in range(2)]
        for k in range(2):
            for u, gi, pal in zip(ups[k], indices, palettes[k]):
                u.geometry, u.jointMatrices = gi, pal.ctypes.data_as(C.POINTER(C.c_float))
        torch.cuda.synchronize()
        row["skin"] = timed(lambda k: r._check(r._lib.neb_gi_skin_vertices(r._ctx, ups[k % 2], len(indices), C.c_void_p(0)), "neb_gi_skin_vertices"))
        row["skin_over_torch_route_device"] = row["skin"]["update_device_us"] / row["torch_route"]["update_device_us"]
        row["status"] = r.update_status()
        cases[label] = row

    out = {"what": "neb_gi_skin_vertices on the sponza stand-in against one batched torch blend + one neb_gi_update_vertices_device; device times between events, medians",
           "updates_per_case": args.updates, "warmup": args.warmup, "build_id": library_build_id(), "device": torch.cuda.get_device_name(0),
           "triangles": tris, "nodes": nodes, "submeshes": n_geoms, "drapes": drapes, "build_ms": build_ms, "cases": cases}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.destroy()


if __name__ == "__main__":
    main()
