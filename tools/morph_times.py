"""Cost of blending morph targets with neb_gi_morph_vertices on the bench scene (sponza stand-in: 262 k triangles, 103 submeshes, six of
them drapes), against the route that existed before it.

  python tools/morph_times.py [--out profiles/morph_times.json] [--updates 50] [--warmup 5] [--triangles 262267]

The method of tools/skin_times.py: 1080p context, medians of `updates` calls between two events on the null stream after `warmup`, in
the same process as the build, the library's build id recorded.  Every submesh of a case carries 4 targets with position, normal and
tangent deltas (smooth fields of the position; their values do not matter to the time), as one drape, all six drapes, and every
submesh, in three variants:
  all_active:   four non-zero weights per submesh;
  one_of_four:  one non-zero weight per submesh (target 1): the cost follows the active list;
  skinned:      four non-zero weights under a skin of 4 joints (tests/skin_ref.py's hat skins and poses): morph, then skin, one call.
Per case and variant, two arms:
  (a) morph:       neb_gi_morph_vertices -- weights (and palettes) go in, the library blends from the rest pose into the pools;
  (b) torch_route: what a host could do before, done well: ONE batched torch expression over all the case's vertices -- the resident
                   delta tensors of the ACTIVE targets only, weighted per vertex through a resident submesh index, summed onto the rest
                   pose; under a skin followed by skin_times' batched linear blend -- writes device tensors, then ONE
                   neb_gi_update_vertices_device reads them.  The case's weights (and palettes) are uploaded inside the timed region in
                   one non-blocking copy each from pinned memory, as arm (a) uploads its own.
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

N_TARGETS, N_JOINTS = 4, 4
VARIANTS = {"all_active": ([0, 1, 2, 3], False), "one_of_four": ([1], False), "skinned": ([0, 1, 2, 3], True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_times.json"))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262267)
    ap.add_argument("--only", default=None, help="case/variant/arm, e.g. every_submesh/all_active/morph: that one arm alone (for a kernel trace)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import skin_ref
    from bench import library_build_id
    from nebulae_amd import _lib, scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo

    if not torch.cuda.is_available():
        raise SystemExit("morph_times: no GPU visible")
    F = np.float32
    W, H = 1920, 1080
    sc = S.atrium_standin(target_triangles=args.triangles)
    cam = S.sponza_camera()
    n_geoms = len(sc.geometries)
    drapes = [i for i, g in enumerate(sc.geometries) if g["positions"].shape[0] == 49 * 41 and len(g["indices"]) == 6 * 48 * 40]
    if len(drapes) != 6:
        raise SystemExit(f"morph_times: expected the stand-in's six drapes, found {len(drapes)}")

    r = DeferredRenderer()
    r.init(W, H, atrous_levels=5)
    r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=1))  # neb_gi_set_scene + neb_gi_build_bvh
    torch.cuda.synchronize()
    build_ms = r.build_ms()
    tris, nodes = r.scene_info()

    valid = {gi: all(g[k] is not None for k in ("normals", "uvs", "tangents")) for gi, g in enumerate(sc.geometries)}
    skins = {gi: skin_ref.hat_skin(g["positions"], N_JOINTS) for gi, g in enumerate(sc.geometries)}

    def targets(gi):
        """T x n x 3 position, normal and tangent deltas: two per cent of the box's diagonal along the normal, a tenth of a unit for the directions"""
        g = sc.geometries[gi]
        P = g["positions"].astype(np.float64)
        N = g["normals"].astype(np.float64) if g["normals"] is not None else np.tile([0.0, 1.0, 0.0], (len(P), 1))
        diag = float(np.linalg.norm(P.max(0) - P.min(0)))
        h = skin_ref.height(P)
        dP = np.stack([0.02 * diag * np.sin(np.pi * (k + 1) * h + 0.7 * k)[:, None] * N for k in range(N_TARGETS)])
        dN = np.stack([0.1 * np.cos(np.pi * (k + 1) * h + 0.3 * k)[:, None] * np.roll(N, 1 + k % 2, axis=1) for k in range(N_TARGETS)])
        return np.ascontiguousarray(dP, F), np.ascontiguousarray(dN, F), np.ascontiguousarray(-dN[:, :, ::-1], F)

    deltas = {gi: targets(gi) for gi in range(n_geoms)}

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

    fp = C.POINTER(C.c_float)
    cases = {}
    for label, indices in (("one_drape", drapes[:1]), ("all_drapes", drapes), ("every_submesh", list(range(n_geoms)))):
        counts = [sc.geometries[gi]["positions"].shape[0] for gi in indices]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        row = {"submeshes": len(indices), "vertices": int(sum(counts)), "triangles_morphed": int(sum(len(sc.geometries[i]["indices"]) // 3 for i in indices)),
               "targets_per_submesh": N_TARGETS}
        cat = lambda key, width: np.concatenate([sc.geometries[gi][key] if valid[gi] else np.zeros((n, width), F) for gi, n in zip(indices, counts)])
        for variant, (active, skinned) in VARIANTS.items():
            only = args.only.split("/") if args.only else None
            if only and only[:2] != [label, variant]:
                continue
            # two weight sets per submesh, zero where the variant leaves a target out; two poses
            weights = [np.zeros((len(indices), N_TARGETS), F) for _ in range(2)]
            for k in range(2):
                for a in active:
                    weights[k][:, a] = [0.3 + 0.5 * (((a + 1) * 0.37 + 0.11 * i + 0.29 * k) % 1.0) for i in range(len(indices))]
            palettes = [[skin_ref.pose(sc.geometries[gi]["positions"], N_JOINTS, k) for gi in indices] for k in range(2)]
            out = {"active_targets": len(active), "joints_per_submesh": N_JOINTS if skinned else 0}
            if not only or only[2] == "torch_route":
                # (b) first, on a context without targets: one batched torch expression, one neb_gi_update_vertices_device
                r.init_pathtracer_scene(sc)
                torch.cuda.synchronize()
                q = dict(p=torch.from_numpy(np.concatenate([sc.geometries[gi]["positions"] for gi in indices])).cuda(),
                         n=torch.from_numpy(cat("normals", 3)).cuda(), t=torch.from_numpy(cat("tangents", 4)).cuda(),
                         g=torch.from_numpy(np.repeat(np.arange(len(indices)), counts)).cuda(),
                         j=torch.from_numpy(np.concatenate([skins[gi][0].astype(np.int64) + N_JOINTS * k for k, gi in enumerate(indices)])).cuda(),
                         w=torch.from_numpy(np.concatenate([skins[gi][1] for gi in indices])).cuda())
                d = [torch.from_numpy(np.ascontiguousarray(np.concatenate([deltas[gi][s] for gi in indices], axis=1)[active])).cuda() for s in range(3)]
                o = dict(p=torch.empty_like(q["p"]), n=torch.empty_like(q["n"]), t=q["t"].clone())  # (.w of the tangents never changes)
                pin_w = [torch.from_numpy(np.ascontiguousarray(weights[k][:, active].T)).pin_memory() for k in range(2)]  # active x submeshes
                Wd = torch.empty(tuple(pin_w[0].shape), dtype=torch.float32, device="cuda")
                pin_j = [torch.from_numpy(np.concatenate(palettes[k])).pin_memory() for k in range(2)]
                J = torch.empty(tuple(pin_j[0].shape), dtype=torch.float32, device="cuda")
                arr = (_lib.VertexUpdate * len(indices))()
                for u, gi, first, n in zip(arr, indices, starts, counts):
                    u.geometry, u.firstVertex, u.numVertices = gi, 0, n
                    u.positions, u.positionStride = o["p"].data_ptr() + 12 * int(first), 12
                    if valid[gi]:
                        u.normals, u.normalStride = o["n"].data_ptr() + 12 * int(first), 12
                        u.tangents, u.tangentStride = o["t"].data_ptr() + 16 * int(first), 16

                def torch_route(k, q=q, d=d, o=o, pin_w=pin_w, Wd=Wd, pin_j=pin_j, J=J, arr=arr, skinned=skinned):
                    Wd.copy_(pin_w[k % 2], non_blocking=True)
                    Wv = Wd[:, q["g"]]  # active x vertices
                    m = q["p"] + torch.einsum("kn,knc->nc", Wv, d[0])
                    n = q["n"] + torch.einsum("kn,knc->nc", Wv, d[1])
                    t = q["t"][:, :3] + torch.einsum("kn,knc->nc", Wv, d[2])
                    if skinned:
                        J.copy_(pin_j[k % 2], non_blocking=True)
                        Sm = (q["w"][:, :, None, None] * J[q["j"]]).sum(1)  # n x 4 x 4
                        R = Sm[:, :3, :3]
                        torch.add(torch.einsum("nr,nrc->nc", m, R), Sm[:, 3, :3], out=o["p"])
                        o["n"].copy_(torch.einsum("nr,nrc->nc", n, R))
                        o["t"][:, :3].copy_(torch.einsum("nr,nrc->nc", t, R))
                    else:
                        o["p"].copy_(m), o["n"].copy_(n), o["t"][:, :3].copy_(t)
                    r._check(r._lib.neb_gi_update_vertices_device(r._ctx, arr, len(arr), C.c_void_p(0)), "neb_gi_update_vertices_device")

                out["torch_route"] = timed(torch_route)
            if not only or only[2] == "morph":
                # (a) the library's blend, from the rest pose the scene was set with
                r.init_pathtracer_scene(sc)
                keep = []
                descs = (_lib.MorphDesc * len(indices))()
                for dsc, gi in zip(descs, indices):
                    dsc.geometry, dsc.numTargets, dsc.positionStride, dsc.normalStride, dsc.tangentStride = gi, N_TARGETS, 12, 12, 12
                    for key, a in zip(("positionDeltas", "normalDeltas", "tangentDeltas"), deltas[gi] if valid[gi] else deltas[gi][:1]):
                        p = (C.c_void_p * N_TARGETS)(*[a[t].ctypes.data for t in range(N_TARGETS)])
                        keep.append(p)
                        setattr(dsc, key, p)
                r._check(r._lib.neb_gi_set_morph_targets(r._ctx, descs, len(indices), C.c_void_p(0)), "neb_gi_set_morph_targets")
                if skinned:
                    sk = (_lib.SkinDesc * len(indices))()
                    for s, gi in zip(sk, indices):
                        j, w = skins[gi]
                        s.geometry, s.numJoints, s.joints, s.jointStride, s.weights, s.weightStride = gi, N_JOINTS, j.ctypes.data, 8, w.ctypes.data, 16
                    r._check(r._lib.neb_gi_set_skin(r._ctx, sk, len(indices), C.c_void_p(0)), "neb_gi_set_skin")
                ups = [(_lib.MorphUpdate * len(indices))() for _ in range(2)]
                for k in range(2):
                    for i, (u, gi) in enumerate(zip(ups[k], indices)):
                        u.geometry, u.weights = gi, weights[k][i].ctypes.data_as(fp)
                        if skinned:
                            u.jointMatrices = palettes[k][i].ctypes.data_as(fp)
                torch.cuda.synchronize()
                out["morph"] = timed(lambda k, ups=ups: r._check(r._lib.neb_gi_morph_vertices(r._ctx, ups[k % 2], len(indices), C.c_void_p(0)),
                                                                   "neb_gi_morph_vertices"))
                out["status"] = r.update_status()
            if "morph" in out and "torch_route" in out:
                out["morph_over_torch_route_device"] = out["morph"]["update_device_us"] / out["torch_route"]["update_device_us"]
            row[variant] = out
        cases[label] = row

    out = {"what": "neb_gi_morph_vertices on the sponza stand-in against one batched torch expression + one neb_gi_update_vertices_device; "
                   "device times between events, medians",
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
