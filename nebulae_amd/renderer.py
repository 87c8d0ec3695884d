"""Host-side mirror of the GI + SVGF portion of the reference's ``Neb::DeferredRenderer``.

Names follow /root/reference/src/DeferredRenderer.h:45-81 (snake_case): ``init``, ``begin_frame``
(with a ``RenderInfo``), ``submit_commands_gi_pathtrace``, ``submit_commands_svgf_denoising``,
``end_frame``.  The frame policy is the reference's: SVGF is skipped while the camera (or sun) moves
and history is reset on the first static frame (src/DeferredRenderer.cpp:133-146,593-614); the first
rendered frame index is 1 (src/Renderer.cpp:262-273).  The raster G-buffer, PBR and tonemap passes
of the reference are outside this path: the G-buffer comes from ``submit_commands_gbuffer`` (a
primary-visibility ray cast with the reference encodings) or is uploaded by the caller.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib, scene as S
from .svgf import PLANE_RADIANCE, SLOT_CURRENT, NebError, SVGFDenoiser  # noqa: F401

HIT_DTYPE = np.dtype([("t", np.float32), ("geometry", np.uint32), ("primitive", np.uint32), ("flags", np.uint32)])


@dataclass
class SceneSunUI:  # src/DeferredRenderer.h:111-116
    rough_diameter: float = 0.58
    direction: tuple = (0.5, -1.0, -0.2)
    radiance: tuple = (20.0, 20.0, 20.0)


@dataclass
class GlobalIlluminationUI:  # src/DeferredRenderer.h:118-125 (nrcMaxPathVertices: 2 = one bounce, the supported value)
    sky_color: tuple = (8.0, 8.0, 8.0)
    gi_samples_per_pixel: int = 1
    max_path_vertices: int = 2
    throughput_threshold: float = 0.01


@dataclass
class RenderInfo:  # src/DeferredRenderer.h:56-63
    scene: object
    camera: S.CameraDesc
    frame_index: int
    stream: int = 0
    timestep: float = 0.0


@dataclass
class ProbeTail:
    """The probe grid a path ends in (neb_probe_tail; trace_paths / bake_probes, `tail=`): probe_grid's `grid`, the [nx * ny * nz, 32]
    "sh" `records` baked (and accumulated) for it, optionally bake_visibility's `visibility` records with the `normal_bias` the visible
    gather takes, and whether the tail is weighted as the frame weights its diffuse bounce (frame_weight)."""
    grid: object
    records: object
    visibility: object = None
    normal_bias: float = 0.0
    frame_weight: bool = True


class DeferredRenderer:
    def __init__(self):
        self.svgf = SVGFDenoiser()
        self.sun = SceneSunUI()
        self.gi_ui = GlobalIlluminationUI()
        self._scene = None
        self._morph_counts = {}  # geometry -> numTargets, as bound through set_morph_targets
        self._eye = None
        self._sun_key = None
        self.dynamic_scene_this_frame = False
        self.reset_history = False
        # Beyond the reference ("always-on"): keep denoising while the camera moves.  The
        # reference skips SVGF on those frames (DeferredRenderer.cpp:595) and resets the history when the camera stops;
        # with this flag the temporal pass runs every frame (no reprojection: it then exercises quirk 2).
        self.denoise_while_moving = False
        # Beyond the reference: reproject the history through the two frames' cameras (option svgf_reproject, set at init):
        # SVGF runs every frame, moving or not, and the history is never reset when the camera stops.
        self.temporal_reprojection = False
        # ... and follow submeshes moved by update_transforms (option svgf_motion, set at init; needs temporal_reprojection): a pixel's
        # history is looked up where its surface point was one frame ago, and only taps of the same submesh count.  submit_commands_gbuffer
        # writes the ids and takes the transform snapshot; a caller that uploads its own G-buffer uploads PLANE_SUBMESH_ID too and
        # calls svgf.snapshot_transforms(SLOT_CURRENT) once the frame's update_transforms has been made.
        self.motion_vectors = False
        # ... and submeshes deformed by update_vertices (option svgf_vertex_motion, set at init; needs motion_vectors): submit_commands_gbuffer
        # also writes PLANE_PREV_POINT, where each pixel's surface point was one frame ago, from the previous vertices it keeps.  A caller
        # that uploads its own G-buffer uploads that plane too and calls svgf.snapshot_vertices() once per frame.
        self.vertex_motion = False
        # Beyond the reference, independent of the three above: divide the primary surface's albedo out in front of the temporal pass and
        # multiply it back at the last a-trous level, so that the filter smooths lighting and leaves textures sharp (option svgf_demodulate,
        # set at init).  The albedo plane of the frame must be in place before submit_commands_svgf_denoising and stay until it returns.
        self.albedo_demodulation = False
        self.info = None

    # ---- DeferredRenderer::Init (src/DeferredRenderer.cpp:26-57) ----
    def init(self, width, height, atrous_levels=None, device=0, row_begin=0, row_end=0):
        self.svgf.init(width, height, atrous_levels=atrous_levels, device=device, row_begin=row_begin, row_end=row_end)
        if self.motion_vectors and not self.temporal_reprojection:
            self.svgf.destroy()
            raise NebError("DeferredRenderer.init: motion_vectors needs temporal_reprojection")
        if self.vertex_motion and not self.motion_vectors:
            self.svgf.destroy()
            raise NebError("DeferredRenderer.init: vertex_motion needs motion_vectors")
        if self.temporal_reprojection:
            self.svgf.set_option("svgf_reproject", 1)
        if self.motion_vectors:
            self.svgf.set_option("svgf_motion", 1)
        if self.vertex_motion:
            self.svgf.set_option("svgf_vertex_motion", 1)
        if self.albedo_demodulation:
            self.svgf.set_option("svgf_demodulate", 1)
        self.width, self.height = width, height
        return True

    @property
    def _lib(self):
        return self.svgf._lib

    @property
    def _ctx(self):
        return self.svgf._ctx

    def _check(self, rc, what):
        _lib.check(self._lib, self._ctx, rc, what)

    # ---- DeferredRenderer::InitPathtracerScene + InitRTAccelerationStructures (:978-1030,1083-1086) ----
    def init_pathtracer_scene(self, scene, stream=0):
        G, ng, M, nm, T, nt = scene.descs()
        self._morph_counts = {}
        self._scene = None  # (neb_gi_set_scene lets go of the old scene first: if the new one is refused the context has none)
        self._check(self._lib.neb_gi_set_scene(self._ctx, G, ng, M, nm, T, nt), "neb_gi_set_scene")
        self._check(self._lib.neb_gi_build_bvh(self._ctx, C.c_void_p(stream)), "neb_gi_build_bvh")
        self._scene = scene

    # ---- RTAccelerationStructureBuilder::CreateTlas with a valid updateTlas (RTAccelerationStructureBuilder.cpp:100-130) ----
    def update_transforms(self, indices, matrices, stream=None):
        """Move submeshes: geometry indices[k] gets the 4x4 surfaceToWorld matrices[k] (row-vector convention, as Scene.add_geometry's
        M); the tree is refitted in place (neb_gi_update_transforms).  The renderer's scene object takes the same matrices, so its
        G-buffer and oracle helpers see the scene the device holds -- a Scene shared with another renderer moves there too."""
        if self._scene is None:
            raise NebError("update_transforms: no scene (init_pathtracer_scene first)")
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))
        if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise NebError("update_transforms: geometry index out of range")
        idx = idx.astype(np.uint32)
        mats = np.ascontiguousarray(np.asarray(matrices, np.float32).reshape(-1, 4, 4))
        if mats.shape[0] != idx.size:
            raise NebError(f"update_transforms: {idx.size} indices but {mats.shape[0]} matrices")
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        rc = self._lib.neb_gi_update_transforms(self._ctx, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                mats.ctypes.data_as(C.POINTER(C.c_float)), idx.size, st)
        self._check(rc, "neb_gi_update_transforms")
        for k, gi in enumerate(idx):
            self._scene.geometries[int(gi)]["M"] = mats[k].copy()

    # ---- InstanceMask = 0 / 0xFF in that same update (RTCommon.h:90) ----
    def set_visible(self, indices, visible, stream=None):
        """Hide or show submeshes in place: geometry indices[k] is shown where visible[k] is true and hidden -- absent for every ray --
        where it is false; `visible` is one bool for all or a sequence (neb_gi_set_visibility).  The tree is kept, so showing costs what
        hiding costs.  The renderer's scene object is not changed: a hidden submesh keeps its vertices, matrix and index list."""
        if self._scene is None:
            raise NebError("set_visible: no scene (init_pathtracer_scene first)")
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))
        if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise NebError("set_visible: geometry index out of range")
        idx = idx.astype(np.uint32)
        vis = np.asarray(visible)
        vis = np.full(idx.size, bool(vis), np.uint8) if vis.ndim == 0 else np.ascontiguousarray(vis.reshape(-1).astype(bool).astype(np.uint8))
        if vis.size != idx.size:
            raise NebError(f"set_visible: {idx.size} indices but {vis.size} flags")
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        rc = self._lib.neb_gi_set_visibility(self._ctx, idx.ctypes.data_as(C.POINTER(C.c_uint32)), vis.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             idx.size, st)
        self._check(rc, "neb_gi_set_visibility")

    # ---- ray queries: the caller's rays against the scene as it stands (no reference counterpart) ----
    def cast_rays(self, rays, any_hit=False, sort=False, out=None, stream=None):
        """Cast n rays from a device buffer into the scene the renderer holds (neb_gi_cast_rays): `rays` is a contiguous float32 CUDA
        tensor [n, 8], a row = {origin xyz, tmin, direction xyz, tmax} (directions need not be normalised, tmax may be inf).  Closest
        hit: returns a dict of tensors t, u, v (float32), geometry, primitive (uint32 bit patterns as int32: -1 = no hit; t = inf
        then), all views of one [n, 8] float32 buffer, which is under "records" -- `out`, when given.  any_hit=True: returns
        {"occluded": int32 [n]}, 1 = something lies in (tmin, tmax) -- `out`, when given.  sort=True reorders the rays for coherence
        before the walk; the answers are the same bits.  The call only enqueues on `stream` (a raw stream handle; default: the
        frame's), behind every update enqueued before it; nothing is copied to the host."""
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8
                and rays.is_contiguous()):
            raise NebError("cast_rays: rays must be a contiguous float32 CUDA tensor [n, 8]")
        n = rays.shape[0]
        shape, dtype = ((n,), torch.int32) if any_hit else ((n, 8), torch.float32)
        if out is None:
            with torch.cuda.device(rays.device):
                out = torch.empty(shape, dtype=dtype, device=rays.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()):
            raise NebError(f"cast_rays: out must be a contiguous {dtype} CUDA tensor of shape {shape}")
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        flags = (_lib.RAYS_ANY_HIT if any_hit else 0) | (_lib.RAYS_SORT if sort else 0)
        rc = self._lib.neb_gi_cast_rays(self._ctx, C.c_void_p(rays.data_ptr() if n else 0), n, flags, C.c_void_p(out.data_ptr() if n else 0), st)
        self._check(rc, "neb_gi_cast_rays")
        if any_hit:
            return {"occluded": out}
        ids = out.view(torch.int32)
        return {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "geometry": ids[:, 3], "primitive": ids[:, 4], "records": out}

    def shade_rays(self, rays, what="surface", constants=None, sort=False, out=None, stream=None):
        """Cast n rays as cast_rays does and shade their closest hits (neb_gi_shade_rays).  what="surface": returns
        views of one [n, 24] float32 buffer (neb_ray_surface) -- position [n, 3], t, geometric_normal, shading_normal, albedo [n, 3],
        roughness, metalness, texcoord [n, 2], material, u, v, geometry, primitive, flags (the ids and flags as int32; flags of
        _lib.HIT_*) -- with the buffer under "records".  what="radiance": views of one [n, 8] buffer (neb_ray_radiance) -- radiance
        [n, 3], t, geometry, primitive, flags -- where a miss carries the sky and a hit the sun's direct light through one disk-sampled
        shadow ray; `constants` (a scene.GIConstants; default: global_constants() of the frame) gives sky, sun and the frameIndex that
        seeds the disk draws.  `out`, when given, is the buffer.  sort=True reorders the rays for coherence; the answers are the same
        bits.  The call only enqueues on `stream`, behind every update enqueued before it; nothing is copied to the host."""
        import torch
        if what not in ("surface", "radiance"):
            raise NebError('shade_rays: what is "surface" or "radiance"')
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8
                and rays.is_contiguous()):
            raise NebError("shade_rays: rays must be a contiguous float32 CUDA tensor [n, 8]")
        n = rays.shape[0]
        radiance = what == "radiance"
        shape = (n, 8) if radiance else (n, 24)
        if out is None:
            with torch.cuda.device(rays.device):
                out = torch.empty(shape, dtype=torch.float32, device=rays.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
            raise NebError(f"shade_rays: out must be a contiguous torch.float32 CUDA tensor of shape {shape}")
        if radiance and constants is None:
            constants = self.global_constants()
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        rc = self._lib.neb_gi_shade_rays(self._ctx, C.c_void_p(rays.data_ptr() if n else 0), n, _lib.SHADE_RADIANCE if radiance else _lib.SHADE_SURFACE,
                                         _lib.RAYS_SORT if sort else 0, C.byref(constants) if constants is not None else None,
                                         C.c_void_p(out.data_ptr() if n else 0), st)
        self._check(rc, "neb_gi_shade_rays")
        ids = out.view(torch.int32)
        if radiance:
            return {"radiance": out[:, 0:3], "t": out[:, 3], "geometry": ids[:, 4], "primitive": ids[:, 5], "flags": ids[:, 6], "records": out}
        return {"position": out[:, 0:3], "t": out[:, 3], "geometric_normal": out[:, 4:7], "geometry": ids[:, 7], "shading_normal": out[:, 8:11],
                "primitive": ids[:, 11], "albedo": out[:, 12:15], "roughness": out[:, 15], "metalness": out[:, 16], "texcoord": out[:, 17:19],
                "material": ids[:, 19], "u": out[:, 20], "v": out[:, 21], "flags": ids[:, 22], "records": out}

    def _tail_arg(self, who, tail, device, written):
        """ProbeTail -> _lib.ProbeTailDesc (None -> None), checked in the style of gather_probes; `written`: (name, tensor) the call
        writes or reads as its own input, which the grid's buffers must not share memory with."""
        if tail is None:
            return None
        if not isinstance(tail, ProbeTail):
            raise NebError(f"{who}: tail must be a ProbeTail or None")
        count = self._grid_arg(who, tail.grid)
        self._records_arg(who, "tail.records", tail.records, count)
        normal_bias = self._bias_arg(who, tail.normal_bias)
        if tail.visibility is None:
            if normal_bias != 0.0:
                raise NebError(f"{who}: tail.normal_bias is read only with tail.visibility")
        else:
            self._visibility_arg(who, "tail.visibility", tail.visibility, count)
        for name, t in (("tail.records", tail.records), ("tail.visibility", tail.visibility)):
            if t is None:
                continue
            if t.device != device:
                raise NebError(f"{who}: {name} must lie on the device of the call's other tensors")
            a0, a1 = t.data_ptr(), t.data_ptr() + t.numel() * 4
            for wname, w in written:
                if w is not None and w.numel() and a0 < w.data_ptr() + w.numel() * 4 and w.data_ptr() < a1:
                    raise NebError(f"{who}: {name} overlaps {wname} (bake into a second buffer, then accumulate)")
        return _lib.ProbeTailDesc(tail.grid, tail.records.data_ptr(), tail.visibility.data_ptr() if tail.visibility is not None else None, normal_bias,
                                  _lib.TAIL_FRAME_WEIGHT if tail.frame_weight else 0)

    def trace_paths(self, rays, constants=None, max_path_vertices=None, sort=False, vertices=False, out=None, stream=None, tail=None):
        """Cast n rays as cast_rays does and follow each as the frame follows a pixel's path (neb_gi_trace_paths): up to
        K - 1 segments, K = max_path_vertices (2..8; default: the constants' maxPathVertices), the sun's direct light at every vertex and
        the sky where a segment misses.  Returns views of one [n, 8] float32 buffer (neb_ray_path) -- radiance [n, 3], t, geometry,
        primitive, flags (of the first hit; _lib.HIT_* | _lib.PATH_ESCAPED), segments -- with the buffer under "records" (`out`, when
        given).  vertices=True also returns one record per segment (neb_path_vertex) as views of one [n, K - 1, 24] buffer under
        "vertex_records": origin, tmin, direction, vertex_t, throughput, rng, added, vertex_flags, vertex_geometry, vertex_primitive, u, v,
        tmax, pdiff; a record past the path's end is zero.  `constants` (default: global_constants() of the frame) is not changed.  With
        K = 2 the records are shade_rays("radiance")'s.  sort=True reorders the rays for coherence; the answers are the same bits.  The
        call only enqueues on `stream`, behind every update enqueued before it; nothing is copied to the host.
        `tail` (a ProbeTail; neb_gi_trace_paths_tail): a path that reaches its last possible vertex on a surface with a
        material ends in the tail's probe grid -- the vertex adds throughput * albedo * (1 - metalness) / pi * E(hit point, normal turned
        toward the ray), E being gather_probes' answer there, and the vertex and the path gain _lib.PATH_TAIL.  Everything before that
        vertex is the plain call's bits; tail=None is the plain call."""
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8
                and rays.is_contiguous()):
            raise NebError("trace_paths: rays must be a contiguous float32 CUDA tensor [n, 8]")
        n = rays.shape[0]
        if constants is None:
            constants = self.global_constants()
        if max_path_vertices is not None:
            constants = type(constants).from_buffer_copy(constants)
            constants.maxPathVertices = int(max_path_vertices)
        K = int(constants.maxPathVertices)
        if not 2 <= K <= 8:
            raise NebError("trace_paths: max_path_vertices must be 2..8")
        if out is None:
            with torch.cuda.device(rays.device):
                out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 8) and out.is_contiguous()):
            raise NebError(f"trace_paths: out must be a contiguous torch.float32 CUDA tensor of shape {(n, 8)}")
        vert = None
        if vertices is True:
            with torch.cuda.device(rays.device):
                vert = torch.empty((n, K - 1, 24), dtype=torch.float32, device=rays.device)
        elif vertices is not False and vertices is not None:
            vert = vertices
            if not (isinstance(vert, torch.Tensor) and vert.is_cuda and vert.dtype == torch.float32 and tuple(vert.shape) == (n, K - 1, 24)
                    and vert.is_contiguous()):
                raise NebError(f"trace_paths: vertices must be a bool or a contiguous torch.float32 CUDA tensor of shape {(n, K - 1, 24)}")
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        desc = self._tail_arg("trace_paths", tail, rays.device, (("out", out), ("vertices", vert), ("rays", rays)))
        if desc is None:
            rc = self._lib.neb_gi_trace_paths(self._ctx, C.c_void_p(rays.data_ptr() if n else 0), n, _lib.RAYS_SORT if sort else 0, C.byref(constants),
                                              C.c_void_p(out.data_ptr() if n else 0), C.c_void_p(vert.data_ptr() if vert is not None and n else 0), st)
            self._check(rc, "neb_gi_trace_paths")
        else:
            rc = self._lib.neb_gi_trace_paths_tail(self._ctx, C.c_void_p(rays.data_ptr() if n else 0), n, _lib.RAYS_SORT if sort else 0, C.byref(constants),
                                                   C.byref(desc), C.c_void_p(out.data_ptr() if n else 0),
                                                   C.c_void_p(vert.data_ptr() if vert is not None and n else 0), st)
            self._check(rc, "neb_gi_trace_paths_tail")
        ids = out.view(torch.int32)
        res = {"radiance": out[:, 0:3], "t": out[:, 3], "geometry": ids[:, 4], "primitive": ids[:, 5], "flags": ids[:, 6], "segments": ids[:, 7], "records": out}
        if vert is not None:
            vi = vert.view(torch.int32)
            res.update({"origin": vert[..., 0:3], "tmin": vert[..., 3], "direction": vert[..., 4:7], "vertex_t": vert[..., 7], "throughput": vert[..., 8:11],
                        "rng": vi[..., 11], "added": vert[..., 12:15], "vertex_flags": vi[..., 15], "vertex_geometry": vi[..., 16],
                        "vertex_primitive": vi[..., 17], "u": vert[..., 18], "v": vert[..., 19], "tmax": vert[..., 20], "pdiff": vert[..., 21],
                        "vertex_records": vert})
        return res

    # ---- probe baking: S path samples per probe, generated, followed and reduced on the device ----
    @staticmethod
    def _probe_args(who, probes, samples, what):
        import torch
        if what not in ("sh", "irradiance"):
            raise NebError(f'{who}: what is "sh" or "irradiance"')
        if not (isinstance(probes, torch.Tensor) and probes.is_cuda and probes.dtype == torch.float32 and probes.dim() == 2 and probes.shape[1] == 8
                and probes.is_contiguous()):
            raise NebError(f"{who}: probes must be a contiguous float32 CUDA tensor [n, 8]")
        samples = int(samples)
        if samples < 64 or samples > 4096 or samples % 64:
            raise NebError(f"{who}: samples must be a multiple of 64 in 64..4096")
        return probes.shape[0], samples, _lib.BAKE_SH if what == "sh" else _lib.BAKE_IRRADIANCE

    def probe_rays(self, probes, samples=64, what="sh", frame_index=None, out=None, stream=None):
        """The rays bake_probes follows (neb_gi_probe_rays): `probes` is a contiguous float32 CUDA tensor [n, 8], a row = {position xyz,
        tmin, normal xyz, tmax}; returns a [n * samples, 8] float32 tensor of rays (`out`, when given), ray p * samples + s being sample s
        of probe p: uniform over the sphere (what="sh") or cosine-distributed about the normal (what="irradiance"), origin and interval
        the probe's own.  A probe that cannot be baked gets rays of zeroes.  `frame_index` seeds the directions (default: the frame's
        -- what bake_probes takes from global_constants() -- or 0 where no frame has begun).  Needs no scene and no frame.  The call
        only enqueues on `stream`."""
        import torch
        n, samples, what_id = self._probe_args("probe_rays", probes, samples, what)
        shape = (n * samples, 8)
        if out is None:
            with torch.cuda.device(probes.device):
                out = torch.empty(shape, dtype=torch.float32, device=probes.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
            raise NebError(f"probe_rays: out must be a contiguous torch.float32 CUDA tensor of shape {shape}")
        if frame_index is None:
            frame_index = self.info.frame_index if self.info else 0
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        rc = self._lib.neb_gi_probe_rays(self._ctx, C.c_void_p(probes.data_ptr() if n else 0), n, samples, what_id, int(frame_index) & 0xFFFFFFFF,
                                         C.c_void_p(out.data_ptr() if n else 0), st)
        self._check(rc, "neb_gi_probe_rays")
        return out

    def bake_probes(self, probes, samples=64, what="sh", constants=None, max_path_vertices=None, out=None, stream=None, tail=None):
        """Bake n probes on the device (neb_gi_bake_probes): `samples` path samples per probe (a multiple of 64 in
        64..4096), each followed as trace_paths follows ray p * samples + s of probe_rays(probes, samples, what, constants.frameIndex),
        and reduced to one record per probe.  what="sh": the nine second-order spherical-harmonics coefficients of the incoming
        radiance, x rgb; what="irradiance": E = pi * mean(L) over cosine-distributed directions about the probe's normal (a lightmap
        texel).  Returns views of one [n, 32] float32 buffer (neb_probe_record) -- sh [n, 9, 3] (irradiance: sh[:, 0] = E, the rest
        0), irradiance [n, 3] (= sh[:, 0]), samples, hits, backfaces, segments, flags (int32; _lib.PROBE_NOT_BAKED) -- with the buffer
        under "records" (`out`, when given).  `constants` (default: global_constants() of the frame) is not changed;
        max_path_vertices (2..8) overrides its maxPathVertices.  The result equals the documented float32 reduction of trace_paths over
        probe_rays bit for bit and needs none of their buffers.  The call only enqueues on `stream`, behind every update enqueued
        before it; nothing is copied to the host.
        `tail` (a ProbeTail; neb_gi_bake_probes_tail): every sample ends in the tail's grid as trace_paths(tail=) ends
        it, so that bake -> accumulate_probes -> bake(tail=ProbeTail(grid, the accumulated records)) gains one bounce per round with a
        bake as short as two path vertices.  `out` must not be the tail's records: bake into a second buffer, then accumulate."""
        import torch
        n, samples, what_id = self._probe_args("bake_probes", probes, samples, what)
        if constants is None:
            constants = self.global_constants()
        if max_path_vertices is not None:
            constants = type(constants).from_buffer_copy(constants)
            constants.maxPathVertices = int(max_path_vertices)
        if not 2 <= int(constants.maxPathVertices) <= 8:
            raise NebError("bake_probes: max_path_vertices must be 2..8")
        if out is None:
            with torch.cuda.device(probes.device):
                out = torch.empty((n, 32), dtype=torch.float32, device=probes.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 32) and out.is_contiguous()):
            raise NebError(f"bake_probes: out must be a contiguous torch.float32 CUDA tensor of shape {(n, 32)}")
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        desc = self._tail_arg("bake_probes", tail, probes.device, (("out", out), ("probes", probes)))
        if desc is None:
            rc = self._lib.neb_gi_bake_probes(self._ctx, C.c_void_p(probes.data_ptr() if n else 0), n, samples, what_id, 0, C.byref(constants),
                                              C.c_void_p(out.data_ptr() if n else 0), st)
            self._check(rc, "neb_gi_bake_probes")
        else:
            rc = self._lib.neb_gi_bake_probes_tail(self._ctx, C.c_void_p(probes.data_ptr() if n else 0), n, samples, what_id, 0, C.byref(constants),
                                                   C.byref(desc), C.c_void_p(out.data_ptr() if n else 0), st)
            self._check(rc, "neb_gi_bake_probes_tail")
        ids = out.view(torch.int32)
        return {"sh": out[:, 0:27].view(n, 9, 3), "irradiance": out[:, 0:3], "samples": ids[:, 27], "hits": ids[:, 28], "backfaces": ids[:, 29],
                "segments": ids[:, 30], "flags": ids[:, 31], "records": out}

    # ---- probe volumes: grid, running mean and irradiance gather, all on the device ----
    @staticmethod
    def _grid_arg(who, grid):
        if not isinstance(grid, _lib.ProbeGrid):
            raise NebError(f"{who}: grid must be a _lib.ProbeGrid (probe_grid returns one)")
        dims = [int(d) for d in grid.dims]
        count = dims[0] * dims[1] * dims[2]
        if min(dims) < 1 or count > 1 << 24:
            raise NebError(f"{who}: dims must be >= 1 each, with at most 2^24 probes")
        if not all(np.isfinite(o) for o in grid.origin) or not all(np.isfinite(s) and s > 0 for s in grid.spacing):
            raise NebError(f"{who}: origin must be finite, spacing finite and > 0")
        if not 0.0 <= grid.backface_limit <= 1.0:
            raise NebError(f"{who}: backface_limit must lie in 0..1")
        return count

    @staticmethod
    def _records_arg(who, name, t, rows=None):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 32 and t.is_contiguous()
                and (rows is None or t.shape[0] == rows)):
            raise NebError(f"{who}: {name} must be a contiguous float32 CUDA tensor [{'n' if rows is None else rows}, 32]")
        return t.shape[0]

    def probe_grid(self, origin, spacing, dims, tmin=0.0, tmax=float("inf"), backface_limit=0.25, out=None, stream=None):
        """The probes of a regular grid (neb_gi_probe_grid): returns (grid, probes) -- a _lib.ProbeGrid, which
        gather_probes takes, and a [nx * ny * nz, 8] float32 CUDA tensor (`out`, when given) that bake_probes takes: probe
        x + nx * (y + ny * z) at origin + (x, y, z) * spacing, normal (0, 0, 1), interval (tmin, tmax).  `spacing` is one number or
        three.  backface_limit: a probe whose backfaces exceed this share of its samples is ignored by gather_probes.  Needs no scene
        and no frame.  The call only enqueues on `stream`."""
        import torch
        origin = np.asarray(origin, np.float32).reshape(-1)
        spacing = np.broadcast_to(np.asarray(spacing, np.float32).reshape(-1), (3,)) if np.size(spacing) in (1, 3) else np.zeros(0, np.float32)
        dims_ = np.asarray(dims).reshape(-1)
        if origin.size != 3 or spacing.size != 3 or dims_.size != 3 or (dims_ < 1).any() or (dims_ > 1 << 24).any():
            raise NebError("probe_grid: origin and dims have three entries, spacing one or three; dims must be >= 1 each")
        grid = _lib.ProbeGrid((C.c_float * 3)(*origin.tolist()), (C.c_float * 3)(*spacing.tolist()), (C.c_uint32 * 3)(*[int(d) for d in dims_]),
                              float(backface_limit))
        count = self._grid_arg("probe_grid", grid)
        if out is None:
            with torch.cuda.device(self.svgf.device):
                out = torch.empty((count, 8), dtype=torch.float32, device=f"cuda:{self.svgf.device}")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (count, 8) and out.is_contiguous()):
            raise NebError(f"probe_grid: out must be a contiguous torch.float32 CUDA tensor of shape {(count, 8)}")
        rc = self._lib.neb_gi_probe_grid(self._ctx, C.byref(grid), float(tmin), float(tmax), C.c_void_p(out.data_ptr()), self._stream_arg(stream))
        self._check(rc, "neb_gi_probe_grid")
        return grid, out

    def accumulate_probes(self, acc, add, stream=None):
        """Fold one bake into a running mean on the device (neb_gi_accumulate_probes): `acc` and `add` are contiguous
        float32 CUDA tensors [n, 32] of neb_probe_record ("records" of bake_probes, either mode).  Per probe acc becomes the
        sample-weighted mean of the two, its counters their sums; a zeroed `acc` is a valid start, an `add` record that was not baked
        changes nothing, and a probe whose samples would pass 2^32 - 1 keeps its words and gains _lib.PROBE_SATURATED.  Returns `acc`.
        Needs no scene and no frame.  The call only enqueues on `stream`."""
        n = self._records_arg("accumulate_probes", "acc", acc)
        self._records_arg("accumulate_probes", "add", add, n)
        if add.device != acc.device:
            raise NebError("accumulate_probes: acc and add must lie on one device")
        rc = self._lib.neb_gi_accumulate_probes(self._ctx, C.c_void_p(acc.data_ptr() if n else 0), C.c_void_p(add.data_ptr() if n else 0), n,
                                                self._stream_arg(stream))
        self._check(rc, "neb_gi_accumulate_probes")
        return acc

    # ---- probe visibility: distance maps per probe, a running mean of them, the gather's Chebyshev factor ----
    @staticmethod
    def _visibility_arg(who, name, t, rows=None):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 192 and t.is_contiguous()
                and (rows is None or t.shape[0] == rows)):
            raise NebError(f"{who}: {name} must be a contiguous float32 CUDA tensor [{'n' if rows is None else rows}, 192]")
        return t.shape[0]

    @staticmethod
    def _bias_arg(who, normal_bias):
        normal_bias = float(normal_bias)
        if not (np.isfinite(normal_bias) and normal_bias >= 0.0):
            raise NebError(f"{who}: normal_bias must be finite and >= 0")
        return normal_bias

    def bake_visibility(self, probes, samples=64, max_distance=None, constants=None, out=None, stream=None):
        """Bake the distance maps of n probes on the device (neb_gi_bake_visibility): the `samples` rays of
        probe_rays(probes, samples, "sh", constants.frameIndex) are walked once each, as cast_rays walks them, and their distances --
        cut at `max_distance`, which a miss counts as; about 1.5 cell diagonals is DDGI's choice -- are filtered into an 8 x 8 octahedral
        map of (mean distance, mean squared distance) per probe.  Returns views of one [n, 192] float32 buffer (neb_probe_visibility)
        -- moments [n, 64, 2], weight [n, 64] -- with the buffer under "records" (`out`, when given).  `constants` (default:
        global_constants() of the frame) gives the frame index and is not changed.  A probe that cannot be baked gets (max_distance,
        max_distance^2, weight 0) in every texel.  The call only enqueues on `stream`, behind every update enqueued before it."""
        import torch
        n, samples, _ = self._probe_args("bake_visibility", probes, samples, "sh")
        if max_distance is None or not (np.isfinite(float(max_distance)) and float(max_distance) > 0.0):
            raise NebError("bake_visibility: max_distance must be finite and > 0")
        if constants is None:
            constants = self.global_constants()
        if out is None:
            with torch.cuda.device(probes.device):
                out = torch.empty((n, 192), dtype=torch.float32, device=probes.device)
        else:
            self._visibility_arg("bake_visibility", "out", out, n)
        rc = self._lib.neb_gi_bake_visibility(self._ctx, C.c_void_p(probes.data_ptr() if n else 0), n, samples, int(constants.frameIndex) & 0xFFFFFFFF,
                                              float(max_distance), C.c_void_p(out.data_ptr() if n else 0), self._stream_arg(stream))
        self._check(rc, "neb_gi_bake_visibility")
        return {"moments": out[:, 0:128].view(n, 64, 2), "weight": out[:, 128:192], "records": out}

    def accumulate_visibility(self, acc, add, stream=None):
        """Fold one bake of distance maps into a running mean on the device (neb_gi_accumulate_visibility): `acc` and
        `add` are contiguous float32 CUDA tensors [n, 192] ("records" of bake_visibility).  Per texel acc becomes the mean of the two
        weighted by their filter weights, its weight their sum; a zeroed `acc` is a valid start and a texel of `add` with weight 0
        changes nothing.  Returns `acc`.  Needs no scene and no frame.  The call only enqueues on `stream`."""
        n = self._visibility_arg("accumulate_visibility", "acc", acc)
        self._visibility_arg("accumulate_visibility", "add", add, n)
        if add.device != acc.device:
            raise NebError("accumulate_visibility: acc and add must lie on one device")
        rc = self._lib.neb_gi_accumulate_visibility(self._ctx, C.c_void_p(acc.data_ptr() if n else 0), C.c_void_p(add.data_ptr() if n else 0), n,
                                                    self._stream_arg(stream))
        self._check(rc, "neb_gi_accumulate_visibility")
        return acc

    def gather_probes(self, grid, records, points, out=None, stream=None, visibility=None, normal_bias=0.0):
        """Irradiance at n points from a grid of SH records (neb_gi_gather_probes): `grid` is probe_grid's, `records` the
        [nx * ny * nz, 32] float32 CUDA tensor of what="sh" records baked (and accumulated) for its probes, `points` a contiguous
        float32 CUDA tensor [n, 8] in the layout of probes -- position and normal are read, the normal need not be normalised.  The
        eight records around a point are blended with trilinear weights times DDGI's direction weight, probes that were not baked or
        see too many backfaces left out, and the blend is convolved with the cosine lobe about the normal.  Returns views of one [n, 8]
        float32 buffer (neb_probe_gather) -- irradiance [n, 3], weight, corners, cell, flags (int32; _lib.GATHER_*) -- with the buffer
        under "records" (`out`, when given).  Needs no scene and no frame.  The call only enqueues on `stream`.
        `visibility` (the [nx * ny * nz, 192] "records" of bake_visibility for the grid's probes) switches to
        neb_gi_gather_probes_visible: every corner's weight takes a Chebyshev factor from the probe's distance map, looked
        up toward the point moved by `normal_bias` along its normal, so that a probe behind a thin wall keeps as little as 0.05 of its weight.
        Without it the plain gather runs, and normal_bias must be left at 0."""
        import torch
        count = self._grid_arg("gather_probes", grid)
        self._records_arg("gather_probes", "records", records, count)
        normal_bias = self._bias_arg("gather_probes", normal_bias)
        if visibility is None:
            if normal_bias != 0.0:
                raise NebError("gather_probes: normal_bias is read only with visibility")
        else:
            self._visibility_arg("gather_probes", "visibility", visibility, count)
            if visibility.device != records.device:
                raise NebError("gather_probes: records and visibility must lie on one device")
        if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 8
                and points.is_contiguous()):
            raise NebError("gather_probes: points must be a contiguous float32 CUDA tensor [n, 8]")
        if points.device != records.device:
            raise NebError("gather_probes: records and points must lie on one device")
        n = points.shape[0]
        if out is None:
            with torch.cuda.device(points.device):
                out = torch.empty((n, 8), dtype=torch.float32, device=points.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 8) and out.is_contiguous()):
            raise NebError(f"gather_probes: out must be a contiguous torch.float32 CUDA tensor of shape {(n, 8)}")
        if visibility is None:
            rc = self._lib.neb_gi_gather_probes(self._ctx, C.byref(grid), C.c_void_p(records.data_ptr()), C.c_void_p(points.data_ptr() if n else 0), n,
                                                C.c_void_p(out.data_ptr() if n else 0), self._stream_arg(stream))
            self._check(rc, "neb_gi_gather_probes")
        else:
            rc = self._lib.neb_gi_gather_probes_visible(self._ctx, C.byref(grid), C.c_void_p(records.data_ptr()), C.c_void_p(visibility.data_ptr()),
                                                        normal_bias, C.c_void_p(points.data_ptr() if n else 0), n,
                                                        C.c_void_p(out.data_ptr() if n else 0), self._stream_arg(stream))
            self._check(rc, "neb_gi_gather_probes_visible")
        ids = out.view(torch.int32)
        return {"irradiance": out[:, 0:3], "weight": out[:, 3], "corners": ids[:, 4], "cell": ids[:, 5], "flags": ids[:, 6], "records": out}

    # ---- probe-lit frames: the G-buffer as the gather's points, the gather as the frame's indirect term ----
    def _rows_arg(self, who, rows):
        if rows is None:
            return self.svgf.row_begin, self.svgf.row_end
        try:
            r0, r1 = (int(v) for v in rows)
        except (TypeError, ValueError):
            raise NebError(f"{who}: rows must be (row0, row1)") from None
        if not self.svgf.row_begin <= r0 < r1 <= self.svgf.row_end:
            raise NebError(f"{who}: rows must satisfy {self.svgf.row_begin} <= row0 < row1 <= {self.svgf.row_end}, the context's rows")
        return r0, r1

    def gbuffer_points(self, rows=None, out=None, stream=None):
        """The points the frame's ray generation shades, one per pixel of `rows` (default: all the context's rows), as a [n, 8] float32
        CUDA tensor in the layout of probes (neb_gbuffer_points; `out`, when given): {world position, 0.01, shading
        normal, inf}, pixel (x, y) at row (y - rows[0]) * width + x.  A sky pixel has position and normal 0, which gather_probes answers
        with _lib.GATHER_NOT_GATHERED.  gather_probes takes the tensor as `points`, bake_probes(what="irradiance") as `probes`.  Reads the
        G-buffer planes of the current frame, needs no scene.  The call only enqueues on `stream`."""
        import torch
        r0, r1 = self._rows_arg("gbuffer_points", rows)
        shape = ((r1 - r0) * self.width, 8)
        if out is None:
            with torch.cuda.device(self.svgf.device):
                out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.svgf.device}")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
            raise NebError(f"gbuffer_points: out must be a contiguous torch.float32 CUDA tensor of shape {shape}")
        rc = self._lib.neb_gbuffer_points(self._ctx, r0, r1, C.c_void_p(out.data_ptr()), self._stream_arg(stream))
        self._check(rc, "neb_gbuffer_points")
        return out

    def submit_commands_gi_probes(self, grid, records, frame_weight=True, rows=None, stream=None, visibility=None, normal_bias=0.0):
        """Stand-in for submit_commands_gi_pathtrace in a frame: add the irradiance a probe grid gives at every pixel's point, weighted as
        the frame's diffuse term, to radiance[cur] (neb_gi_probe_indirect).  `grid` is probe_grid's, `records` the
        [nx * ny * nz, 32] float32 CUDA tensor of what="sh" records baked (and accumulated) for its probes.  Per pixel: albedo * (1 -
        metalness) * E / pi; frame_weight=True multiplies by the mean of what the path tracer's ray generation does to its throughput
        (reads the frame's camera position), so that the probe-lit frame converges toward what the traced one converges toward.  Sky
        pixels and pixels without a valid probe keep their radiance.  No noise: the SVGF chain may follow, but is not needed.  Needs no
        scene.  The call only enqueues on `stream`.  `visibility` and `normal_bias` as gather_probes takes them: with a visibility buffer
        the gather is the visible one (neb_gi_probe_indirect_visible), without it the plain call runs."""
        count = self._grid_arg("submit_commands_gi_probes", grid)
        self._records_arg("submit_commands_gi_probes", "records", records, count)
        normal_bias = self._bias_arg("submit_commands_gi_probes", normal_bias)
        if visibility is None:
            if normal_bias != 0.0:
                raise NebError("submit_commands_gi_probes: normal_bias is read only with visibility")
        else:
            self._visibility_arg("submit_commands_gi_probes", "visibility", visibility, count)
            if visibility.device != records.device:
                raise NebError("submit_commands_gi_probes: records and visibility must lie on one device")
        r0, r1 = self._rows_arg("submit_commands_gi_probes", rows)
        if frame_weight and self.info is None:
            raise NebError("submit_commands_gi_probes: frame_weight needs a frame (begin_frame) for its camera")
        c = self.global_constants() if frame_weight else None
        flags = _lib.INDIRECT_FRAME_WEIGHT if frame_weight else 0
        if visibility is None:
            rc = self._lib.neb_gi_probe_indirect_rows(self._ctx, C.byref(grid), C.c_void_p(records.data_ptr()), None if c is None else C.byref(c),
                                                      flags, r0, r1, self._stream_arg(stream))
            self._check(rc, "neb_gi_probe_indirect")
        else:
            rc = self._lib.neb_gi_probe_indirect_visible_rows(self._ctx, C.byref(grid), C.c_void_p(records.data_ptr()),
                                                              C.c_void_p(visibility.data_ptr()), normal_bias, None if c is None else C.byref(c),
                                                              flags, r0, r1, self._stream_arg(stream))
            self._check(rc, "neb_gi_probe_indirect_visible")

    def visibility(self):
        """one bool per geometry of the scene: True = visible (neb_gi_get_visibility)"""
        n = C.c_uint32(0)
        self._check(self._lib.neb_gi_get_visibility(self._ctx, None, 0, C.byref(n)), "neb_gi_get_visibility")
        out = np.zeros(n.value, np.uint8)
        if n.value:
            self._check(self._lib.neb_gi_get_visibility(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), n.value, None), "neb_gi_get_visibility")
        return out.astype(bool)

    # ---- the material table and the textures uploaded again, the TLAS untouched (GIProcessedScene.cpp:16-137) ----
    def _stream_arg(self, stream):
        return C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)

    def update_materials(self, indices, albedo=None, rough_metal=None, stream=None):
        """New factors for materials indices[k]: albedo[k] (rgb; a fourth component is ignored) and / or rough_metal[k] (roughness,
        metalness); None keeps what the material has.  The maps a material binds do not change (neb_gi_update_materials).  The tree and
        the sun table are kept.  The renderer's scene object takes the same factors."""
        if self._scene is None:
            raise NebError("update_materials: no scene (init_pathtracer_scene first)")
        idx = np.asarray(indices, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self._scene.materials)):
            raise NebError("update_materials: material index out of range")
        alb = None if albedo is None else np.asarray(albedo, np.float32).reshape(idx.size, -1)
        rm = None if rough_metal is None else np.asarray(rough_metal, np.float32).reshape(idx.size, -1)
        if (alb is not None and alb.shape[1] not in (3, 4)) or (rm is not None and rm.shape[1] != 2):
            raise NebError("update_materials: albedo is n x 3 (or 4), rough_metal n x 2")
        descs = (S.MaterialDesc * max(1, idx.size))()
        new = []
        for k, mi in enumerate(idx):
            m = self._scene.materials[int(mi)]
            a = tuple(float(v) for v in alb[k][:3]) + (m["albedo"][3],) if alb is not None else m["albedo"]
            r = tuple(float(v) for v in rm[k]) if rm is not None else m["rm"]
            descs[k].textureIndices[:] = m["textures"]
            descs[k].albedo[:] = a
            descs[k].roughnessMetalness[:] = r
            new.append((a, r))
        ids = np.ascontiguousarray(idx.astype(np.uint32))
        self._check(self._lib.neb_gi_update_materials(self._ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)), descs, idx.size, self._stream_arg(stream)),
                    "neb_gi_update_materials")
        self._scene.materials = list(self._scene.materials)  # (a fresh list and fresh dicts: a Scene that shares its materials with a clone does not change the clone)
        for mi, (a, r) in zip(idx, new):
            self._scene.materials[int(mi)] = dict(self._scene.materials[int(mi)], albedo=a, rm=r)

    def set_geometry_materials(self, indices, materials, stream=None):
        """Geometry indices[k] names material materials[k] from here on; -1 = none (neb_gi_set_geometry_materials).  The tree and the sun
        table are kept.  The renderer's scene object follows."""
        if self._scene is None:
            raise NebError("set_geometry_materials: no scene (init_pathtracer_scene first)")
        idx = np.asarray(indices, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self._scene.geometries)):
            raise NebError("set_geometry_materials: geometry index out of range")
        mats = np.asarray(materials, np.int64).reshape(-1)
        mats = np.full(idx.size, int(mats[0]), np.int64) if mats.size == 1 and idx.size != 1 else mats
        if mats.size != idx.size:
            raise NebError(f"set_geometry_materials: {idx.size} indices but {mats.size} materials")
        if mats.size and mats.max() >= len(self._scene.materials):
            raise NebError("set_geometry_materials: material index out of range")
        ids, ms = np.ascontiguousarray(idx.astype(np.uint32)), np.ascontiguousarray(np.maximum(mats, -1).astype(np.int32))
        self._check(self._lib.neb_gi_set_geometry_materials(self._ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ms.ctypes.data_as(C.POINTER(C.c_int32)),
                                                            idx.size, self._stream_arg(stream)), "neb_gi_set_geometry_materials")
        for gi, mi in zip(idx, ms):
            self._scene.geometries[int(gi)]["material"] = int(mi)

    def update_texture(self, index, rgba8, x=0, y=0, stream=None, mirror=True):
        """New texels for texture `index`: the rectangle at (x, y) of the size of rgba8 (rows x columns x 4 uint8).  A numpy array goes
        through the host call (neb_gi_update_textures: copied before the call returns); a torch tensor on this renderer's device through
        the device call (neb_gi_update_textures_device): rows may be strided and are read where they lie, in stream order -- `stream` has
        to be ordered behind whatever wrote them and they must stay untouched until the stream has passed the update.  The tree and the sun
        table are kept.  mirror=True: the renderer's scene object takes the texels (a device tensor is copied back for it: .cpu() waits)."""
        if self._scene is None:
            raise NebError("update_texture: no scene (init_pathtracer_scene first)")
        index, x, y = int(index), int(x), int(y)
        if not 0 <= index < len(self._scene.textures) or x < 0 or y < 0:
            raise NebError("update_texture: texture index or origin out of range")
        u = _lib.TextureUpdate(texture=index, x=x, y=y)
        host = isinstance(rgba8, np.ndarray) or not hasattr(rgba8, "data_ptr")
        if host:
            px = np.asarray(rgba8)
            if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 4:
                raise NebError("update_texture: rgba8 must be uint8 of shape (rows, columns, 4)")
            if px.size and (px.strides[2] != 1 or px.strides[1] != 4 or px.strides[0] < 4 * px.shape[1] or px.strides[0] % 4):
                px = np.ascontiguousarray(px)
            u.height, u.width = px.shape[0], px.shape[1]
            u.pitchBytes = px.strides[0] if px.shape[0] > 1 else 4 * px.shape[1]
            u.rgba8 = px.ctypes.data
            fn, name = self._lib.neb_gi_update_textures, "neb_gi_update_textures"
        else:
            import torch
            px = rgba8
            if not isinstance(px, torch.Tensor) or not px.is_cuda or px.dtype != torch.uint8 or px.dim() != 3 or px.shape[2] != 4:
                raise NebError("update_texture: rgba8 must be a uint8 device tensor of shape (rows, columns, 4)")
            if px.numel() and (px.stride(2) != 1 or px.stride(1) != 4 or (px.shape[0] > 1 and (px.stride(0) < 4 * px.shape[1] or px.stride(0) % 4))):
                raise NebError("update_texture: the texels of a row must be contiguous, rows a multiple of 4 bytes apart and not overlapping")
            if px.device.index != self.svgf.device:
                raise NebError("update_texture: rgba8 is on another device than the renderer")
            u.height, u.width = px.shape[0], px.shape[1]
            u.pitchBytes = px.stride(0) if px.shape[0] > 1 else 4 * px.shape[1]
            u.rgba8 = px.data_ptr() if px.numel() else None
            fn, name = self._lib.neb_gi_update_textures_device, "neb_gi_update_textures_device"
        self._check(fn(self._ctx, C.byref(u), 1, self._stream_arg(stream)), name)
        if mirror:  # (a fresh array and a fresh list: a Scene that shares its textures with a clone does not change the clone)
            full = np.array(self._scene.textures[index], np.uint8, copy=True)
            full[y:y + u.height, x:x + u.width] = px if host else px.cpu().numpy()
            self._scene.textures = list(self._scene.textures)
            self._scene.textures[index] = full

    def texture_tables(self, stream=None):
        """the texture tables as the device holds them, as bytes: the standalone footprint tables, then the material bundles
        (neb_gi_debug_texture_tables; waits for the copy)"""
        n = C.c_size_t(0)
        self._check(self._lib.neb_gi_debug_texture_tables(self._ctx, None, 0, C.byref(n), None), "neb_gi_debug_texture_tables")
        out = np.zeros(n.value, np.uint8)
        if n.value:
            self._check(self._lib.neb_gi_debug_texture_tables(self._ctx, out.ctypes.data, n.value, None, self._stream_arg(stream)),
                        "neb_gi_debug_texture_tables")
        return out

    def shade_records(self, stream=None):
        """the sun table as the device holds it (neb_gi_debug_shade_records; waits for the copy): (records, tris, info) -- records
        (n_slots, 32) uint32, the 128-byte shading records in leaf order; tris (n_slots, 12) float32, what the traverser tests in each
        slot; info = neb_shade_records_info as a dict (valid: the last dispatch used the table, built for sun / tan_half)"""
        n = C.c_size_t(0)
        self._check(self._lib.neb_gi_debug_shade_records(self._ctx, None, 0, C.byref(n), None), "neb_gi_debug_shade_records")
        raw = np.zeros(n.value, np.uint8)
        self._check(self._lib.neb_gi_debug_shade_records(self._ctx, raw.ctypes.data, n.value, None, self._stream_arg(stream)),
                    "neb_gi_debug_shade_records")
        n_slots = (n.value - 56) // 176  # (56 = sizeof(neb_shade_records_info): eight 4-byte words, three counters of 8 bytes)
        tail = raw[176 * n_slots:].tobytes()
        u32, f32, u64 = np.frombuffer(tail[:32], np.uint32), np.frombuffer(tail[:32], np.float32), np.frombuffer(tail[32:56], np.uint64)
        if len(tail) != 56 or int(u32[0]) != n_slots:
            raise NebError("neb_gi_debug_shade_records: the size does not match the slot count")
        info = {"n_slots": n_slots, "valid": bool(u32[1]), "sun": tuple(float(x) for x in f32[2:5]), "tan_half": float(f32[5]), "builds": int(u32[6]),
                "lit_plus": int(u64[0]), "lit_minus": int(u64[1]), "hinted": int(u64[2])}
        return raw[:128 * n_slots].view(np.uint32).reshape(n_slots, 32), raw[128 * n_slots:176 * n_slots].view(np.float32).reshape(n_slots, 12), info

    # ---- no reference counterpart: its BLASes are built without ALLOW_UPDATE (RTAccelerationStructureBuilder.cpp:79) ----
    def update_vertices(self, index, positions, normals=None, tangents=None, first_vertex=0, stream=None):
        """Deform a submesh: vertices [first_vertex, first_vertex + len(positions)) of geometry `index` get new object-space positions
        and, when given, normals (n x 3) and tangents (n x 4); the tree is refitted in place and the shading records follow
        (neb_gi_update_vertices).  The renderer's scene object takes the same arrays (as copies), as update_transforms writes M."""
        if self._scene is None:
            raise NebError("update_vertices: no scene (init_pathtracer_scene first)")
        index, first_vertex = int(index), int(first_vertex)
        if not 0 <= index < len(self._scene.geometries) or not 0 <= first_vertex <= 0xFFFFFFFF:
            raise NebError("update_vertices: geometry index or first vertex out of range")
        arrays = {"positions": np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 3))}
        n = arrays["positions"].shape[0]
        for key, a, width in (("normals", normals, 3), ("tangents", tangents, 4)):
            if a is not None:
                arrays[key] = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, width))
                if arrays[key].shape[0] != n:
                    raise NebError(f"update_vertices: {n} positions but {arrays[key].shape[0]} {key}")
        u = _lib.VertexUpdate(geometry=index, firstVertex=first_vertex, numVertices=n)
        for key, width in (("positions", 3), ("normals", 3), ("tangents", 4)):
            if key in arrays:
                setattr(u, key, arrays[key].ctypes.data)
                setattr(u, key[:-1] + "Stride", 4 * width)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_update_vertices(self._ctx, C.byref(u), 1, st), "neb_gi_update_vertices")
        gm = self._scene.geometries[index]
        for key, a in arrays.items():  # (a fresh array: a Scene that shares its vertex streams with a clone does not deform the clone)
            full = np.array(gm[key], np.float32, copy=True)
            full[first_vertex:first_vertex + n] = a
            gm[key] = full

    def update_vertices_device(self, index, positions, normals=None, tangents=None, first_vertex=0, stream=None, mirror=True):
        """update_vertices with sources in device memory (neb_gi_update_vertices_device): float32 torch tensors on this renderer's
        device, n x 3 positions and, when given, n x 3 normals and n x 4 tangents.  A strided view is read where it lies (its row stride
        goes to the library; the elements of a row must be contiguous): no hidden copy.  The call only enqueues; the sources are read in
        stream order, so `stream` has to be ordered behind whatever wrote them and they must stay untouched until the stream has passed
        the update (the caller keeps them alive, e.g. with Tensor.record_stream).  A position that is not finite is refused on the
        device, later: see update_status.  mirror=True: the renderer's scene object follows from a .cpu() copy made after the enqueue
        -- only if the device accepted the update, so the scene object never holds positions the library refused (the call waits for
        the updates before it and for its own: for hosts that use the scene's G-buffer and oracle helpers); mirror=False: the scene
        object keeps its arrays and nothing waits."""
        if self._scene is None:
            raise NebError("update_vertices_device: no scene (init_pathtracer_scene first)")
        index, first_vertex = int(index), int(first_vertex)
        if not 0 <= index < len(self._scene.geometries) or not 0 <= first_vertex <= 0xFFFFFFFF:
            raise NebError("update_vertices_device: geometry index or first vertex out of range")
        import torch
        tensors = {"positions": positions}
        if normals is not None:
            tensors["normals"] = normals
        if tangents is not None:
            tensors["tangents"] = tangents
        n = None
        u = _lib.VertexUpdate(geometry=index, firstVertex=first_vertex)
        for key, t in tensors.items():
            width = 4 if key == "tangents" else 3
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width:
                raise NebError(f"update_vertices_device: {key} must be a float32 device tensor of shape (n, {width})")
            if t.shape[0] and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < width)):
                raise NebError(f"update_vertices_device: the rows of {key} must be contiguous and must not overlap")
            if t.device.index != self.svgf.device:
                raise NebError(f"update_vertices_device: {key} is on another device than the renderer")
            if n is None:
                n = t.shape[0]
            elif t.shape[0] != n:
                raise NebError(f"update_vertices_device: {n} positions but {t.shape[0]} {key}")
            setattr(u, key, t.data_ptr())
            setattr(u, key[:-1] + "Stride", 4 * (t.stride(0) if t.shape[0] > 1 else width))
        if n == 0:
            return  # (an empty range moves nothing; an empty tensor has no storage to point at)
        u.numVertices = n
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        refused = self.update_status()["refused"] if mirror else 0  # (harvests every earlier update: the difference below is this call's)
        self._check(self._lib.neb_gi_update_vertices_device(self._ctx, C.byref(u), 1, st), "neb_gi_update_vertices_device")
        if mirror and self.update_status()["refused"] == refused:
            gm = self._scene.geometries[index]
            for key, t in tensors.items():
                full = np.array(gm[key], np.float32, copy=True)
                full[first_vertex:first_vertex + n] = t.cpu().numpy()
                gm[key] = full

    # ---- skinned submeshes (neb_gi_set_skin / neb_gi_skin_vertices: DESIGN.md 3.4d); nothing here computes a skin on the CPU ----
    def set_skin(self, index, joints, weights, num_joints, stream=None):
        """Bind a skin to geometry `index`: joints (n x 4 integers below num_joints, glTF JOINTS_0) and weights (n x 4 float32, used as
        given) for every one of its vertices.  The bind pose is what the device pools hold at the call (neb_gi_set_skin)."""
        if self._scene is None:
            raise NebError("set_skin: no scene (init_pathtracer_scene first)")
        index, num_joints = int(index), int(num_joints)
        if not 0 <= index < len(self._scene.geometries) or not 0 <= num_joints <= 0xFFFFFFFF:
            raise NebError("set_skin: geometry index or num_joints out of range")
        j = np.asarray(joints).reshape(-1, 4)
        if j.size and (j.min() < 0 or j.max() > 0xFFFF):
            raise NebError("set_skin: a joint index does not fit 16 bits")
        j = np.ascontiguousarray(j.astype(np.uint16))
        w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1, 4))
        nv = len(self._scene.geometries[index]["positions"])
        if j.shape[0] != nv or w.shape[0] != nv:
            raise NebError(f"set_skin: the geometry has {nv} vertices but {j.shape[0]} joints / {w.shape[0]} weights rows were given")
        d = _lib.SkinDesc(geometry=index, numJoints=num_joints, joints=j.ctypes.data, jointStride=8, weights=w.ctypes.data, weightStride=16)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_set_skin(self._ctx, C.byref(d), 1, st), "neb_gi_set_skin")

    def remove_skin(self, index, stream=None):
        """Let go of geometry `index`'s skin and bind pose (the pools keep what they hold)."""
        if self._scene is None:
            raise NebError("remove_skin: no scene (init_pathtracer_scene first)")
        index = int(index)
        if not 0 <= index < len(self._scene.geometries):
            raise NebError("remove_skin: geometry index out of range")
        d = _lib.SkinDesc(geometry=index)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_set_skin(self._ctx, C.byref(d), 1, st), "neb_gi_set_skin")

    def skin_vertices(self, index, joint_matrices, stream=None, mirror=False):
        """Skin geometries on the device (neb_gi_skin_vertices): `index` is one geometry or a sequence of them, `joint_matrices` its palette
        (num_joints x 4 x 4, layout and convention of Scene.add_geometry's M, object space) or one palette per geometry -- all in ONE call.
        The call only enqueues; a skinned vertex that is not finite refuses the whole call on the device, later: see update_status.
        mirror=True follows update_vertices_device: after the enqueue, and only if the device accepted, the scene object's arrays are
        refreshed through download_vertices (the call then waits)."""
        if self._scene is None:
            raise NebError("skin_vertices: no scene (init_pathtracer_scene first)")
        if np.ndim(index) == 0:
            index, joint_matrices = [index], [joint_matrices]
        idx = [int(i) for i in index]
        if len(idx) != len(joint_matrices):
            raise NebError(f"skin_vertices: {len(idx)} geometries but {len(joint_matrices)} palettes")
        if any(not 0 <= i < len(self._scene.geometries) for i in idx):
            raise NebError("skin_vertices: geometry index out of range")
        pals = [np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1, 16)) for m in joint_matrices]
        ups = (_lib.SkinUpdate * max(len(idx), 1))()
        for k, (i, p) in enumerate(zip(idx, pals)):
            ups[k].geometry = i
            ups[k].jointMatrices = p.ctypes.data_as(C.POINTER(C.c_float))
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        refused = self.update_status()["refused"] if mirror else 0  # (harvests every earlier update: the difference below is this call's)
        self._check(self._lib.neb_gi_skin_vertices(self._ctx, ups, len(idx), st), "neb_gi_skin_vertices")
        if mirror and self.update_status()["refused"] == refused:
            for i in idx:
                gm = self._scene.geometries[i]
                p, n, t = self.download_vertices(i, stream=st.value or 0)
                gm["positions"] = p
                if all(gm.get(key) is not None for key in ("normals", "uvs", "tangents")):  # (else the library skins positions only)
                    gm["normals"], gm["tangents"] = n, t

    # ---- morph targets (neb_gi_set_morph_targets / neb_gi_morph_vertices: DESIGN.md 3.4e); nothing here blends on the CPU ----
    def set_morph_targets(self, index, position_deltas, normal_deltas=None, tangent_deltas=None, stream=None):
        """Bind morph targets to geometry `index`: position_deltas of shape T x n x 3 float32 (glTF target POSITION) for every one of its
        n vertices, and optionally normal and tangent deltas of the same shape.  The rest pose is what the device pools hold at the call
        (neb_gi_set_morph_targets)."""
        if self._scene is None:
            raise NebError("set_morph_targets: no scene (init_pathtracer_scene first)")
        index = int(index)
        if not 0 <= index < len(self._scene.geometries):
            raise NebError("set_morph_targets: geometry index out of range")
        nv = len(self._scene.geometries[index]["positions"])
        streams = []
        for what, a in (("position", position_deltas), ("normal", normal_deltas), ("tangent", tangent_deltas)):
            if a is None:
                streams.append(None)
                continue
            a = np.ascontiguousarray(np.asarray(a, np.float32))
            if a.ndim != 3 or a.shape[1:] != (nv, 3):
                raise NebError(f"set_morph_targets: {what} deltas of shape {a.shape}, the geometry has {nv} vertices (T x {nv} x 3 expected)")
            streams.append(a)
        if streams[0] is None:
            raise NebError("set_morph_targets: position deltas are required")
        T = streams[0].shape[0]
        if not 1 <= T <= 0xFFFF or any(a is not None and a.shape[0] != T for a in streams):
            raise NebError("set_morph_targets: 1 .. 65535 targets, the same number in every stream")
        d = _lib.MorphDesc(geometry=index, numTargets=T, positionStride=12, normalStride=12, tangentStride=12)
        for key, a in zip(("positionDeltas", "normalDeltas", "tangentDeltas"), streams):
            if a is not None:
                setattr(d, key, (C.c_void_p * T)(*[a[t].ctypes.data for t in range(T)]))
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_set_morph_targets(self._ctx, C.byref(d), 1, st), "neb_gi_set_morph_targets")
        self._morph_counts[index] = T

    def remove_morph_targets(self, index, stream=None):
        """Let go of geometry `index`'s targets and rest pose (the pools keep what they hold)."""
        if self._scene is None:
            raise NebError("remove_morph_targets: no scene (init_pathtracer_scene first)")
        index = int(index)
        if not 0 <= index < len(self._scene.geometries):
            raise NebError("remove_morph_targets: geometry index out of range")
        d = _lib.MorphDesc(geometry=index)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_set_morph_targets(self._ctx, C.byref(d), 1, st), "neb_gi_set_morph_targets")
        self._morph_counts.pop(index, None)

    def morph_vertices(self, index, weights, joint_matrices=None, stream=None, mirror=False):
        """Blend morph targets on the device (neb_gi_morph_vertices): `index` is one geometry or a sequence of them, `weights` its T weights
        or one array per geometry, `joint_matrices` None, or the palette of a skinned geometry (one entry per geometry, None where it is
        not to be skinned) -- all in ONE call.  The call only enqueues; a vertex that is not finite refuses the whole call on the device,
        later: see update_status.  mirror=True follows skin_vertices: after the enqueue, and only if the device accepted, the scene
        object's arrays are refreshed through download_vertices (the call then waits)."""
        if self._scene is None:
            raise NebError("morph_vertices: no scene (init_pathtracer_scene first)")
        if np.ndim(index) == 0:
            index, weights, joint_matrices = [index], [weights], [joint_matrices]
        idx = [int(i) for i in index]
        if joint_matrices is None:
            joint_matrices = [None] * len(idx)
        if len(idx) != len(weights) or len(idx) != len(joint_matrices):
            raise NebError(f"morph_vertices: {len(idx)} geometries but {len(weights)} weight arrays / {len(joint_matrices)} palettes")
        if any(not 0 <= i < len(self._scene.geometries) for i in idx):
            raise NebError("morph_vertices: geometry index out of range")
        ws = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1)) for w in weights]
        for i, w in zip(idx, ws):  # (the library reads numTargets floats: a shorter array is refused here)
            if i in self._morph_counts and len(w) != self._morph_counts[i]:
                raise NebError(f"morph_vertices: geometry {i} has {self._morph_counts[i]} targets but {len(w)} weights were given")
        pals = [None if m is None else np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1, 16)) for m in joint_matrices]
        fp = C.POINTER(C.c_float)
        ups = (_lib.MorphUpdate * max(len(idx), 1))()
        for k, (i, w, p) in enumerate(zip(idx, ws, pals)):
            ups[k].geometry = i
            ups[k].weights = w.ctypes.data_as(fp)
            if p is not None:
                ups[k].jointMatrices = p.ctypes.data_as(fp)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        refused = self.update_status()["refused"] if mirror else 0  # (harvests every earlier update: the difference below is this call's)
        self._check(self._lib.neb_gi_morph_vertices(self._ctx, ups, len(idx), st), "neb_gi_morph_vertices")
        if mirror and self.update_status()["refused"] == refused:
            for i in idx:
                gm = self._scene.geometries[i]
                p, n, t = self.download_vertices(i, stream=st.value or 0)
                gm["positions"] = p
                if all(gm.get(key) is not None for key in ("normals", "uvs", "tangents")):  # (else the library blends positions only)
                    gm["normals"], gm["tangents"] = n, t

    def download_vertices(self, index, first_vertex=0, n=None, stream=None):
        """-> positions (n x 3), normals (n x 3), tangents (n x 4): what the device pools hold now of geometry `index`'s vertices
        [first_vertex, first_vertex + n) (n=None: to its end).  Waits for the copies (neb_gi_download_vertices)."""
        if self._scene is None:
            raise NebError("download_vertices: no scene (init_pathtracer_scene first)")
        index, first_vertex = int(index), int(first_vertex)
        if not 0 <= index < len(self._scene.geometries) or not 0 <= first_vertex <= 0xFFFFFFFF:
            raise NebError("download_vertices: geometry index or first vertex out of range")
        if n is None:
            n = max(len(self._scene.geometries[index]["positions"]) - first_vertex, 0)
        n = int(n)
        if not 0 <= n <= 0xFFFFFFFF:
            raise NebError("download_vertices: vertex count out of range")
        p, nr, t = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
        fp = C.POINTER(C.c_float)
        st = C.c_void_p((self.info.stream if self.info else 0) if stream is None else stream)
        self._check(self._lib.neb_gi_download_vertices(self._ctx, index, first_vertex, n, p.ctypes.data_as(fp), nr.ctypes.data_as(fp),
                                                       t.ctypes.data_as(fp), st), "neb_gi_download_vertices")
        return p, nr, t

    def update_status(self):
        """{"accepted", "refused"}: device-sourced updates applied / refused on the device (a position that was not finite) since the scene
        was set.  Waits for the updates enqueued so far."""
        v = (C.c_uint64 * 2)()
        self._check(self._lib.neb_gi_update_status(self._ctx, v), "neb_gi_update_status")
        return {"accepted": int(v[0]), "refused": int(v[1])}

    def scene_box(self):
        """(lo, hi): the exact world-space box of the scene as the library holds it, two float32 arrays of 3.  Waits like update_status."""
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        self._check(self._lib.neb_gi_scene_box(self._ctx, lo, hi), "neb_gi_scene_box")
        return np.array(lo[:], np.float32), np.array(hi[:], np.float32)

    def scene_info(self):
        t, n = C.c_uint32(), C.c_uint32()
        self._check(self._lib.neb_gi_scene_info(self._ctx, C.byref(t), C.byref(n)), "neb_gi_scene_info")
        return t.value, n.value

    def scene_bytes(self):
        """device bytes of {texture tables, triangles + shading records, BVH nodes}"""
        v = (C.c_uint64 * 3)()
        self._check(self._lib.neb_gi_scene_bytes(self._ctx, v), "neb_gi_scene_bytes")
        return dict(zip(("texture_tables", "triangles", "bvh_nodes"), [int(x) for x in v]))

    def bvh_depth(self):
        d = C.c_uint32()
        self._check(self._lib.neb_gi_bvh_depth(self._ctx, C.byref(d)), "neb_gi_bvh_depth")
        return d.value

    def build_ms(self):
        """wall time (ms) of the last BVH build"""
        d = C.c_float()
        self._check(self._lib.neb_gi_build_ms(self._ctx, C.byref(d)), "neb_gi_build_ms")
        return float(d.value)

    def build_passes(self):
        d = C.c_uint32()
        self._check(self._lib.neb_gi_build_passes(self._ctx, C.byref(d)), "neb_gi_build_passes")
        return d.value

    # ---- DeferredRenderer::BeginFrame (src/DeferredRenderer.cpp:89-149) ----
    def begin_frame(self, info):
        self.info = info
        if info.scene is not None and info.scene is not self._scene:
            self.init_pathtracer_scene(info.scene, info.stream)
        self.svgf.begin_frame(info.frame_index)
        if self.temporal_reprojection:  # (for a caller that uploads its own G-buffer; submit_commands_gbuffer records the same camera)
            self.svgf.set_camera(SLOT_CURRENT, info.camera)
        eye = tuple(info.camera.eye)
        sun_key = (self.sun.rough_diameter, tuple(self.sun.direction), tuple(self.sun.radiance))
        moved = (eye != self._eye) or (self._sun_key is not None and sun_key != self._sun_key)  # :133-146,169-171
        self._sun_key = sun_key
        if moved:
            self._eye = eye
            self.dynamic_scene_this_frame = True
        elif self.dynamic_scene_this_frame:
            self.dynamic_scene_this_frame = False  # camera stopped: reset history and start denoising
            self.reset_history = not (self.denoise_while_moving or self.temporal_reprojection)

    def end_frame(self):
        self.svgf.end_frame()

    def global_constants(self):
        """GlobalConstants upload of SubmitCommandsGIPathtrace (src/DeferredRenderer.cpp:403-421)."""
        import math
        c = S.GIConstants()
        c.frameIndex = self.info.frame_index & 0xFFFFFFFF
        c.samplesPerPixel = int(self.gi_ui.gi_samples_per_pixel)
        c.maxPathVertices = int(self.gi_ui.max_path_vertices)
        c.cameraWorldPos[:] = tuple(self.info.camera.eye)
        c.skyColor[:] = self.gi_ui.sky_color
        c.sunLightDirection[:] = self.sun.direction
        c.sunLightRadiance[:] = self.sun.radiance
        c.sunTanHalfAngle = math.tan(math.radians(self.sun.rough_diameter * 0.5))
        c.throughputThreshold = self.gi_ui.throughput_threshold
        return c

    # ---- passes ----
    def submit_commands_gbuffer(self):
        """Stand-in for SubmitCommandsGbuffer (:254-324): primary visibility by ray cast, reference encodings."""
        self._check(self._lib.neb_gbuffer_raycast(self._ctx, C.byref(self.info.camera), C.c_void_p(self.info.stream)),
                    "neb_gbuffer_raycast")

    def submit_commands_pbr_lighting(self):
        """SubmitCommandsPBRLighting (src/DeferredRenderer.cpp:326-394): direct sun light, overwrites radiance[cur]."""
        c = self.global_constants()
        self._check(self._lib.neb_pbr_direct(self._ctx, C.byref(c), C.c_void_p(self.info.stream)), "neb_pbr_direct")

    def submit_commands_hdr_tonemapping(self):
        """SubmitCommandsHDRTonemapping (src/DeferredRenderer.cpp:616-660): radiance[cur] -> LDR plane (RGBA8)."""
        self._check(self._lib.neb_tonemap(self._ctx, C.c_void_p(self.info.stream)), "neb_tonemap")

    def submit_commands_gi_pathtrace(self, rows=None, stream=None):
        c = self.global_constants()
        st = C.c_void_p(self.info.stream if stream is None else stream)
        if rows is None:
            rc = self._lib.neb_gi_trace(self._ctx, C.byref(c), st)
        else:
            rc = self._lib.neb_gi_trace_rows(self._ctx, C.byref(c), rows[0], rows[1], st)
        self._check(rc, "neb_gi_trace")

    def submit_commands_gi_pathtrace_begin(self, rows=None, stream=None):
        """The first half of SubmitCommandsGIPathtrace -- ray generation + the closest-hit walk (neb_gi_trace_begin): touches only the
        G-buffer and GI records, so the next frame's may run beside this frame's shadow pass and SVGF on another stream."""
        c = self.global_constants()
        st = C.c_void_p(self.info.stream if stream is None else stream)
        r0, r1 = (self.svgf.row_begin, self.svgf.row_end) if rows is None else rows
        self._check(self._lib.neb_gi_trace_begin(self._ctx, C.byref(c), r0, r1, st), "neb_gi_trace_begin")

    def submit_commands_gi_pathtrace_finish(self, stream=None, after_shade_event=None):
        """The second half: shading + shadow passes of the dispatch begun longest ago, adding into radiance[cur] (neb_gi_trace_finish).
        after_shade_event: a raw hipEvent_t (e.g. torch.cuda.Event(...).cuda_event) recorded between the two passes."""
        self._check(self._lib.neb_gi_trace_finish(self._ctx, C.c_void_p(self.info.stream if stream is None else stream),
                                                  C.c_void_p(after_shade_event or 0)), "neb_gi_trace_finish")

    def set_defer_resolve(self, on=True):
        """Split the GI dispatch as the reference does (QueryAndTrain ... then Resolve, DeferredRenderer.cpp:560,586)."""
        self.svgf.set_option("gi_defer_resolve", int(on))

    def submit_commands_gi_resolve(self, stream=None):
        self._check(self._lib.neb_gi_resolve(self._ctx, C.c_void_p(self.info.stream if stream is None else stream)), "neb_gi_resolve")

    def submit_commands_svgf_denoising(self):
        if self.dynamic_scene_this_frame and not (self.denoise_while_moving or self.temporal_reprojection):  # :595
            return False
        self._lib.neb_marker_push(b"SVGF Denoising")  # NEB_PIX_SCOPED_EVENT, src/DeferredRenderer.cpp:599
        try:
            if self.reset_history:
                self.reset_history = False
                self.svgf.reset_history(self.info.stream)
            self.svgf.submit_temporal_accumulation(self.info.stream)
            self.svgf.submit_atrous_compute_wavelet(self.info.stream)
        finally:
            self._lib.neb_marker_pop()
        return True

    # ---- introspection ----
    def ray_count(self, reset=False):
        v = C.c_uint64()
        self._check(self._lib.neb_gi_ray_count(self._ctx, C.byref(v), int(reset), C.c_void_p(self.info.stream if self.info else 0)),
                    "neb_gi_ray_count")
        return v.value

    def traversal_stats(self):
        """{rays, node visits and triangle tests of the bounce rays (+ shadow rays while debug hits are on)} as of the
        last ray_count() call."""
        v = (C.c_uint64 * 5)()
        self._check(self._lib.neb_gi_traversal_stats(self._ctx, v), "neb_gi_traversal_stats")
        return dict(zip(("rays", "bounce_nodes", "bounce_tris", "shadow_nodes", "shadow_tris"), [int(x) for x in v]))

    def wave_stats(self):
        """closest-hit pass, as of the last ray_count() with debug hits on: where its waves' loop iterations go"""
        v = (C.c_uint64 * 6)()
        self._check(self._lib.neb_gi_wave_stats(self._ctx, v), "neb_gi_wave_stats")
        return dict(zip(("waves", "iterations", "node_iterations", "node_lanes", "leaf_iterations", "leaf_lanes"), [int(x) for x in v]))

    def node_index_stats(self):
        """closest-hit pass, same collection: node visits by position in the breadth-first node array, and deep stacks"""
        v = (C.c_uint64 * 5)()
        self._check(self._lib.neb_gi_node_index_stats(self._ctx, v), "neb_gi_node_index_stats")
        return dict(zip(("below_64", "below_256", "below_1024", "below_4096", "deep_stack_phases"), [int(x) for x in v]))

    def sun_table_stats(self):
        """{sides proven lit (+normal side / -normal side), shadow rays the table answered as of the last ray_count(), builds}"""
        v = (C.c_uint64 * 4)()
        self._check(self._lib.neb_gi_sun_table_stats(self._ctx, v, C.c_void_p(self.info.stream if self.info else 0)), "neb_gi_sun_table_stats")
        return dict(zip(("lit_plus", "lit_minus", "rays_answered", "builds"), [int(x) for x in v]))

    def sun_table_build_ms(self):
        """device time of the last build of the sun table, or None when none has been built"""
        ms = C.c_float()
        if self._lib.neb_gi_sun_table_build_ms(self._ctx, C.byref(ms)) != 0:
            return None
        return float(ms.value)

    def shadow_tail_mode(self):
        """-> (mode, (us_lists, us_sorted)): 0 the compacted lists take the rays the sun table leaves, 1 the sorted pass, -1 not decided yet for this table"""
        mode, us = C.c_int(), (C.c_float * 2)()
        self._check(self._lib.neb_gi_shadow_tail_mode(self._ctx, C.byref(mode), us), "neb_gi_shadow_tail_mode")
        return int(mode.value), (float(us[0]), float(us[1]))

    def set_debug_hits(self, on=True):
        self.svgf.set_option("gi_debug_hits", int(on))

    def download_hits(self):
        rows = self.svgf.row_end - self.svgf.row_begin
        out = np.zeros((rows, self.width), HIT_DTYPE)
        self._check(self._lib.neb_gi_download_hits(self._ctx, out.ctypes.data_as(C.c_void_p),
                                                   C.c_void_p(self.info.stream if self.info else 0)), "neb_gi_download_hits")
        return out

    def destroy(self):
        self.svgf.destroy()
