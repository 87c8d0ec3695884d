"""ctypes binding of libnebulae_hip.so (include/nebulae_hip.h).

There is no CPU fallback: if the library is missing it is built with hipcc, and if
that fails, or a GPU call is made with no device, the error is raised to the caller.
"""
import ctypes as C
import os

from . import build as _build

NEB_OK = 0
PLANE_RADIANCE, PLANE_NORMAL, PLANE_DEPTH, PLANE_MOMENTS, PLANE_VARIANCE, PLANE_SCRATCH = 0, 1, 2, 3, 4, 5
PLANE_ALBEDO, PLANE_ROUGH_METAL, PLANE_WORLDPOS, PLANE_LDR, PLANE_GEOMETRY = 6, 7, 8, 9, 10
PLANE_HISTORY_LENGTH = 11  # only while option svgf_reproject is 1
PLANE_SUBMESH_ID = 12  # only while option svgf_motion is 1 (NEB_PLANE_SUBMESH_ID: behind the enum, not counted by NEB_PLANE_COUNT)
PLANE_PREV_POINT = 13  # only while option svgf_vertex_motion is 1 (NEB_PLANE_PREV_POINT: behind the enum as well, one slot)
PLANE_DEMOD = 14  # only while option svgf_demodulate is 1 (NEB_PLANE_DEMOD: behind the enum as well, one slot)
SLOT_CURRENT, SLOT_HISTORY = -1, -2


class NebError(RuntimeError):
    pass


class CreateInfo(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("row_begin", C.c_uint32),
                ("row_end", C.c_uint32), ("atrous_levels", C.c_uint32)]


class HaloPlane(C.Structure):
    _fields_ = [("plane", C.c_int32), ("slot", C.c_int32)]


class HaloSwap(C.Structure):
    _fields_ = [("peer", C.c_int32), ("send_row0", C.c_uint32), ("send_row1", C.c_uint32), ("recv_row0", C.c_uint32), ("recv_row1", C.c_uint32)]


class SvgfParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("depthSigma", "alpha", "varianceEps", "phiColor", "phiNormal", "phiDepth")]


_SIGS = {
    # name: (restype, argtypes)
    "neb_create": (C.c_int, [C.POINTER(CreateInfo), C.POINTER(C.c_void_p)]),
    "neb_resize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "neb_destroy": (C.c_int, [C.c_void_p]),
    "neb_last_error": (C.c_char_p, [C.c_void_p]),
    "neb_version": (C.c_char_p, []),
    "neb_marker_push": (C.c_int, [C.c_char_p]),
    "neb_marker_pop": (C.c_int, []),
    "neb_begin_frame": (C.c_int, [C.c_void_p, C.c_uint32]),
    "neb_end_frame": (C.c_int, [C.c_void_p]),
    "neb_current_index": (C.c_int, [C.c_void_p]),
    "neb_history_index": (C.c_int, [C.c_void_p]),
    "neb_svgf_default_params": (C.c_int, [C.POINTER(SvgfParams)]),
    "neb_svgf_set_params": (C.c_int, [C.c_void_p, C.POINTER(SvgfParams)]),
    "neb_svgf_get_params": (C.c_int, [C.c_void_p, C.POINTER(SvgfParams)]),
    "neb_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "neb_get_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                C.POINTER(C.c_uint32)]),
    "neb_upload_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "neb_download_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "neb_stream_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_reset_history": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_snapshot_transforms": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "neb_svgf_snapshot_vertices": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_debug_delta_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]),
    "neb_svgf_level_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "neb_svgf_temporal": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_atrous": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_denoise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "neb_svgf_temporal_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "neb_svgf_atrous_level_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "neb_svgf_atrous_level_planes": (C.c_int, [C.c_void_p, C.c_uint32] + [C.POINTER(C.c_int)] * 4),
    "neb_strips_unique_id": (C.c_int, [C.c_void_p]),
    "neb_strips_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "neb_strips_comm_destroy": (C.c_int, [C.c_void_p]),
    "neb_strips_group_begin": (C.c_int, []),
    "neb_strips_group_end": (C.c_int, []),
    "neb_strips_exchange": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HaloPlane), C.c_uint32, C.POINTER(HaloSwap), C.c_uint32, C.c_void_p]),
    "neb_strips_last_error": (C.c_char_p, []),
}



class StripPlan(C.Structure):
    """neb_strip_plan"""
    _fields_ = [("n_strips", C.c_uint32), ("strip", C.c_uint32), ("scheme", C.c_uint32), ("flags", C.c_uint32)]


class StripPeers(C.Structure):
    """neb_strip_peers"""
    _fields_ = [("up", C.c_void_p), ("down", C.c_void_p)]


class VertexUpdate(C.Structure):
    """neb_vertex_update"""
    _fields_ = [("geometry", C.c_uint32), ("firstVertex", C.c_uint32), ("numVertices", C.c_uint32),
                ("positions", C.c_void_p), ("positionStride", C.c_uint32), ("normals", C.c_void_p), ("normalStride", C.c_uint32),
                ("tangents", C.c_void_p), ("tangentStride", C.c_uint32)]


class SkinDesc(C.Structure):
    """neb_skin_desc"""
    _fields_ = [("geometry", C.c_uint32), ("numJoints", C.c_uint32), ("joints", C.c_void_p), ("jointStride", C.c_uint32),
                ("weights", C.c_void_p), ("weightStride", C.c_uint32)]


class SkinUpdate(C.Structure):
    """neb_skin_update"""
    _fields_ = [("geometry", C.c_uint32), ("jointMatrices", C.POINTER(C.c_float))]


class MorphDesc(C.Structure):
    """neb_morph_desc"""
    _fields_ = [("geometry", C.c_uint32), ("numTargets", C.c_uint32), ("positionDeltas", C.POINTER(C.c_void_p)), ("positionStride", C.c_uint32),
                ("normalDeltas", C.POINTER(C.c_void_p)), ("normalStride", C.c_uint32), ("tangentDeltas", C.POINTER(C.c_void_p)),
                ("tangentStride", C.c_uint32)]


class MorphUpdate(C.Structure):
    """neb_morph_update"""
    _fields_ = [("geometry", C.c_uint32), ("weights", C.POINTER(C.c_float)), ("jointMatrices", C.POINTER(C.c_float))]


class TextureUpdate(C.Structure):
    """neb_texture_update"""
    _fields_ = [("texture", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pitchBytes", C.c_uint32), ("rgba8", C.c_void_p)]


RAYS_ANY_HIT, RAYS_SORT = 1, 2  # NEB_RAYS_*: flags of neb_gi_cast_rays
SHADE_SURFACE, SHADE_RADIANCE = 0, 1  # NEB_SHADE_*: `what` of neb_gi_shade_rays
HIT_FOUND, HIT_ATTRIBUTES, HIT_MATERIAL, HIT_BACKFACE, HIT_NOT_WALKED, HIT_SUN_VISIBLE = 1, 2, 4, 8, 16, 32  # NEB_HIT_*: flags of its records
PATH_ESCAPED, PATH_DIVIDED = 64, 128  # NEB_PATH_*: flags of neb_gi_trace_paths' records, beside NEB_HIT_*
PATH_TAIL = 256  # NEB_PATH_TAIL: the vertex's `added` contains a grid tail / the path took one (neb_gi_trace_paths_tail)
TAIL_FRAME_WEIGHT = 1  # NEB_TAIL_FRAME_WEIGHT: flags of neb_probe_tail
BAKE_SH, BAKE_IRRADIANCE = 0, 1  # NEB_BAKE_*: `what` of neb_gi_probe_rays / neb_gi_bake_probes
PROBE_NOT_BAKED = 1  # NEB_PROBE_NOT_BAKED: flags of neb_probe_record
PROBE_SATURATED = 2  # NEB_PROBE_SATURATED: flags of neb_probe_record, set by neb_gi_accumulate_probes
GATHER_NO_PROBE, GATHER_CLAMPED, GATHER_NOT_GATHERED = 1, 2, 4  # NEB_GATHER_*: flags of neb_probe_gather
INDIRECT_FRAME_WEIGHT = 1  # NEB_INDIRECT_FRAME_WEIGHT: flags of neb_gi_probe_indirect


class Probe(C.Structure):
    """neb_probe"""
    _fields_ = [("position", C.c_float * 3), ("tmin", C.c_float), ("normal", C.c_float * 3), ("tmax", C.c_float)]


class ProbeRecord(C.Structure):
    """neb_probe_record"""
    _fields_ = [("sh", (C.c_float * 3) * 9), ("samples", C.c_uint32), ("hits", C.c_uint32), ("backfaces", C.c_uint32), ("segments", C.c_uint32),
                ("flags", C.c_uint32)]


class ProbeGrid(C.Structure):
    """neb_probe_grid"""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_uint32 * 3), ("backface_limit", C.c_float)]


class ProbeGather(C.Structure):
    """neb_probe_gather"""
    _fields_ = [("irradiance", C.c_float * 3), ("weight", C.c_float), ("corners", C.c_uint32), ("cell", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class ProbeVisibility(C.Structure):
    """neb_probe_visibility"""
    _fields_ = [("moments", (C.c_float * 2) * 64), ("weight", C.c_float * 64)]


class ProbeTailDesc(C.Structure):
    """neb_probe_tail"""
    _fields_ = [("grid", ProbeGrid), ("records", C.c_void_p), ("visibility", C.c_void_p), ("normal_bias", C.c_float), ("flags", C.c_uint32)]


STRIP_SCHEMES = {"once": 0, "per_level": 1, "overlap": 2}
STRIP_RESET_HISTORY = 1


def _gi_sigs():
    from . import scene as S
    return {
        "neb_gi_set_scene": (C.c_int, [C.c_void_p, C.POINTER(S.GeometryDesc), C.c_uint32, C.POINTER(S.MaterialDesc), C.c_uint32,
                                       C.POINTER(S.TextureDesc), C.c_uint32]),
        "neb_gi_build_bvh": (C.c_int, [C.c_void_p, C.c_void_p]),
        "neb_gi_update_transforms": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.c_void_p]),
        "neb_gi_set_visibility": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_uint32, C.c_void_p]),
        "neb_gi_get_visibility": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]),
        "neb_gi_update_materials": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(S.MaterialDesc), C.c_uint32, C.c_void_p]),
        "neb_gi_set_geometry_materials": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_uint32, C.c_void_p]),
        "neb_gi_update_textures": (C.c_int, [C.c_void_p, C.POINTER(TextureUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_update_textures_device": (C.c_int, [C.c_void_p, C.POINTER(TextureUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_debug_texture_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
        "neb_gi_debug_shade_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
        "neb_gi_update_vertices": (C.c_int, [C.c_void_p, C.POINTER(VertexUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_update_vertices_device": (C.c_int, [C.c_void_p, C.POINTER(VertexUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_set_skin": (C.c_int, [C.c_void_p, C.POINTER(SkinDesc), C.c_uint32, C.c_void_p]),
        "neb_gi_skin_vertices": (C.c_int, [C.c_void_p, C.POINTER(SkinUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_set_morph_targets": (C.c_int, [C.c_void_p, C.POINTER(MorphDesc), C.c_uint32, C.c_void_p]),
        "neb_gi_morph_vertices": (C.c_int, [C.c_void_p, C.POINTER(MorphUpdate), C.c_uint32, C.c_void_p]),
        "neb_gi_download_vertices": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float), C.c_void_p]),
        "neb_gi_update_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_scene_box": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "neb_gi_scene_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "neb_gi_bvh_depth": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
        "neb_gi_build_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
        "neb_gi_build_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
        "neb_gi_scene_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_trace": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.c_void_p]),
        "neb_gi_trace_rows": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.c_uint32, C.c_uint32, C.c_void_p]),
        "neb_gi_resolve": (C.c_int, [C.c_void_p, C.c_void_p]),
        "neb_gi_trace_begin": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.c_uint32, C.c_uint32, C.c_void_p]),
        "neb_gi_trace_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
        "neb_gi_ray_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_void_p]),
        "neb_gi_traversal_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_wave_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_node_index_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_debug_set_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
        "neb_gi_debug_sun_walk_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "neb_gi_sun_table_build_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
        "neb_gi_shadow_tail_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
        "neb_gi_sun_table_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
        "neb_gi_download_hits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
        "neb_debug_sort_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
        "neb_pbr_direct": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.c_void_p]),
        "neb_tonemap": (C.c_int, [C.c_void_p, C.c_void_p]),
        "neb_gbuffer_raycast": (C.c_int, [C.c_void_p, C.POINTER(S.CameraDesc), C.c_void_p]),
        "neb_gi_cast_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "neb_gi_shade_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants), C.c_void_p, C.c_void_p]),
        "neb_gi_trace_paths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants), C.c_void_p, C.c_void_p, C.c_void_p]),
        "neb_gi_probe_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "neb_gi_bake_probes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants), C.c_void_p, C.c_void_p]),
        "neb_gi_trace_paths_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants), C.POINTER(ProbeTailDesc), C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
        "neb_gi_bake_probes_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(S.GIConstants),
                                              C.POINTER(ProbeTailDesc), C.c_void_p, C.c_void_p]),
        "neb_gi_probe_grid": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
        "neb_gi_accumulate_probes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
        "neb_gi_gather_probes": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "neb_gbuffer_points": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "neb_gi_probe_indirect": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.POINTER(S.GIConstants), C.c_uint32, C.c_void_p]),
        "neb_gi_probe_indirect_rows": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.POINTER(S.GIConstants), C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.c_void_p]),
        "neb_gi_bake_visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
        "neb_gi_accumulate_visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
        "neb_gi_gather_probes_visible": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p,
                                                   C.c_void_p]),
        "neb_gi_probe_indirect_visible": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_float, C.POINTER(S.GIConstants), C.c_uint32,
                                                    C.c_void_p]),
        "neb_gi_probe_indirect_visible_rows": (C.c_int, [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_float, C.POINTER(S.GIConstants),
                                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
        "neb_svgf_set_camera": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(S.CameraDesc)]),
        "neb_strip_frame": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.c_void_p, C.POINTER(StripPlan), C.c_void_p]),
        "neb_strip_frame_begin": (C.c_int, [C.c_void_p, C.POINTER(S.GIConstants), C.POINTER(StripPlan), C.POINTER(StripPeers), C.c_void_p]),
        "neb_strip_frame_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StripPlan), C.POINTER(StripPeers), C.c_void_p]),
        "neb_strip_rows": (C.c_int, [C.c_void_p, C.POINTER(StripPlan), C.POINTER(C.c_uint32)]),
    }


_LIB = None


def exported_symbols():
    return sorted(set(_SIGS) | set(_gi_sigs()))


def load(build_if_missing=True):
    """Load (building first if needed) libnebulae_hip.so.  Raises if it cannot be had."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("NEB_LIB_PATH")  # tuning only: A/B another build of the same sources (still the HIP library)
    if not path:
        path = _build.LIB_PATH
        if build_if_missing and _build.needs_build():
            _build.build()
    if not os.path.exists(path):
        raise NebError(f"{path} is missing and could not be built; nebulae_amd has no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in {**_SIGS, **_gi_sigs()}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(lib, ctx, rc, what):
    if rc != NEB_OK:
        msg = lib.neb_last_error(ctx)
        raise NebError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
