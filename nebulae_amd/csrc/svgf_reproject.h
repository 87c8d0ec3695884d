// svgf_reproject.h -- the two validity constants of the reprojecting temporal pass (option "svgf_reproject", see
// neb_svgf_set_camera in include/nebulae_hip.h).  The only place they are defined: tests/reproject_ref.py reads them from here.
// Below them, the layout of the per-geometry delta table of option "svgf_motion" (tests/motion_ref.py reads it from here).
#pragma once

namespace neb {

// a history tap counts only if the geometric normals of the pixel and of the tap have dot >= this (about 25.8 degrees)
constexpr float kReprojNormalCos = 0.9f;
// ... and the tap's world point lies within this fraction of the point's linear depth (in the history camera) of the pixel's plane
constexpr float kReprojPlaneTol = 0.01f;

// One entry of the delta table (reproj_delta_kernel -> svgf_temporal_reproject_kernel<ReprojMode::Submesh>): 128 bytes = 8 float4.
//   float4 0      {flag as uint32 bits, 0, 0, 0}
//   float4 1 .. 3 D, 4 rows x 3 columns in row-major order: P_h = (P, 1) . D  (rows 0 .. 2 the 3x3, row 3 the translation)
//   float4 4 .. 6 K, 3 rows x 3 columns in row-major order, then three zeros: N_h = normalise(N . K)
//   float4 7      zeros
constexpr int kReprojDeltaFloat4 = 8;
constexpr unsigned kReprojDeltaSame = 0;     // the two matrices are equal bit for bit: D = K = identity, not read
constexpr unsigned kReprojDeltaMoved = 1;    // the geometry moved
constexpr unsigned kReprojDeltaSingular = 2; // a matrix is singular or not finite: D = K = 0, its pixels take no history
constexpr unsigned kReprojNoSubmesh = 0xFFFFFFFFu; // NEB_PLANE_SUBMESH_ID where depth holds no surface
// NEB_PLANE_PREV_POINT .w where the pixel has no per-vertex motion (option "svgf_vertex_motion"): two half NaNs, which oct_pack of a
// finite normal never yields (its components lie in [-1, 1])
constexpr unsigned kReprojNoPrevPoint = 0xFFFFFFFFu;

} // namespace neb
