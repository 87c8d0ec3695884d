// svgf_reproject.h -- the two validity constants of the reprojecting temporal pass (option "svgf_reproject", see
// neb_svgf_set_camera in include/nebulae_hip.h).  The only place they are defined: tests/reproject_ref.py reads them from here.
#pragma once

namespace neb {

// a history tap counts only if the geometric normals of the pixel and of the tap have dot >= this (about 25.8 degrees)
constexpr float kReprojNormalCos = 0.9f;
// ... and the tap's world point lies within this fraction of the point's linear depth (in the history camera) of the pixel's plane
constexpr float kReprojPlaneTol = 0.01f;

} // namespace neb
