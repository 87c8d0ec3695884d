// gi_refit.hip -- moving submeshes: new instance transforms, the tree kept (neb_gi_update_transforms).
//
// Reference: RTAccelerationStructureBuilder::CreateTlas with a valid updateTlas (src/nri/raytracing/RTAccelerationStructureBuilder.cpp:100-130):
// the build re-runs with PERFORM_UPDATE, new instance transforms replace the old ones in place, the BLASes are not touched.  Here the
// acceleration structure is ONE tree over world-space triangles, so the counterpart is: bake the moved submeshes' triangles again on the
// device (same operation order as the host bake of neb_gi_set_scene, same bits), refit the boxes of the 128-byte nodes bottom-up, one
// launch per level, and quantise the 64-byte nodes again.  Topology, node numbering, leaf order and depth stay.
//
// neb_gi_update_vertices has NO reference counterpart: the reference builds its BLASes without ALLOW_UPDATE
// (RTAccelerationStructureBuilder.cpp:79), so a deformed mesh means new BLASes there.  Here a deformation is the same refit with
// another way in: new object-space vertices are scattered into the device pools, the stamped geometries are baked again by the
// very rebake_kernel of the transform path, and the normal / tangent words of their 128-byte shading records are rewritten.
//
// neb_gi_update_vertices_device is that update with sources the host never reads: a check kernel validates them, the
// scatter reads them where they lie, geom_box_kernel reduces the boxes the host used to fold from h_pos, and one small copy at the end
// of the chain brings {refusal word, boxes} back to a pinned result record the host harvests later (gi_harvest_results).
//
// neb_gi_set_skin / neb_gi_skin_vertices are the producer such a host otherwise brings itself: joints, weights and the
// bind pose of a geometry stay on the device, a call hands over one palette of joint matrices per geometry, skin_check_kernel and
// skin_scatter_kernel stand where the check and the scatter of the device-sourced update stand, and the rest of its chain follows.
//
// neb_gi_set_morph_targets / neb_gi_morph_vertices are the same producer for glTF morph targets: per-target delta streams
// and the rest pose of a geometry stay on the device, a call hands over one weight per target -- compacted on the host to the targets
// that act -- and, for a skinned geometry, optionally its palette: morph_check_kernel and morph_scatter_kernel blend the rest pose and,
// with a palette, put the blend through the skin's own arithmetic in the place of its bind pose (glTF's order: morph, then skin).
//
// neb_gi_set_visibility is the reference's InstanceMask = 0 in the TLAS update it already runs (RTCommon.h:90 sets 0xFF,
// RTAccelerationStructureBuilder.cpp:100-130 is the PERFORM_UPDATE build): a word per geometry says whether its triangles exist for the rays.
// visibility_apply_kernel stands where refit_apply_kernel stands; rebake_kernel gives the slots of a hidden geometry triangles no ray can hit,
// refit_level_kernel leaves them out of the boxes, and every other update call goes through the same two kernels: hidden stays hidden.
//
// What the six update calls share is written once.  On the device: lane_range (a lane's range by bisection) and source_lane,
// refuse_unless_finite (the refusal of the three check kernels), stamp_geometry and store_vertex (the end of the three scatter kernels),
// skin_vertex (the skin kernels, and the skinned arm of the morph kernels).  On the host: geometry_named_once, collect_vertex_spans and
// palette_finite for the refusals; UpdateCall with update_begin, update_touch, update_record_init, stage_slot_release and update_finish
// for the chain -- each entry point keeps its own order of enqueues between them --; setup_fresh_blocks for the two set-up calls.
#include <algorithm>

#include "gi_device.h"

namespace neb {

// lane k: entry k of the update -> the geometry's 4x4, DevGeom::m, ShadeHeader::m, and its stamp
__global__ void refit_apply_kernel(const GiState::StageEntry* __restrict__ stage, uint32_t n, uint32_t n_geoms, uint32_t epoch, float* __restrict__ xf,
                                   DevGeom* __restrict__ geoms, ShadeHeader* __restrict__ heads, uint32_t* __restrict__ geom_epoch)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t gi = stage[k].geom;
    if (gi >= n_geoms)
        return;
    float m[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
        m[q] = stage[k].m[q];
#pragma unroll
    for (int q = 0; q < 16; ++q)
        xf[16 * (size_t)gi + q] = m[q];
    const float m3[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        geoms[gi].m[q] = m3[q];
        heads[gi].m[q] = m3[q];
    }
    geom_epoch[gi] = epoch;
}

// lane k: entry k of neb_gi_set_visibility (StageEntry::pad[0] = the new flag) -> the geometry's visibility word, and its stamp
__global__ void visibility_apply_kernel(const GiState::StageEntry* __restrict__ stage, uint32_t n, uint32_t n_geoms, uint32_t epoch,
                                        uint32_t* __restrict__ visible, uint32_t* __restrict__ geom_epoch)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t gi = stage[k].geom;
    if (gi >= n_geoms)
        return;
    visible[gi] = stage[k].pad[0] ? 1u : 0u;
    geom_epoch[gi] = epoch;
}
// lane gi: a hidden geometry is stamped (the end of a build: the fresh tree holds every triangle, the hidden ones leave it again)
__global__ void visibility_stamp_kernel(uint32_t n_geoms, uint32_t epoch, const uint32_t* __restrict__ visible, uint32_t* __restrict__ geom_epoch)
{
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi < n_geoms && !visible[gi])
        geom_epoch[gi] = epoch;
}

// world = (p, 1) * M: gi_bake_point (gi_internal.h) with every rounding spelled out, same bits as the host.  HIP's __fmul_rn /
// __fadd_rn are plain operators, and with the compiler's default contraction mode the back end fuses a product into the sum that
// takes it whatever a pragma says: each product passes through an empty asm statement, which the optimiser cannot see through
// (checked in the ISA: v_mul_f32 / v_add_f32 only).
__device__ __forceinline__ float rounded_product(float a, float b)
{
    float p = __fmul_rn(a, b);
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ float3 bake_point(const float* __restrict__ m, const float* __restrict__ p)
{
    const float a0 = p[0], a1 = p[1], a2 = p[2];
    float3 w;
    w.x = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(a0, m[0]), rounded_product(a1, m[4])), rounded_product(a2, m[8])), m[12]);
    w.y = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(a0, m[1]), rounded_product(a1, m[5])), rounded_product(a2, m[9])), m[13]);
    w.z = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(a0, m[2]), rounded_product(a1, m[6])), rounded_product(a2, m[10])), m[14]);
    return w;
}

// one lane per leaf-order triangle slot: a slot of a moved geometry gets its triangle baked again, {geom, prim} stay.
// A stamped geometry that is hidden (neb_gi_set_visibility) gets the triangle no ray can hit instead: v0 = e1 = e2 = +0, det == 0 in
// intersect_tri_regs whatever the ray, every word finite; the id words keep their bits, so that showing it finds {geom, prim} again.
__global__ void rebake_kernel(float4* __restrict__ tris, uint32_t n_slots, uint32_t n_geoms, uint32_t epoch, const uint32_t* __restrict__ geom_epoch,
                              const DevGeom* __restrict__ geoms, const uint32_t* __restrict__ indices, const float* __restrict__ pos,
                              const float* __restrict__ xf, const uint32_t* __restrict__ visible)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots)
        return;
    const float4 ids = tris[3 * (size_t)i + 2];
    const uint32_t gi = __float_as_uint(ids.y), prim = __float_as_uint(ids.z);
    if (gi >= n_geoms || geom_epoch[gi] != epoch)
        return;
    if (!visible[gi]) {
        tris[3 * (size_t)i] = make_float4(0.f, 0.f, 0.f, 0.f);
        tris[3 * (size_t)i + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        tris[3 * (size_t)i + 2] = make_float4(0.f, ids.y, ids.z, ids.w);
        return;
    }
    const uint32_t first = geoms[gi].firstIndex + 3u * prim, vb = geoms[gi].vertexBase;
    const float* m = xf + 16 * (size_t)gi;
    const float3 w0 = bake_point(m, pos + 3 * (size_t)(vb + indices[first]));
    const float3 w1 = bake_point(m, pos + 3 * (size_t)(vb + indices[first + 1]));
    const float3 w2 = bake_point(m, pos + 3 * (size_t)(vb + indices[first + 2]));
    tris[3 * (size_t)i] = make_float4(w0.x, w0.y, w0.z, __fsub_rn(w1.x, w0.x));
    tris[3 * (size_t)i + 1] = make_float4(__fsub_rn(w1.y, w0.y), __fsub_rn(w1.z, w0.z), __fsub_rn(w2.x, w0.x), __fsub_rn(w2.y, w0.y));
    tris[3 * (size_t)i + 2] = make_float4(__fsub_rn(w2.z, w0.z), ids.y, ids.z, ids.w);
}

// ---- what the per-vertex kernels share ----
// THE lane lookup: the index of the last range with first_lane <= k, by bisection (n ranges, ascending by first_lane, none empty).
// Range: GiState::DeformRange or GiState::RollSpan.
template <typename Range>
__device__ __forceinline__ uint32_t lane_range(const Range* __restrict__ ranges, uint32_t n, uint32_t k)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ranges[mid].first_lane <= k)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
// The lane's range, the source beside it (GiState::SkinSource / MorphSource) and its vertex inside the geometry; false: the lane has nothing to do.
template <typename Source>
__device__ __forceinline__ bool source_lane(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const Source* __restrict__ sources, uint32_t k,
                                            uint32_t n_geoms, GiState::DeformRange& r, Source& s, uint32_t& j)
{
    const uint32_t i = lane_range(ranges, n_ranges, k);
    r = ranges[i];
    s = sources[i];
    j = k - r.first_lane;
    return j < r.count && j < s.n_verts && r.geom < n_geoms;
}
// THE refusal: the object-space position a, and its world point under the geometry's matrix m, must be finite within gi_bake_point's
// bound -- what neb_gi_update_vertices checks on the host.  A failing lane sets the call's refusal word.
__device__ __forceinline__ void refuse_unless_finite(const float a[3], const float* __restrict__ m, uint32_t* __restrict__ refused)
{
    const float3 w = bake_point(m, a);
    const bool ok = fabsf(a[0]) <= 3.0e38f && fabsf(a[1]) <= 3.0e38f && fabsf(a[2]) <= 3.0e38f && fabsf(w.x) <= 3.0e38f && fabsf(w.y) <= 3.0e38f &&
                    fabsf(w.z) <= 3.0e38f; // (a NaN fails every comparison)
    if (!ok)
        atomicOr(refused, 1u);
}
// THE stamp (lane 0 of a range): the geometry belongs to update `epoch`, and -- option svgf_vertex_motion, deform_dirty null with the
// option off -- its dirty word is set, which gbuffer_kernel reads and deform_roll_kernel clears.
__device__ __forceinline__ void stamp_geometry(uint32_t geom, uint32_t epoch, uint32_t* __restrict__ geom_epoch, uint32_t* __restrict__ deform_dirty)
{
    geom_epoch[geom] = epoch;
    if (deform_dirty)
        deform_dirty[geom] = 1u;
}
// vertex v of the pools: the position, and the normal (3 floats) and the tangent (4 floats) where the pointer is not null
__device__ __forceinline__ void store_vertex(float* __restrict__ pos, float* __restrict__ normals, float* __restrict__ tangents, size_t v, const float* p,
                                             const float* n, const float* t)
{
    pos[3 * v] = p[0], pos[3 * v + 1] = p[1], pos[3 * v + 2] = p[2];
    if (n)
        normals[3 * v] = n[0], normals[3 * v + 1] = n[1], normals[3 * v + 2] = n[2];
    if (t)
        tangents[4 * v] = t[0], tangents[4 * v + 1] = t[1], tangents[4 * v + 2] = t[2], tangents[4 * v + 3] = t[3];
}

// One lane per staged vertex: the compact streams of the update -> the object-space position pool and the normal / tangent pools.
// The lane finds its range by lane_range; lane 0 of a range stamps its geometry.
// `stage` is the pinned slot itself or its device copy ("gi_deform_stage").
// DEVICE_SRC: the vertices are not in the slot but where sources[range] points (strided device memory), and the whole launch leaves
// at once when deform_check_kernel has set the call's refusal word -- nothing is written, no geometry is stamped, and every kernel
// behind this one acts on stamped geometries only: a refused update is a no-op on the device.
template <bool DEVICE_SRC>
__global__ void deform_scatter_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const float* __restrict__ data, uint32_t n_lanes,
                                      uint32_t n_pool, uint32_t n_geoms, uint32_t epoch, float* __restrict__ pos, float* __restrict__ normals,
                                      float* __restrict__ tangents, uint32_t* __restrict__ geom_epoch,
                                      const GiState::DeformSource* __restrict__ sources, const uint32_t* __restrict__ refused,
                                      uint32_t* __restrict__ deform_dirty)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    if constexpr (DEVICE_SRC)
        if (*refused)
            return;
    const uint32_t i = lane_range(ranges, n_ranges, k);
    const GiState::DeformRange r = ranges[i];
    const uint32_t j = k - r.first_lane;
    if (j >= r.count || r.dst + j >= n_pool)
        return;
    const float *sp, *sn = nullptr, *st = nullptr;
    if constexpr (DEVICE_SRC) {
        const GiState::DeformSource s = sources[i];
        sp = reinterpret_cast<const float*>(s.pos + (size_t)j * s.pos_stride);
        if (r.nrm_off != GiState::kNoStream)
            sn = reinterpret_cast<const float*>(s.nrm + (size_t)j * s.nrm_stride);
        if (r.tan_off != GiState::kNoStream)
            st = reinterpret_cast<const float*>(s.tan + (size_t)j * s.tan_stride);
    } else {
        sp = data + r.pos_off + 3 * (size_t)j;
        if (r.nrm_off != GiState::kNoStream)
            sn = data + r.nrm_off + 3 * (size_t)j;
        if (r.tan_off != GiState::kNoStream)
            st = data + r.tan_off + 4 * (size_t)j;
    }
    store_vertex(pos, normals, tangents, (size_t)r.dst + j, sp, sn, st);
    if (j == 0 && r.geom < n_geoms)
        stamp_geometry(r.geom, epoch, geom_epoch, deform_dirty);
}

// Option svgf_vertex_motion: one lane per vertex of the spans updated since the last roll, found by lane_range over the spans' first
// lanes.  The lane copies its vertex's position and normal from the live pools to the previous pools; lane 0 of a span clears its
// geometry's dirty word.  Enqueued behind gbuffer_kernel, which has read both.
__global__ void deform_roll_kernel(const GiState::RollSpan* __restrict__ spans, uint32_t n_spans, uint32_t n_lanes, uint32_t n_pool, uint32_t n_geoms,
                                   const float* __restrict__ pos, const float* __restrict__ normals, float* __restrict__ pos_prev,
                                   float* __restrict__ nrm_prev, uint32_t* __restrict__ deform_dirty)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    const GiState::RollSpan r = spans[lane_range(spans, n_spans, k)];
    const uint32_t j = k - r.first_lane;
    if (j >= r.count || r.dst + j >= n_pool)
        return;
    const size_t v = (size_t)r.dst + j;
    pos_prev[3 * v] = pos[3 * v], pos_prev[3 * v + 1] = pos[3 * v + 1], pos_prev[3 * v + 2] = pos[3 * v + 2];
    nrm_prev[3 * v] = normals[3 * v], nrm_prev[3 * v + 1] = normals[3 * v + 1], nrm_prev[3 * v + 2] = normals[3 * v + 2];
    if (j == 0 && r.geom < n_geoms)
        deform_dirty[r.geom] = 0u;
}

// One lane per leaf-order slot: the record of a slot whose geometry is stamped gets its normal and tangent words again from the pools,
// in pack_shade_records_kernel's layout (r0-r2 .xyz the normals, r3-r5 the tangents).  Every other word keeps its bits: the UV words
// (r0-r2 .w, r6.xyz), geometry + lit bits (r6.w), primitive and hints (r7).  The record of a geometry without attributes stays zeros.
__global__ void repack_records_kernel(float* __restrict__ shade, const float4* __restrict__ tris, uint32_t n_slots, uint32_t n_geoms, uint32_t epoch,
                                      const uint32_t* __restrict__ geom_epoch, const DevGeom* __restrict__ geoms, const uint32_t* __restrict__ indices,
                                      const float* __restrict__ normals, const float* __restrict__ tangents)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots)
        return;
    const float4 ids = tris[3 * (size_t)i + 2];
    const uint32_t gi = __float_as_uint(ids.y), prim = __float_as_uint(ids.z);
    if (gi >= n_geoms || geom_epoch[gi] != epoch || !geoms[gi].valid)
        return;
    const uint32_t first = geoms[gi].firstIndex + 3u * prim, vb = geoms[gi].vertexBase;
    float* rec = shade + 32 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t v = (size_t)vb + indices[first + k];
        rec[4 * k] = normals[3 * v], rec[4 * k + 1] = normals[3 * v + 1], rec[4 * k + 2] = normals[3 * v + 2];
        reinterpret_cast<float4*>(rec)[3 + k] = make_float4(tangents[4 * v], tangents[4 * v + 1], tangents[4 * v + 2], tangents[4 * v + 3]);
    }
}

// min / max in the order the builder's LDS atomics use (-0 below +0): a refit over unmoved boxes reproduces the builder's bits
__device__ __forceinline__ uint32_t refit_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float refit_min(float a, float b) { return refit_ordered(b) < refit_ordered(a) ? b : a; }
__device__ __forceinline__ float refit_max(float a, float b) { return refit_ordered(b) > refit_ordered(a) ? b : a; }
__device__ __forceinline__ float refit_min4(const float4 v) { return refit_min(refit_min(v.x, v.y), refit_min(v.z, v.w)); }
__device__ __forceinline__ float refit_max4(const float4 v) { return refit_max(refit_max(v.x, v.y), refit_max(v.z, v.w)); }

// One lane per source vertex of a device-sourced update, the ranges of deform_scatter_kernel: the source position goes through
// refuse_unless_finite under the geometry's current matrix.
__global__ void deform_check_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const GiState::DeformSource* __restrict__ sources,
                                    uint32_t n_lanes, uint32_t n_geoms, const float* __restrict__ xf, uint32_t* __restrict__ refused)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    const uint32_t i = lane_range(ranges, n_ranges, k);
    const GiState::DeformRange r = ranges[i];
    const uint32_t j = k - r.first_lane;
    if (j >= r.count || r.geom >= n_geoms)
        return;
    const GiState::DeformSource s = sources[i];
    const float* sp = reinterpret_cast<const float*>(s.pos + (size_t)j * s.pos_stride);
    const float a[3] = {sp[0], sp[1], sp[2]};
    refuse_unless_finite(a, xf + 16 * (size_t)r.geom, refused);
}

// ---- skinning ----
// The blended matrix of vertex j, THE written order: S[q] = ((w0 J0[q] + w1 J1[q]) + w2 J2[q]) + w3 J3[q] for rows 0-3, columns 0-2, every
// product and every sum rounded by itself (rounded_product, __fadd_rn).  Column 3 of the joint matrices is never read.  A joint index is
// clamped to the palette (neb_gi_set_skin refused the skin that has one beyond it: the clamp only keeps the read inside the buffer).
__device__ __forceinline__ void skin_blend(const GiState::SkinSource& s, const float* __restrict__ palette, uint32_t j, float S[16])
{
    const float4 w = reinterpret_cast<const float4*>(s.block)[j];
    const uint2 jj = reinterpret_cast<const uint2*>(s.block + 32 * (size_t)s.n_verts)[j];
    const uint32_t last = s.n_joints - 1u;
    // (a matrix is one 64-byte line of the palette buffer: four 16-byte loads each; column 3 comes along and is dropped)
    const float4* J0 = reinterpret_cast<const float4*>(palette) + 4 * (size_t)(s.pal_first + min(jj.x & 0xffffu, last));
    const float4* J1 = reinterpret_cast<const float4*>(palette) + 4 * (size_t)(s.pal_first + min(jj.x >> 16, last));
    const float4* J2 = reinterpret_cast<const float4*>(palette) + 4 * (size_t)(s.pal_first + min(jj.y & 0xffffu, last));
    const float4* J3 = reinterpret_cast<const float4*>(palette) + 4 * (size_t)(s.pal_first + min(jj.y >> 16, last));
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const float4 a = J0[row], b = J1[row], c = J2[row], d = J3[row];
        S[4 * row] = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(w.x, a.x), rounded_product(w.y, b.x)), rounded_product(w.z, c.x)), rounded_product(w.w, d.x));
        S[4 * row + 1] = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(w.x, a.y), rounded_product(w.y, b.y)), rounded_product(w.z, c.y)), rounded_product(w.w, d.y));
        S[4 * row + 2] = __fadd_rn(__fadd_rn(__fadd_rn(rounded_product(w.x, a.z), rounded_product(w.y, b.z)), rounded_product(w.z, c.z)), rounded_product(w.w, d.z));
        S[4 * row + 3] = 0.f;
    }
}
__device__ __forceinline__ const float* skin_bind_pos(const GiState::SkinSource& s, uint32_t j)
{
    return reinterpret_cast<const float*>(s.block + 40 * (size_t)s.n_verts) + 3 * (size_t)j;
}
// n' = n * upper 3x3 of S, left to right, not renormalised (the shading normalises every vertex normal at the hit)
__device__ __forceinline__ float3 skin_direction(const float* S, float x, float y, float z)
{
    float3 d;
    d.x = __fadd_rn(__fadd_rn(rounded_product(x, S[0]), rounded_product(y, S[4])), rounded_product(z, S[8]));
    d.y = __fadd_rn(__fadd_rn(rounded_product(x, S[1]), rounded_product(y, S[5])), rounded_product(z, S[9]));
    d.z = __fadd_rn(__fadd_rn(rounded_product(x, S[2]), rounded_product(y, S[6])), rounded_product(z, S[10]));
    return d;
}
// THE skinned vertex under the blended matrix S: the position by bake_point, then -- where the caller has them -- the normal and the
// tangent's xyz by skin_direction, in this order; the tangent's w keeps its bits.  The skin kernels hand the bind pose, the morph kernels
// the blended rest pose (glTF's order: morph, then skin).
__device__ __forceinline__ float3 skin_vertex(const float* S, float3 p, bool attrs = false, float3* n = nullptr, float4* t = nullptr)
{
    const float a[3] = {p.x, p.y, p.z};
    p = bake_point(S, a);
    if (attrs) {
        *n = skin_direction(S, n->x, n->y, n->z);
        const float3 td = skin_direction(S, t->x, t->y, t->z);
        t->x = td.x, t->y = td.y, t->z = td.z;
    }
    return p;
}

// One lane per vertex of the skinned geometries a call names: the skinned position goes through refuse_unless_finite under the
// geometry's current matrix (deform_check_kernel's contract).
__global__ void skin_check_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const GiState::SkinSource* __restrict__ sources,
                                  const float* __restrict__ palette, uint32_t n_lanes, uint32_t n_geoms, const float* __restrict__ xf,
                                  uint32_t* __restrict__ refused)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    GiState::DeformRange r;
    GiState::SkinSource s;
    uint32_t j;
    if (!source_lane(ranges, n_ranges, sources, k, n_geoms, r, s, j) || !s.n_joints)
        return;
    float S[16];
    skin_blend(s, palette, j, S);
    const float* bp = skin_bind_pos(s, j);
    const float3 a3 = skin_vertex(S, make_float3(bp[0], bp[1], bp[2]));
    const float a[3] = {a3.x, a3.y, a3.z};
    refuse_unless_finite(a, xf + 16 * (size_t)r.geom, refused);
}

// One lane per vertex: position, normal and tangent from the BIND pose (never the live pools: a chain of calls does not drift) under the
// blended matrix, into the pools.  The whole launch leaves at once when skin_check_kernel has set the refusal word.  Lane 0 of a range
// stamps its geometry and, with option svgf_vertex_motion, sets its dirty word -- as deform_scatter_kernel does.  A geometry set without
// its attribute streams (attrs == 0) gets positions only.
__global__ void skin_scatter_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const GiState::SkinSource* __restrict__ sources,
                                    const float* __restrict__ palette, uint32_t n_lanes, uint32_t n_pool, uint32_t n_geoms, uint32_t epoch,
                                    float* __restrict__ pos, float* __restrict__ normals, float* __restrict__ tangents, uint32_t* __restrict__ geom_epoch,
                                    const uint32_t* __restrict__ refused, uint32_t* __restrict__ deform_dirty)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    if (*refused)
        return;
    GiState::DeformRange r;
    GiState::SkinSource s;
    uint32_t j;
    if (!source_lane(ranges, n_ranges, sources, k, n_geoms, r, s, j) || !s.n_joints || r.dst + j >= n_pool)
        return;
    float S[16];
    skin_blend(s, palette, j, S);
    const float* bp = skin_bind_pos(s, j);
    float3 p = make_float3(bp[0], bp[1], bp[2]), n = make_float3(0.f, 0.f, 0.f);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s.attrs) {
        const float* bn = reinterpret_cast<const float*>(s.block + 52 * (size_t)s.n_verts) + 3 * (size_t)j;
        n = make_float3(bn[0], bn[1], bn[2]);
        t = reinterpret_cast<const float4*>(s.block + 16 * (size_t)s.n_verts)[j];
    }
    p = skin_vertex(S, p, s.attrs != 0u, &n, &t);
    if (s.attrs)
        store_vertex(pos, normals, tangents, (size_t)r.dst + j, &p.x, &n.x, &t.x);
    else
        store_vertex(pos, normals, tangents, (size_t)r.dst + j, &p.x, nullptr, nullptr);
    if (j == 0)
        stamp_geometry(r.geom, epoch, geom_epoch, deform_dirty);
}

// ---- morph targets ----
// THE written order of one float3 stream: v[c] = v[c] + w * d_k[c] for each pair {k, w} of the lane's active list, in the list's order,
// every product and every sum rounded by itself.  The order of the sums is fixed, the loads are not: four targets' deltas are fetched
// before the first of their dependent adds, so that four round trips are in flight, not one.  `deltas` is the target-major stream
// [n_targets][n_verts] float3; a target index is clamped to the stream (the host writes none beyond it: the clamp only keeps the read inside).
__device__ __forceinline__ void morph_accumulate(const float* __restrict__ deltas, const GiState::MorphSource& s, uint32_t j, const uint2* __restrict__ act,
                                                 float& x, float& y, float& z)
{
    const uint32_t last = s.n_targets - 1u;
    uint32_t a = 0;
    for (; a + 4u <= s.n_active; a += 4u) {
        float w[4], d[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint2 p = act[a + q];
            const float* sp = deltas + 3 * ((size_t)min(p.x, last) * s.n_verts + j);
            w[q] = __uint_as_float(p.y);
            d[q][0] = sp[0], d[q][1] = sp[1], d[q][2] = sp[2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x = __fadd_rn(x, rounded_product(w[q], d[q][0]));
            y = __fadd_rn(y, rounded_product(w[q], d[q][1]));
            z = __fadd_rn(z, rounded_product(w[q], d[q][2]));
        }
    }
    for (; a < s.n_active; ++a) {
        const uint2 p = act[a];
        const float* sp = deltas + 3 * ((size_t)min(p.x, last) * s.n_verts + j);
        const float w = __uint_as_float(p.y), d0 = sp[0], d1 = sp[1], d2 = sp[2];
        x = __fadd_rn(x, rounded_product(w, d0));
        y = __fadd_rn(y, rounded_product(w, d1));
        z = __fadd_rn(z, rounded_product(w, d2));
    }
}
// the streams of a geometry's block (GiState::Morph)
__device__ __forceinline__ const float* morph_rest_pos(const GiState::MorphSource& s) { return reinterpret_cast<const float*>(s.block + 16 * (size_t)s.n_verts); }
__device__ __forceinline__ const float* morph_rest_nrm(const GiState::MorphSource& s) { return reinterpret_cast<const float*>(s.block + 28 * (size_t)s.n_verts); }
__device__ __forceinline__ const float* morph_deltas(const GiState::MorphSource& s, uint32_t stream)
{
    return reinterpret_cast<const float*>(s.block + 40 * (size_t)s.n_verts) + 3 * (size_t)stream * s.n_targets * s.n_verts;
}
__device__ __forceinline__ float3 morph_position(const GiState::MorphSource& s, const uint2* __restrict__ act, uint32_t j)
{
    const float* rp = morph_rest_pos(s) + 3 * (size_t)j;
    float3 m = make_float3(rp[0], rp[1], rp[2]);
    morph_accumulate(morph_deltas(s, 0), s, j, act + s.act_first, m.x, m.y, m.z);
    return m;
}
__device__ __forceinline__ GiState::SkinSource morph_skin(const GiState::MorphSource& s)
{
    return {s.skin_block, s.n_verts, s.pal_first, s.n_joints, 0u, {0u, 0u}};
}

// One lane per vertex of the geometries a morph call names: the final position -- the blend, skinned where the call hands a palette --
// and its world point under the geometry's current matrix must be finite within gi_bake_point's bound; a failing lane sets the call's
// refusal word (deform_check_kernel's contract).
__global__ void morph_check_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const GiState::MorphSource* __restrict__ sources,
                                   const uint2* __restrict__ act, const float* __restrict__ palette, uint32_t n_lanes, uint32_t n_geoms,
                                   const float* __restrict__ xf, uint32_t* __restrict__ refused)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    GiState::DeformRange r;
    GiState::MorphSource s;
    uint32_t j;
    if (!source_lane(ranges, n_ranges, sources, k, n_geoms, r, s, j) || !s.n_targets)
        return;
    float3 m = morph_position(s, act, j);
    if (s.n_joints) {
        float S[16];
        skin_blend(morph_skin(s), palette, j, S);
        m = skin_vertex(S, m);
    }
    const float a[3] = {m.x, m.y, m.z};
    refuse_unless_finite(a, xf + 16 * (size_t)r.geom, refused);
}

// One lane per vertex: m, n, t = the REST pose (never the live pools: a chain of calls does not drift) plus the active targets in the
// written order; into the pools as they are, or -- with a palette -- in the place of the bind pose in skin_scatter_kernel's order, through
// no buffer in between.  The whole launch leaves at once when morph_check_kernel has set the refusal word.  Lane 0 of a range stamps its
// geometry and, with option svgf_vertex_motion, sets its dirty word.  A geometry set without its attribute streams gets positions only;
// targets that carry no normal (tangent) deltas leave the rest normal (tangent), its bits kept.
__global__ void morph_scatter_kernel(const GiState::DeformRange* __restrict__ ranges, uint32_t n_ranges, const GiState::MorphSource* __restrict__ sources,
                                     const uint2* __restrict__ act, const float* __restrict__ palette, uint32_t n_lanes, uint32_t n_pool, uint32_t n_geoms,
                                     uint32_t epoch, float* __restrict__ pos, float* __restrict__ normals, float* __restrict__ tangents,
                                     uint32_t* __restrict__ geom_epoch, const uint32_t* __restrict__ refused, uint32_t* __restrict__ deform_dirty)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lanes)
        return;
    if (*refused)
        return;
    GiState::DeformRange r;
    GiState::MorphSource s;
    uint32_t j;
    if (!source_lane(ranges, n_ranges, sources, k, n_geoms, r, s, j) || !s.n_targets || r.dst + j >= n_pool)
        return;
    float3 m = morph_position(s, act, j);
    const bool attrs = (s.flags & GiState::kMorphAttrs) != 0u;
    float3 n = make_float3(0.f, 0.f, 0.f);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (attrs) {
        const float* rn = morph_rest_nrm(s) + 3 * (size_t)j;
        n = make_float3(rn[0], rn[1], rn[2]);
        t = reinterpret_cast<const float4*>(s.block)[j];
        uint32_t stream = 1;
        if (s.flags & GiState::kMorphNormals)
            morph_accumulate(morph_deltas(s, stream++), s, j, act + s.act_first, n.x, n.y, n.z);
        if (s.flags & GiState::kMorphTangents)
            morph_accumulate(morph_deltas(s, stream), s, j, act + s.act_first, t.x, t.y, t.z);
    }
    if (s.n_joints) {
        float S[16];
        skin_blend(morph_skin(s), palette, j, S);
        m = skin_vertex(S, m, attrs, &n, &t);
    }
    if (attrs)
        store_vertex(pos, normals, tangents, (size_t)r.dst + j, &m.x, &n.x, &t.x);
    else
        store_vertex(pos, normals, tangents, (size_t)r.dst + j, &m.x, nullptr, nullptr);
    if (j == 0)
        stamp_geometry(r.geom, epoch, geom_epoch, deform_dirty);
}

// the result record of a call before its chain: {call, refusal word = 0, entries, 0}, every box word at the neutral element of atomicMin
__global__ void result_init_kernel(uint32_t* __restrict__ res, uint32_t call, uint32_t n_entries)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < GiState::kResultHead + GiState::kResultEntry * n_entries)
        res[i] = i == 0 ? call : i == 2 ? n_entries : i < GiState::kResultHead ? 0u : 0xffffffffu;
}

// The boxes of the listed geometries over their REFERENCED vertices (a vertex no triangle names is no part of the scene): an entry
// owns `per_entry` consecutive blocks of the one-dimensional grid (no limit of 65535 entries as gridDim.y would set), the lanes of its
// blocks stride over the geometry's referenced vertices, object space as stored and world space by bake_point under the current matrix.  The wave folds its 12 keys (refit_ordered; an upper bound as its complement, so that every
// fold is a min) with __shfl_xor, and lane 0 issues one atomicMin per component: 12 atomics per wave, not per lane.
__global__ __launch_bounds__(256) void geom_box_kernel(const uint32_t* __restrict__ list, uint32_t n_entries, uint32_t n_geoms,
                                                       const uint2* __restrict__ ref_spans, const uint32_t* __restrict__ ref_verts, uint32_t n_ref_verts,
                                                       const DevGeom* __restrict__ geoms, const float* __restrict__ pos, uint32_t n_pool,
                                                       const float* __restrict__ xf, uint32_t* __restrict__ entries, uint32_t per_entry)
{
    const uint32_t e = blockIdx.x / per_entry, block = blockIdx.x - e * per_entry;
    if (e >= n_entries)
        return;
    const uint32_t gi = list[e];
    if (gi >= n_geoms)
        return;
    const uint2 span = ref_spans[gi];
    const uint32_t vb = geoms[gi].vertexBase;
    const float* m = xf + 16 * (size_t)gi;
    uint32_t key[GiState::kResultEntry];
#pragma unroll
    for (int q = 0; q < (int)GiState::kResultEntry; ++q)
        key[q] = 0xffffffffu;
    bool any = false;
    for (uint32_t r = block * blockDim.x + threadIdx.x; r < span.y; r += per_entry * blockDim.x) {
        if ((uint64_t)span.x + r >= n_ref_verts)
            break;
        const size_t v = (size_t)vb + ref_verts[span.x + r];
        if (v >= n_pool)
            continue;
        const float a[3] = {pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]};
        const float3 w3 = bake_point(m, a);
        const float w[3] = {w3.x, w3.y, w3.z};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint32_t ka = refit_ordered(a[q]), kw = refit_ordered(w[q]);
            key[q] = min(key[q], ka), key[3 + q] = min(key[3 + q], ~ka);
            key[6 + q] = min(key[6 + q], kw), key[9 + q] = min(key[9 + q], ~kw);
        }
        any = true;
    }
    if (__ballot(any) == 0ull)
        return; // (wave-uniform)
#pragma unroll
    for (int q = 0; q < (int)GiState::kResultEntry; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            key[q] = min(key[q], (uint32_t)__shfl_xor((int)key[q], off));
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int q = 0; q < (int)GiState::kResultEntry; ++q)
            atomicMin(entries + GiState::kResultEntry * (size_t)e + q, key[q]);
    }
}

// One level of the tree, four lanes per node, one per child slot.  A leaf one of whose triangles moved takes the exact bounds of
// its triangles -- the whole triangle also where the slot holds a clipped reference of the splitting pass: conservative.  An inner
// child below which something changed takes the exact min / max of that node's four boxes (its level was refitted by the launch
// before: unused slots are inverted boxes and drop out of min / max by themselves).  Everything else keeps its bits.
// Hidden geometries (neb_gi_set_visibility): a leaf takes the bounds of its VISIBLE triangles, and the inverted box when it has none; an
// inner child all of whose slots are inverted becomes inverted itself (min / max of four inverted boxes).  Such a slot has to come
// back when its geometry is shown, so the slots nothing ever lived in are told by the mask the build wrote (Bvh4Node::pad.x), not by
// their box -- and not by the child word: ~0 is the unused slot and also the leaf {slot 0, one triangle}.
__global__ void refit_level_kernel(Bvh4Node* __restrict__ nodes, uint32_t first, uint32_t count, uint32_t n_nodes, const float4* __restrict__ tris,
                                   uint32_t n_slots, uint32_t n_geoms, uint32_t epoch, const uint32_t* __restrict__ geom_epoch,
                                   uint32_t* __restrict__ node_epoch, const uint32_t* __restrict__ visible)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4u * count)
        return;
    const uint32_t i = first + (t >> 2), q = t & 3u;
    float* nf = reinterpret_cast<float*>(nodes + i);
    if (!(((uint32_t)nodes[i].pad.x >> q) & 1u))
        return; // a slot the build left unused
    const int c = reinterpret_cast<const int*>(nodes + i)[12 + q];
    float lo[3], hi[3];
    if (c < 0) {
        const uint32_t code = (uint32_t)~c, slot = code >> 2, cnt = (code & 3u) + 1u;
        if (slot + cnt > n_slots)
            return;
        bool moved = false;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t gi = __float_as_uint(tris[3 * (size_t)(slot + k) + 2].y);
            moved = moved || (gi < n_geoms && geom_epoch[gi] == epoch);
        }
        if (!moved)
            return;
        for (int ax = 0; ax < 3; ++ax)
            lo[ax] = INFINITY, hi[ax] = -INFINITY;
        for (uint32_t k = 0; k < cnt; ++k) {
            const float4 a = tris[3 * (size_t)(slot + k)], b = tris[3 * (size_t)(slot + k) + 1], d = tris[3 * (size_t)(slot + k) + 2];
            const uint32_t gi = __float_as_uint(d.y);
            if (gi < n_geoms && !visible[gi])
                continue; // (a hidden triangle bounds nothing)
            // (the vertices as the builder's reference_box and the triangle test form them: v0, v0 + e1, v0 + e2)
            const float v[3][3] = {{a.x, a.y, a.z}, {__fadd_rn(a.x, a.w), __fadd_rn(a.y, b.x), __fadd_rn(a.z, b.y)},
                                   {__fadd_rn(a.x, b.z), __fadd_rn(a.y, b.w), __fadd_rn(a.z, d.x)}};
            for (int ax = 0; ax < 3; ++ax) {
                lo[ax] = refit_min(lo[ax], refit_min(v[0][ax], refit_min(v[1][ax], v[2][ax])));
                hi[ax] = refit_max(hi[ax], refit_max(v[0][ax], refit_max(v[1][ax], v[2][ax])));
            }
        }
    } else {
        if ((uint32_t)c >= n_nodes || node_epoch[c] != epoch)
            return;
        const Bvh4Node* ch = nodes + c;
        lo[0] = refit_min4(ch->lox), lo[1] = refit_min4(ch->loy), lo[2] = refit_min4(ch->loz);
        hi[0] = refit_max4(ch->hix), hi[1] = refit_max4(ch->hiy), hi[2] = refit_max4(ch->hiz);
    }
    nf[q] = lo[0], nf[4 + q] = lo[1], nf[8 + q] = lo[2];
    nf[16 + q] = hi[0], nf[20 + q] = hi[1], nf[24 + q] = hi[2];
    node_epoch[i] = epoch; // (up to four lanes store the same word)
}

// ---- what the two kinds of update share on the host ----
// the scene box: the union of the geometries' exact boxes, as neb_gi_set_scene folds it
// -- of the VISIBLE ones (neb_gi_set_visibility): the box of a scene built without the hidden ones.  Nothing visible: the zero box of
// an empty scene, and no sun table is built (GiState::nothing_visible).
void gi_fold_scene_box(const GiState* g, bool visible_only, float lo[3], float hi[3])
{
    float smin[3] = {3.4e38f, 3.4e38f, 3.4e38f}, smax[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    bool any = false;
    for (size_t gi = 0; gi < g->h_geoms.size(); ++gi) {
        const GiState::HostGeom& hg = g->h_geoms[gi];
        if (!hg.n_tris || (visible_only && !g->h_visible[gi]))
            continue;
        any = true;
        for (int q = 0; q < 3; ++q) {
            smin[q] = fminf(smin[q], hg.world_lo[q]);
            smax[q] = fmaxf(smax[q], hg.world_hi[q]);
        }
    }
    for (int q = 0; q < 3; ++q)
        lo[q] = any ? smin[q] : 0.f, hi[q] = any ? smax[q] : 0.f;
}
static void refit_scene_box(GiState* g)
{
    if (g->n_hidden == 0) { // (the fold of every release before hidden geometries existed, its bits kept)
        float smin[3] = {3.4e38f, 3.4e38f, 3.4e38f}, smax[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
        for (const GiState::HostGeom& hg : g->h_geoms)
            if (hg.n_tris)
                for (int q = 0; q < 3; ++q) {
                    smin[q] = fminf(smin[q], hg.world_lo[q]);
                    smax[q] = fmaxf(smax[q], hg.world_hi[q]);
                }
        memcpy(g->scene_min, smin, sizeof(smin));
        memcpy(g->scene_max, smax, sizeof(smax));
        g->nothing_visible = false;
        return;
    }
    gi_fold_scene_box(g, true, g->scene_min, g->scene_max);
    bool any = false;
    for (size_t gi = 0; gi < g->h_geoms.size(); ++gi)
        any = any || (g->h_geoms[gi].n_tris && g->h_visible[gi]);
    g->nothing_visible = !any;
}
// The sun table as after a scene change: the flags in the records are those of the old positions and are ignored from here on (state 2); the hold
// policy of gi_sun_table_update decides when the next table is built -- and looks at the new scene box when it does.
static void refit_drop_sun_table(GiState* g)
{
    if (g->sun_table_state == 0)
        return;
    if (g->sun_table_state == 1)
        g->sun_hold = g->sun_hold_option > 0 ? (uint32_t)g->sun_hold_option : (g->sun_table_age < 32u ? 32u : 2u); // (kSunTableLife, kSunHoldAfterShortLife)
    g->sun_table_state = 2;
    g->sun_table_stale = true;
    g->sun_seen = 0;
}
// the levels of the tree, deepest first, then the 64-byte nodes again
static hipError_t refit_enqueue_levels(GiState* g, uint32_t call, hipStream_t stream)
{
    const uint32_t n_slots = g->view.n_tris;
    for (size_t lv = g->level_first.size(); lv-- > 1;) {
        const uint32_t first = g->level_first[lv - 1], count = g->level_first[lv] - first;
        if (count)
            hipLaunchKernelGGL(refit_level_kernel, dim3((4u * count + 255) / 256), dim3(256), 0, stream, const_cast<Bvh4Node*>(g->view.nodes), first, count,
                               g->n_nodes, g->view.tris, n_slots, g->n_geoms, call, (const uint32_t*)g->d_geom_epoch, g->d_node_epoch,
                               (const uint32_t*)g->d_visible);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    return gi_quantise_nodes(g->view.nodes, g->n_nodes, const_cast<Bvh4NodeQ*>(g->view.qnodes), stream);
}

// ---- what every update call does with the ring and with the end of its chain ----
// The pinned vertex staging holds at least `bytes` per slot; when it has to grow it grows to `want` (>= bytes), rounded up to pages.
// Growing frees the ring: every update that may still read it has to be done first.
hipError_t vstage_reserve(GiState* g, size_t bytes, size_t want)
{
    if (bytes <= g->vstage_cap)
        return hipSuccess;
    for (int q = 0; q < GiState::kStageSlots; ++q)
        if (g->stage_used[q])
            if (hipError_t e = hipEventSynchronize(g->stage_ev[q]); e != hipSuccess)
                return e;
    void* fresh = nullptr;
    const size_t cap = (std::max(bytes, want) + 4095u) & ~(size_t)4095u;
    if (hipError_t e = hipHostMalloc(&fresh, cap * GiState::kStageSlots, hipHostMallocDefault); e != hipSuccess)
        return e;
    if (g->h_vstage)
        (void)hipHostFree(g->h_vstage);
    g->h_vstage = fresh;
    g->vstage_cap = cap;
    return hipSuccess;
}
// the slot of update `call`: its event exists, and the update kStageSlots calls ago has read it (long done unless the host runs that far ahead)
hipError_t stage_slot_acquire(GiState* g, uint32_t call, int* slot)
{
    const int s = (int)(call % (uint32_t)GiState::kStageSlots);
    *slot = s;
    if (!g->stage_ev[s])
        if (hipError_t e = hipEventCreateWithFlags(&g->stage_ev[s], hipEventDisableTiming); e != hipSuccess)
            return e;
    return g->stage_used[s] ? hipEventSynchronize(g->stage_ev[s]) : hipSuccess;
}
// the slot is let go behind what has been enqueued on `stream` so far: the last command that reads the pinned memory
hipError_t stage_slot_release(GiState* g, int slot, hipStream_t stream)
{
    if (hipError_t e = hipEventRecord(g->stage_ev[slot], stream); e != hipSuccess)
        return e;
    g->stage_used[slot] = true;
    return hipSuccess;
}
static hipError_t results_enqueue_boxes(GiState* g, int slot, uint32_t n_entries, hipStream_t stream);
// the triangles of the geometries stamped `call` baked again (hidden ones: emptied), one lane per leaf-order slot
static void refit_enqueue_rebake(GiState* g, uint32_t call, hipStream_t stream)
{
    const uint32_t n_slots = g->view.n_tris;
    hipLaunchKernelGGL(rebake_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, stream, const_cast<float4*>(g->view.tris), n_slots, g->n_geoms, call,
                       (const uint32_t*)g->d_geom_epoch, g->view.geoms, g->view.indices, (const float*)g->d_pos, (const float*)g->d_xf,
                       (const uint32_t*)g->d_visible);
}
// what follows the kernel that stamped the geometries: their triangles baked again, the normal and tangent words of their records where
// these changed, the boxes of the slot's entry list, the levels of the tree, the 64-byte nodes
static hipError_t refit_enqueue_rewrite(GiState* g, int slot, uint32_t call, bool repack, uint32_t n_boxed, hipStream_t stream)
{
    const uint32_t n_slots = g->view.n_tris;
    refit_enqueue_rebake(g, call, stream);
    if (repack)
        hipLaunchKernelGGL(repack_records_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, stream,
                           reinterpret_cast<float*>(const_cast<float4*>(g->view.shade)), g->view.tris, n_slots, g->n_geoms, call,
                           (const uint32_t*)g->d_geom_epoch, g->view.geoms, g->view.indices, g->view.normals, g->view.tangents);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (hipError_t e = results_enqueue_boxes(g, slot, n_boxed, stream); e != hipSuccess)
        return e;
    return refit_enqueue_levels(g, call, stream);
}

// ---- boxes reduced on the device, result records ----
static float refit_unordered(uint32_t k) // the float whose refit_ordered key is k
{
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static size_t result_stride(const GiState* g) { return GiState::kResultHead + (size_t)GiState::kResultEntry * g->n_geoms; }
static uint32_t* result_refusal_word(GiState* g, int slot) { return g->d_result + (size_t)slot * result_stride(g) + 1; }

hipError_t gi_harvest_results(GiState* g, bool block, uint32_t upto)
{
    for (;;) {
        int s = -1;
        for (int q = 0; q < GiState::kStageSlots; ++q)
            if (g->result_rec[q].used && (s < 0 || g->result_rec[q].call < g->result_rec[s].call))
                s = q;
        if (s < 0 || g->result_rec[s].call > upto)
            return hipSuccess;
        GiState::ResultRecord& rec = g->result_rec[s];
        if (block) {
            if (hipError_t e = hipEventSynchronize(g->result_ev[s]); e != hipSuccess)
                return e;
        } else {
            const hipError_t q = hipEventQuery(g->result_ev[s]);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError(); // (an answer, not a failure)
                return hipSuccess;
            }
            if (q != hipSuccess)
                return q;
        }
        const uint32_t* h = g->h_result + (size_t)s * result_stride(g);
        const bool refused = h[1] != 0u;
        if (rec.device_sourced)
            ++(refused ? g->device_updates_refused : g->device_updates_accepted);
        if (!refused) { // (a refused update wrote nothing: every box stays)
            for (size_t e = 0; e < rec.geoms.size(); ++e) {
                GiState::HostGeom& hg = g->h_geoms[rec.geoms[e]];
                const uint32_t* k = h + GiState::kResultHead + GiState::kResultEntry * e;
                for (int q = 0; q < 3; ++q) {
                    hg.obj_lo[q] = refit_unordered(k[q]), hg.obj_hi[q] = refit_unordered(~k[3 + q]);
                    hg.world_lo[q] = refit_unordered(k[6 + q]), hg.world_hi[q] = refit_unordered(~k[9 + q]);
                }
            }
            if (!rec.geoms.empty())
                refit_scene_box(g);
        }
        rec.used = false;
        rec.geoms.clear();
    }
}

// what the first device-reduced update allocates: the device copy of the referenced-vertex lists, the result ring, the entry lists
static hipError_t results_prepare(GiState* g)
{
    if (g->d_result)
        return hipSuccess;
    if (g->n_geoms > 0x7fffffffu) // (geom_box_kernel: at least one block per entry in a one-dimensional grid)
        return hipErrorInvalidValue;
    if (!g->d_ref_spans) {
        std::vector<uint2> spans(g->n_geoms);
        for (uint32_t gi = 0; gi < g->n_geoms; ++gi)
            spans[gi] = make_uint2(g->h_geoms[gi].firstRef, g->h_geoms[gi].n_refs);
        const uint2* d_spans = nullptr;
        const uint32_t* d_refs = nullptr;
        if (hipError_t e = upload(g, spans, &d_spans); e != hipSuccess)
            return e;
        g->d_ref_spans = const_cast<uint2*>(d_spans);
        if (hipError_t e = upload(g, g->h_ref_verts, &d_refs); e != hipSuccess)
            return e;
        g->d_ref_verts = const_cast<uint32_t*>(d_refs);
    }
    const size_t bytes = GiState::kStageSlots * result_stride(g) * sizeof(uint32_t);
    if (!g->h_result)
        if (hipError_t e = hipHostMalloc((void**)&g->h_result, bytes, hipHostMallocDefault); e != hipSuccess)
            return e;
    if (!g->h_box_list)
        if (hipError_t e = hipHostMalloc((void**)&g->h_box_list, (size_t)GiState::kStageSlots * g->n_geoms * sizeof(uint32_t), hipHostMallocDefault); e != hipSuccess)
            return e;
    void* d = nullptr;
    if (hipError_t e = hipMalloc(&d, bytes); e != hipSuccess)
        return e;
    g->allocs.push_back(d);
    g->d_result = (uint32_t*)d;
    return hipSuccess;
}
// the slot's record of kStageSlots calls ago is applied before the slot is written again (long done unless the host runs that far ahead)
static hipError_t results_acquire(GiState* g, int slot)
{
    if (!g->result_ev[slot])
        if (hipError_t e = hipEventCreateWithFlags(&g->result_ev[slot], hipEventDisableTiming); e != hipSuccess)
            return e;
    return g->result_rec[slot].used ? gi_harvest_results(g, true, g->result_rec[slot].call) : hipSuccess;
}
static hipError_t results_enqueue_init(GiState* g, int slot, uint32_t call, uint32_t n_entries, hipStream_t stream)
{
    const uint32_t words = GiState::kResultHead + GiState::kResultEntry * n_entries;
    hipLaunchKernelGGL(result_init_kernel, dim3((words + 255) / 256), dim3(256), 0, stream, g->d_result + (size_t)slot * result_stride(g), call, n_entries);
    return hipGetLastError();
}
// geom_box_kernel over the slot's entry list (entry e = geometry h_box_list[slot][e]), about eight vertices per lane
static hipError_t results_enqueue_boxes(GiState* g, int slot, uint32_t n_entries, hipStream_t stream)
{
    if (!n_entries)
        return hipSuccess;
    const uint32_t* list = g->h_box_list + (size_t)slot * g->n_geoms;
    uint32_t most = 1;
    for (uint32_t e = 0; e < n_entries; ++e)
        most = std::max(most, g->h_geoms[list[e]].n_refs);
    // blocks per entry, by the largest geometry (the blocks of a smaller one leave on the ballot); fewer where the grid would pass 2^31 - 1
    // blocks: the lanes stride, any count from 1 up covers every vertex (n_entries <= n_geoms < 2^31: results_prepare)
    const uint32_t per_entry = std::max(1u, std::min((most + 2047u) / 2048u, 0x7fffffffu / n_entries));
    hipLaunchKernelGGL(geom_box_kernel, dim3(per_entry * n_entries), dim3(256), 0, stream, list, n_entries, g->n_geoms, (const uint2*)g->d_ref_spans,
                       (const uint32_t*)g->d_ref_verts, (uint32_t)g->h_ref_verts.size(), g->view.geoms, (const float*)g->d_pos, (uint32_t)(g->h_pos.size() / 3),
                       (const float*)g->d_xf, g->d_result + (size_t)slot * result_stride(g) + GiState::kResultHead, per_entry);
    return hipGetLastError();
}
// the end of the chain: the record comes back to the pinned slot, the event says when
static hipError_t results_enqueue_readback(GiState* g, int slot, uint32_t call, bool device_sourced, hipStream_t stream)
{
    GiState::ResultRecord& rec = g->result_rec[slot];
    const size_t words = GiState::kResultHead + GiState::kResultEntry * rec.geoms.size();
    if (hipError_t e = hipMemcpyAsync(g->h_result + (size_t)slot * result_stride(g), g->d_result + (size_t)slot * result_stride(g), words * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, stream);
        e != hipSuccess)
        return e;
    rec.used = true, rec.device_sourced = device_sourced, rec.call = call;
    return hipEventRecord(g->result_ev[slot], stream);
}

// A source of neb_gi_update_vertices_device: `bytes` from p must be memory this context's device reads at the very address p --
// device memory of this device (and then inside its allocation), managed memory, or pinned host memory mapped at its own address.
bool device_readable(const neb_ctx* ctx, const void* p, size_t bytes)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // (how the runtime answers for plain host memory)
        return false;
    }
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != ctx->device)
            return false;
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void*>(p)) != hipSuccess) {
            (void)hipGetLastError();
            return false; // (no allocation to check the range against: refused rather than trusted)
        }
        return (uintptr_t)p + bytes <= (uintptr_t)base + size;
    }
    if (at.type == hipMemoryTypeManaged)
        return true;
    return at.type == hipMemoryTypeHost && at.devicePointer == p;
}

// order: behind the last rewrite, and behind every stream that may still be reading what is about to be rewritten
int refit_order_behind_readers(neb_ctx* ctx, GiState* g, hipStream_t stream)
{
    GI_HIP(ctx, gi_sun_table_order(g, stream));
    if (g->reader_overflow) {
        GI_HIP(ctx, hipDeviceSynchronize());
    } else {
        for (int k = 0; k < g->n_reader_streams; ++k) {
            if (g->reader_streams[k] == stream)
                continue;
            if (!g->reader_ev[k])
                GI_HIP(ctx, hipEventCreateWithFlags(&g->reader_ev[k], hipEventDisableTiming));
            GI_HIP(ctx, hipEventRecord(g->reader_ev[k], g->reader_streams[k]));
            GI_HIP(ctx, hipStreamWaitEvent(stream, g->reader_ev[k], 0));
        }
    }
    g->n_reader_streams = 0;
    g->reader_overflow = false;
    return NEB_OK;
}

// ---- option svgf_vertex_motion: previous pools, dirty spans, the roll ----
// an update call names vertices [first, first + count) of geometry gi: the union per geometry is what the next roll copies
static void roll_mark(GiState* g, uint32_t gi, uint32_t first, uint32_t count)
{
    if (!g->d_pos_prev || !count)
        return;
    uint2& sp = g->roll_span[gi];
    if (sp.x >= sp.y)
        sp = make_uint2(first, first + count);
    else
        sp = make_uint2(std::min(sp.x, first), std::max(sp.y, first + count));
    g->roll_pending = true;
}

void gi_vertex_motion_free(neb_ctx* ctx)
{
    GiState* g = ctx->gi;
    if (!g)
        return;
    for (void* p : {(void*)g->d_pos_prev, (void*)g->d_nrm_prev, (void*)g->d_deform_dirty})
        if (p)
            (void)hipFree(p);
    g->d_pos_prev = g->d_nrm_prev = nullptr;
    g->d_deform_dirty = nullptr;
    g->roll_span.clear();
    g->roll_pending = false;
}

int gi_vertex_motion_alloc(neb_ctx* ctx)
{
    gi_vertex_motion_free(ctx);
    GiState* g = ctx->gi;
    if (!g || !g->n_geoms || !g->d_pos || !g->view.normals || !g->h_stage || g->h_pos.empty())
        return NEB_OK; // no scene: nothing can deform
    GI_GUARD(ctx);
    const size_t bytes = g->h_pos.size() * sizeof(float); // (the normal pool holds three floats per vertex as well)
    hipError_t e = hipDeviceSynchronize(); // (an update still in flight would be copied half done)
    if (e == hipSuccess)
        e = hipMalloc((void**)&g->d_pos_prev, bytes);
    if (e == hipSuccess)
        e = hipMalloc((void**)&g->d_nrm_prev, bytes);
    if (e == hipSuccess)
        e = hipMalloc((void**)&g->d_deform_dirty, (size_t)g->n_geoms * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(g->d_pos_prev, g->d_pos, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(g->d_nrm_prev, g->view.normals, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess)
        e = hipMemset(g->d_deform_dirty, 0, (size_t)g->n_geoms * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        gi_vertex_motion_free(ctx);
        return gi_fail(ctx, NEB_ERR_HIP, "svgf_vertex_motion: previous vertex pools", e);
    }
    g->roll_span.assign(g->n_geoms, make_uint2(0u, 0u));
    return NEB_OK;
}

// The spans travel in the ring of pinned argument slots (h_stage, stage_ev): the slot two calls ahead of the last update's, the one
// furthest from the slots the updates around this roll use, under the ring's own rule -- whoever writes a slot waits for the event of
// its last user first (long passed unless the host runs a whole ring ahead).  Enqueue only, nothing allocated.
int gi_roll_vertices(neb_ctx* ctx, hipStream_t stream)
{
    GiState* g = ctx->gi;
    if (!g || !g->d_pos_prev || !g->roll_pending)
        return NEB_OK;
    GI_GUARD(ctx);
    static_assert(sizeof(GiState::RollSpan) <= sizeof(GiState::StageEntry), "a slot of h_stage holds one span per geometry");
    const int slot = (int)((g->epoch + 2u) % (uint32_t)GiState::kStageSlots);
    if (!g->stage_ev[slot])
        GI_HIP(ctx, hipEventCreateWithFlags(&g->stage_ev[slot], hipEventDisableTiming));
    if (g->stage_used[slot])
        GI_HIP(ctx, hipEventSynchronize(g->stage_ev[slot]));
    GI_HIP(ctx, gi_scene_reader(g, stream)); // an update enqueued on another stream comes first; a later one waits for this roll
    GiState::RollSpan* spans = reinterpret_cast<GiState::RollSpan*>(g->h_stage + (size_t)slot * g->n_geoms);
    const uint32_t n_pool = (uint32_t)(g->h_pos.size() / 3);
    uint32_t n_spans = 0, lane = 0;
    for (uint32_t gi = 0; gi < g->n_geoms; ++gi) {
        uint2& sp = g->roll_span[gi];
        if (sp.x < sp.y) {
            spans[n_spans++] = {lane, sp.y - sp.x, g->h_geoms[gi].vertexBase + sp.x, gi};
            lane += sp.y - sp.x;
        }
        sp = make_uint2(0u, 0u);
    }
    g->roll_pending = false;
    if (!lane)
        return NEB_OK;
    hipLaunchKernelGGL(deform_roll_kernel, dim3((lane + 255) / 256), dim3(256), 0, stream, (const GiState::RollSpan*)spans, n_spans, lane, n_pool,
                       g->n_geoms, (const float*)g->d_pos, g->view.normals, g->d_pos_prev, g->d_nrm_prev, g->d_deform_dirty);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, slot, stream));
    return NEB_OK;
}

// The fresh tree of neb_gi_build_bvh holds every triangle at its real position -- its topology does not depend on the flags, so showing
// never needs a rebuild --; the hidden geometries leave it here: stamped, their slots emptied, the levels refitted, the 64-byte nodes
// quantised again.  One more update in the count of epochs; no argument slot (the flags are on the device already).
hipError_t gi_visibility_after_build(GiState* g, hipStream_t stream)
{
    if (!g->n_hidden || !g->n_geoms || !g->view.n_tris)
        return hipSuccess;
    const uint32_t call = ++g->epoch;
    hipLaunchKernelGGL(visibility_stamp_kernel, dim3((g->n_geoms + 63) / 64), dim3(64), 0, stream, g->n_geoms, call, (const uint32_t*)g->d_visible,
                       g->d_geom_epoch);
    refit_enqueue_rebake(g, call, stream);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    return refit_enqueue_levels(g, call, stream);
}

// ---- what the update calls share on the host: refusals ----
static int fail_who(neb_ctx* ctx, int code, const char* who, const char* what, hipError_t e = hipSuccess)
{
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return gi_fail(ctx, code, msg, e);
}
// One entry of a call's geometry list: the index is in range (range_code where it is not) and the call has not named it before.
// stamp = ++g->seen_stamp, one per call, accepted or not: h_seen needs no clearing.
static int geometry_named_once(neb_ctx* ctx, GiState* g, uint32_t stamp, uint32_t gi, const char* who, int range_code)
{
    if (gi >= g->n_geoms)
        return fail_who(ctx, range_code, who, "geometry index out of range");
    if (g->h_seen[gi] == stamp)
        return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "a geometry is named twice");
    g->h_seen[gi] = stamp;
    return NEB_OK;
}
// columns 0-2 of every joint matrix of a palette are finite (column 3 is never read: skin_blend)
static bool palette_finite(const float* m, uint32_t n_joints)
{
    for (uint32_t q = 0; q < 16u * n_joints; ++q)
        if ((q & 3u) != 3u && !std::isfinite(m[q]))
            return false;
    return true;
}
// What neb_gi_update_vertices and neb_gi_update_vertices_device (device_sources: pointers and strides are multiples of 4, the lanes
// load floats) check of their entries before anything changes.  The ranges that are not empty come back sorted by {geometry, first
// vertex}, with the numbers of vertices in all of them, and in those that carry normals and tangents.
struct VertexSpan { uint32_t geom, first, count, k; };
static int collect_vertex_spans(neb_ctx* ctx, const GiState* g, const neb_vertex_update* updates, uint32_t n, const char* who, bool device_sources,
                                std::vector<VertexSpan>& spans, size_t& n_lanes, size_t& n_nrm, size_t& n_tan)
{
    spans.reserve(n);
    n_lanes = n_nrm = n_tan = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_vertex_update& u = updates[k];
        if (!u.positions)
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "null positions");
        if (u.geometry >= g->n_geoms)
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "geometry index out of range");
        const GiState::HostGeom& hg = g->h_geoms[u.geometry];
        if ((uint64_t)u.firstVertex + u.numVertices > hg.n_verts)
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "vertex range beyond the geometry's numVertices");
        if ((u.normals || u.tangents) && !hg.valid)
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "normals or tangents for a geometry that was set without its attribute streams");
        if (u.positionStride < 12u || (u.normals && u.normalStride < 12u) || (u.tangents && u.tangentStride < 16u))
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "a stride is smaller than its element");
        if (device_sources && ((((uintptr_t)u.positions | u.positionStride) & 3u) || (u.normals && (((uintptr_t)u.normals | u.normalStride) & 3u)) ||
                               (u.tangents && (((uintptr_t)u.tangents | u.tangentStride) & 3u))))
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "a pointer or a stride is not a multiple of 4");
        if (u.numVertices == 0)
            continue;
        spans.push_back({u.geometry, u.firstVertex, u.numVertices, k});
        n_lanes += u.numVertices;
        n_nrm += u.normals ? u.numVertices : 0u;
        n_tan += u.tangents ? u.numVertices : 0u;
    }
    std::sort(spans.begin(), spans.end(), [](const VertexSpan& a, const VertexSpan& b) { return a.geom != b.geom ? a.geom < b.geom : a.first < b.first; });
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].geom == spans[i - 1].geom && (uint64_t)spans[i - 1].first + spans[i - 1].count > spans[i].first)
            return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "two ranges of one geometry overlap");
    if (n_lanes > 0xffffffffull / 10u) // (lanes are 32-bit, and so are the offsets into the slot, in floats: at most 10 floats per vertex)
        return fail_who(ctx, NEB_ERR_INVALID_ARG, who, "too many vertices in one call");
    return NEB_OK;
}

// ---- what the update calls share on the host: the chain ----
// One accepted call from its ring slot to the end of its chain.  device_sourced: the new vertices never pass the host (neb_gi_update_
// vertices_device, neb_gi_skin_vertices, neb_gi_morph_vertices) -- h_pos of every touched geometry goes stale, and the call always has
// a result record, which counts in neb_gi_update_status.  Every other call has one where it touches a geometry whose h_pos is stale.
struct UpdateCall {
    neb_ctx* ctx;
    GiState* g;
    hipStream_t stream;
    bool device_sourced;
    uint32_t call = 0;      // the epoch of this update
    int slot = 0;           // its slot in the rings (arguments, entry lists, result records)
    bool may_record = false; // update_begin made the slot's result record ready
    bool any_tris = false;  // a touched geometry has triangles: the chain rewrites them
    GiState::ResultRecord& rec() const { return g->result_rec[slot]; }
    uint32_t n_boxed() const { return may_record ? (uint32_t)rec().geoms.size() : 0u; }
    bool has_record() const { return device_sourced || n_boxed() != 0u; }
};
// The slot of the call, its result record where the call may need one (the record of kStageSlots calls ago is applied first), the
// stream ordered behind every reader -- and then, nothing being able to fail any more, the epoch: the call counts.
static int update_begin(UpdateCall& uc, bool may_record)
{
    GiState* g = uc.g;
    uc.call = g->epoch + 1u;
    uc.may_record = may_record;
    GI_HIP(uc.ctx, stage_slot_acquire(g, uc.call, &uc.slot));
    if (may_record) {
        GI_HIP(uc.ctx, results_acquire(g, uc.slot));
        uc.rec().geoms.clear();
    }
    if (int rc = refit_order_behind_readers(uc.ctx, g, uc.stream); rc != NEB_OK)
        return rc;
    g->epoch = uc.call;
    return NEB_OK;
}
// The call changes geometry gi: h_tris holds an earlier bake of its triangles from here on, and where h_pos does not hold its vertices the
// geometry joins the slot's entry list (geom_box_kernel) and the result record that brings its boxes back -- once: a caller that
// names a geometry several times names it in a row.
static void update_touch(UpdateCall& uc, uint32_t gi)
{
    GiState* g = uc.g;
    GiState::HostGeom& hg = g->h_geoms[gi];
    if (uc.device_sourced)
        hg.host_stale = true;
    if (!hg.n_tris)
        return;
    hg.dirty = true;
    uc.any_tris = true;
    std::vector<uint32_t>& listed = uc.rec().geoms;
    if (!hg.host_stale || (!listed.empty() && listed.back() == gi))
        return;
    g->h_box_list[(size_t)uc.slot * g->n_geoms + listed.size()] = gi;
    listed.push_back(gi);
}
// first in the chain wherever there is a record: its head and the neutral boxes of its entries
static hipError_t update_record_init(const UpdateCall& uc)
{
    return uc.has_record() ? results_enqueue_init(uc.g, uc.slot, uc.call, uc.n_boxed(), uc.stream) : hipSuccess;
}
// The end of every chain, behind the kernel that stamped the geometries: the rewrite where a touched geometry has triangles, the
// record on its way back where there is one, the rewrite marked for the readers on other streams.
static int update_finish(UpdateCall& uc, bool repack)
{
    GiState* g = uc.g;
    if (uc.any_tris && g->view.n_tris)
        GI_HIP(uc.ctx, refit_enqueue_rewrite(g, uc.slot, uc.call, repack, uc.n_boxed(), uc.stream));
    if (uc.has_record())
        GI_HIP(uc.ctx, results_enqueue_readback(g, uc.slot, uc.call, uc.device_sourced, uc.stream));
    GI_HIP(uc.ctx, mark_rewrite(g, uc.stream));
    return NEB_OK;
}

// The second half of neb_gi_set_skin and neb_gi_set_morph_targets, behind their checks.  What the call needs is allocated before anything
// is let go of: a fresh block of block_bytes[k] for entry k (0: the entry removes), and a fresh argument buffer where the capacity changes.
// Everything that can still fail fills the FRESH blocks -- fill(k, block) -- behind a rewrite enqueued on another stream (gi_scene_reader;
// a later rewrite waits for the copies).  A failure frees them and nothing of the context has changed; success commits the argument
// buffer and hands the blocks over in `fresh` for the caller to bind (rebind_block): from there on nothing can fail.
template <typename Fill>
static int setup_fresh_blocks(neb_ctx* ctx, GiState* g, hipStream_t stream, const char* who, const std::vector<size_t>& block_bytes, size_t args_cap,
                              std::vector<void*>& fresh, Fill fill)
{
    const size_t n = block_bytes.size();
    fresh.assign(n, nullptr);
    void* fresh_args = nullptr;
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < n && e == hipSuccess; ++k)
        if (block_bytes[k])
            e = hipMalloc(&fresh[k], block_bytes[k]);
    if (e == hipSuccess && args_cap && args_cap != g->skin_args_cap)
        e = hipMalloc(&fresh_args, args_cap);
    if (e == hipSuccess)
        e = hipDeviceSynchronize(); // (a set-up call: a call still in flight reads the blocks and the argument buffer about to be replaced)
    if (e == hipSuccess)
        e = gi_scene_reader(g, stream);
    for (size_t k = 0; k < n && e == hipSuccess; ++k)
        if (fresh[k])
            e = fill((uint32_t)k, (uint8_t*)fresh[k]);
    if (e != hipSuccess) {
        for (void* p : fresh)
            if (p)
                (void)hipFree(p); // (waits for the device: a copy into the block that was enqueued is done)
        if (fresh_args)
            (void)hipFree(fresh_args);
        return fail_who(ctx, NEB_ERR_HIP, who, "device memory", e);
    }
    if (args_cap != g->skin_args_cap) {
        if (g->d_skin_args)
            (void)hipFree(g->d_skin_args);
        g->d_skin_args = fresh_args;
        g->skin_args_cap = args_cap;
    }
    return NEB_OK;
}
// the geometry's old block is freed and its entry (GiState::Skin / Morph) starts again with the fresh one (null: unbound)
template <typename Bound>
static Bound& rebind_block(std::vector<Bound>& bound, uint32_t gi, void* fresh)
{
    Bound& b = bound[gi];
    if (b.d_block)
        (void)hipFree(b.d_block);
    b = Bound();
    b.d_block = fresh;
    return b;
}

} // namespace neb

using namespace neb;

extern "C" {

int neb_gi_set_visibility(neb_ctx* ctx, const uint32_t* geometry_indices, const uint8_t* visible, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_set_visibility: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!geometry_indices || !visible)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_visibility: null pointer");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t stamp = ++g->seen_stamp;
    for (uint32_t k = 0; k < n; ++k)
        if (int rc = geometry_named_once(ctx, g, stamp, geometry_indices[k], "neb_gi_set_visibility", NEB_ERR_OUT_OF_RANGE); rc != NEB_OK)
            return rc;
    uint32_t n_changed = 0; // (n <= n_geoms from here on: every index is in range and none is named twice)
    for (uint32_t k = 0; k < n; ++k)
        n_changed += (g->h_visible[geometry_indices[k]] != 0) != (visible[k] != 0) ? 1u : 0u;
    if (n_changed == 0)
        return NEB_OK; // every geometry is in the state asked for: nothing is enqueued, the sun table stays
    GI_GUARD(ctx);
    UpdateCall uc{ctx, g, (hipStream_t)stream_, false};
    if (int rc = update_begin(uc, false); rc != NEB_OK)
        return rc;
    // ---- commit the host side; the argument slot is pinned host memory the first kernel reads ----
    GiState::StageEntry* st = g->h_stage + (size_t)uc.slot * g->n_geoms;
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gi = geometry_indices[k];
        const uint8_t v = visible[k] ? 1 : 0;
        if (g->h_visible[gi] == v)
            continue;
        g->h_visible[gi] = v;
        g->n_hidden += v ? (uint32_t)-1 : 1u;
        memset(&st[ns], 0, sizeof(st[ns]));
        st[ns].geom = gi;
        st[ns].pad[0] = v;
        ++ns;
        uc.any_tris = uc.any_tris || g->h_geoms[gi].n_tris != 0; // (no update_touch: the vertices and h_tris stay what they are)
    }
    refit_scene_box(g);
    refit_drop_sun_table(g);
    // ---- enqueue ----
    hipLaunchKernelGGL(visibility_apply_kernel, dim3((ns + 63) / 64), dim3(64), 0, uc.stream, (const GiState::StageEntry*)st, ns, g->n_geoms, uc.call,
                       g->d_visible, g->d_geom_epoch);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream));
    return update_finish(uc, false);
}

int neb_gi_get_visibility(const neb_ctx* ctx, uint8_t* out, uint32_t capacity, uint32_t* n_out)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    const GiState* g = ctx->gi;
    if (!g)
        return NEB_ERR_STATE;
    if (n_out)
        *n_out = g->n_geoms;
    if (capacity && !out)
        return NEB_ERR_INVALID_ARG;
    for (uint32_t gi = 0; gi < g->n_geoms && gi < capacity; ++gi)
        out[gi] = g->h_visible[gi];
    return NEB_OK;
}

int neb_gi_update_transforms(neb_ctx* ctx, const uint32_t* geometry_indices, const float* surfaceToWorld, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_transforms: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!geometry_indices || !surfaceToWorld)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_transforms: null pointer");
    if (n > g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_transforms: more entries than geometries (an index is out of range or named twice)");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t stamp = ++g->seen_stamp;
    for (uint32_t k = 0; k < n; ++k)
        if (int rc = geometry_named_once(ctx, g, stamp, geometry_indices[k], "neb_gi_update_transforms", NEB_ERR_INVALID_ARG); rc != NEB_OK)
            return rc;
    // A geometry whose h_pos is stale (neb_gi_update_vertices_device) is checked by the corners of its object-space box alone -- current
    // once every record has been harvested -- and takes its world box from geom_box_kernel and a result record, not from a host walk.
    bool any_stale = false;
    for (uint32_t k = 0; k < n; ++k)
        any_stale = any_stale || g->h_geoms[geometry_indices[k]].host_stale;
    if (any_stale) {
        neb::DeviceGuard guard(ctx->device);
        if (guard.err != hipSuccess)
            return gi_fail(ctx, NEB_ERR_HIP, "hipSetDevice", guard.err);
        GI_HIP(ctx, gi_harvest_results(g, true));
        GI_HIP(ctx, results_prepare(g));
    }
    struct Box { float lo[3], hi[3]; };
    std::vector<Box> boxes(n);
    std::vector<char> changed(n, 0);
    uint32_t n_changed = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const GiState::HostGeom& hg = g->h_geoms[geometry_indices[k]];
        const float* m = surfaceToWorld + 16 * (size_t)k;
        for (int q = 0; q < 16; ++q)
            if (!(fabsf(m[q]) <= 3.0e38f))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_transforms: a matrix entry is not a finite number");
        if (hg.n_tris) { // the corners of the object-space box kept at neb_gi_set_scene, under the new transform
            for (int corner = 0; corner < 8; ++corner) {
                const float a[3] = {(corner & 1) ? hg.obj_hi[0] : hg.obj_lo[0], (corner & 2) ? hg.obj_hi[1] : hg.obj_lo[1], (corner & 4) ? hg.obj_hi[2] : hg.obj_lo[2]};
                float w[3];
                if (!gi_bake_point(m, a, w))
                    return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_transforms: the transform moves a submesh to a position that is not finite");
            }
        }
        changed[k] = memcmp(m, hg.m, 64) != 0;
        n_changed += changed[k] ? 1u : 0u;
    }
    if (n_changed == 0)
        return NEB_OK; // every matrix is the one already set: nothing moves, nothing is enqueued, the sun table stays
    // the exact world-space box of every moved geometry: its referenced vertices in the bake's own arithmetic
    for (uint32_t k = 0; k < n; ++k) {
        if (!changed[k] || g->h_geoms[geometry_indices[k]].host_stale)
            continue;
        const GiState::HostGeom& hg = g->h_geoms[geometry_indices[k]];
        const float* m = surfaceToWorld + 16 * (size_t)k;
        Box& b = boxes[k];
        for (int q = 0; q < 3; ++q)
            b.lo[q] = 3.4e38f, b.hi[q] = -3.4e38f;
        for (uint32_t r = 0; r < hg.n_refs; ++r) {
            float w[3];
            if (!gi_bake_point(m, &g->h_pos[3 * (size_t)(hg.vertexBase + g->h_ref_verts[hg.firstRef + r])], w))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_transforms: the transform moves a vertex to a position that is not finite");
            for (int q = 0; q < 3; ++q) {
                b.lo[q] = fminf(b.lo[q], w[q]);
                b.hi[q] = fmaxf(b.hi[q], w[q]);
            }
        }
    }
    GI_GUARD(ctx);
    UpdateCall uc{ctx, g, (hipStream_t)stream_, false};
    if (int rc = update_begin(uc, any_stale); rc != NEB_OK)
        return rc;
    // ---- commit the host side; the argument slot is pinned host memory the first kernel reads ----
    GiState::StageEntry* st = g->h_stage + (size_t)uc.slot * g->n_geoms;
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (!changed[k])
            continue;
        const uint32_t gi = geometry_indices[k];
        GiState::HostGeom& hg = g->h_geoms[gi];
        memcpy(hg.m, surfaceToWorld + 16 * (size_t)k, 64);
        st[ns].geom = gi;
        st[ns].pad[0] = st[ns].pad[1] = st[ns].pad[2] = 0;
        memcpy(st[ns].m, hg.m, 64);
        ++ns;
        update_touch(uc, gi); // (the stale geometries among the moved ones become entries of this call's result record)
        if (hg.n_tris && !hg.host_stale) {
            memcpy(hg.world_lo, boxes[k].lo, 12);
            memcpy(hg.world_hi, boxes[k].hi, 12);
        }
    }
    if (uc.any_tris) {
        refit_scene_box(g);
        refit_drop_sun_table(g);
    }
    // ---- enqueue ----
    GI_HIP(ctx, update_record_init(uc));
    hipLaunchKernelGGL(refit_apply_kernel, dim3((ns + 63) / 64), dim3(64), 0, uc.stream, (const GiState::StageEntry*)st, ns, g->n_geoms, uc.call, g->d_xf,
                       const_cast<DevGeom*>(g->view.geoms), const_cast<ShadeHeader*>(g->shade_heads), g->d_geom_epoch);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream));
    return update_finish(uc, false);
}

int neb_gi_update_vertices(neb_ctx* ctx, const neb_vertex_update* updates, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_update_vertices";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_vertices: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_vertices: null pointer");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything that can refuse the call comes before anything changes ----
    std::vector<VertexSpan> spans;
    size_t n_lanes, n_nrm, n_tan;
    if (int rc = collect_vertex_spans(ctx, g, updates, n, who, false, spans, n_lanes, n_nrm, n_tan); rc != NEB_OK)
        return rc;
    for (const VertexSpan& sp : spans) {
        const neb_vertex_update& u = updates[sp.k];
        const float* m = g->h_geoms[sp.geom].m;
        for (uint32_t j = 0; j < sp.count; ++j) {
            float a[3], w[3];
            memcpy(a, (const uint8_t*)u.positions + (size_t)j * u.positionStride, 12);
            if (!(fabsf(a[0]) <= 3.0e38f && fabsf(a[1]) <= 3.0e38f && fabsf(a[2]) <= 3.0e38f))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_vertices: a position is not a finite number");
            if (!gi_bake_point(m, a, w))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_vertices: a position (after the instance transform) is not a finite number");
        }
    }
    if (spans.empty())
        return NEB_OK; // every range is empty: nothing moves, nothing is enqueued, the sun table stays
    GI_GUARD(ctx);
    // a touched geometry whose h_pos is stale (neb_gi_update_vertices_device): its boxes come from geom_box_kernel and a result record
    bool any_boxed = false;
    for (const VertexSpan& sp : spans)
        any_boxed = any_boxed || (g->h_geoms[sp.geom].host_stale && g->h_geoms[sp.geom].n_tris);
    if (any_boxed)
        GI_HIP(ctx, results_prepare(g));
    // ---- the staging slot: pinned host memory, {ranges | positions | normals | tangents}, grown to the largest update seen ----
    const size_t head = (spans.size() * sizeof(GiState::DeformRange) + 15u) & ~(size_t)15u;
    const size_t bytes = head + 4u * (3u * n_lanes + 3u * n_nrm + 4u * n_tan);
    GI_HIP(ctx, vstage_reserve(g, bytes, bytes));
    if (g->deform_stage == 1 && g->vstage_cap > g->d_vstage_cap) {
        void* fresh = nullptr;
        GI_HIP(ctx, hipMalloc(&fresh, g->vstage_cap));
        if (g->d_vstage)
            (void)hipFree(g->d_vstage); // (waits for the device: the update that read it is done)
        g->d_vstage = fresh;
        g->d_vstage_cap = g->vstage_cap;
    }
    UpdateCall uc{ctx, g, (hipStream_t)stream_, false};
    if (int rc = update_begin(uc, any_boxed); rc != NEB_OK)
        return rc;
    // ---- commit the host side: the slot, h_pos, the boxes ----
    uint8_t* base = (uint8_t*)g->h_vstage + (size_t)uc.slot * g->vstage_cap;
    GiState::DeformRange* ranges = (GiState::DeformRange*)base;
    float* data = (float*)(base + head);
    uint32_t lane = 0, off_p = 0, off_n = (uint32_t)(3u * n_lanes), off_t = (uint32_t)(3u * n_lanes + 3u * n_nrm);
    bool any_attr = false;
    for (size_t i = 0; i < spans.size(); ++i) {
        const VertexSpan& sp = spans[i];
        const neb_vertex_update& u = updates[sp.k];
        GiState::HostGeom& hg = g->h_geoms[sp.geom];
        GiState::DeformRange& r = ranges[i];
        r.first_lane = lane, r.count = sp.count, r.dst = hg.vertexBase + sp.first, r.geom = sp.geom, r.pad = 0;
        roll_mark(g, sp.geom, sp.first, sp.count);
        r.pos_off = off_p;
        r.nrm_off = u.normals ? off_n : GiState::kNoStream;
        r.tan_off = u.tangents ? off_t : GiState::kNoStream;
        float* hp = &g->h_pos[3 * (size_t)r.dst];
        for (uint32_t j = 0; j < sp.count; ++j) {
            memcpy(data + off_p + 3 * (size_t)j, (const uint8_t*)u.positions + (size_t)j * u.positionStride, 12);
            memcpy(hp + 3 * (size_t)j, data + off_p + 3 * (size_t)j, 12);
        }
        if (u.normals)
            for (uint32_t j = 0; j < sp.count; ++j)
                memcpy(data + off_n + 3 * (size_t)j, (const uint8_t*)u.normals + (size_t)j * u.normalStride, 12);
        if (u.tangents)
            for (uint32_t j = 0; j < sp.count; ++j)
                memcpy(data + off_t + 4 * (size_t)j, (const uint8_t*)u.tangents + (size_t)j * u.tangentStride, 16);
        lane += sp.count, off_p += 3u * sp.count;
        off_n += u.normals ? 3u * sp.count : 0u;
        off_t += u.tangents ? 4u * sp.count : 0u;
        any_attr = any_attr || u.normals || u.tangents;
        update_touch(uc, sp.geom);
    }
    // the boxes of every touched geometry over its referenced vertices: object space, and world space in the bake's own arithmetic
    for (size_t i = 0; i < spans.size(); ++i) {
        if (i && spans[i].geom == spans[i - 1].geom)
            continue;
        GiState::HostGeom& hg = g->h_geoms[spans[i].geom];
        if (!hg.n_tris || hg.host_stale)
            continue;
        for (int q = 0; q < 3; ++q) {
            hg.obj_lo[q] = hg.world_lo[q] = 3.4e38f;
            hg.obj_hi[q] = hg.world_hi[q] = -3.4e38f;
        }
        for (uint32_t r = 0; r < hg.n_refs; ++r) {
            const float* a = &g->h_pos[3 * (size_t)(hg.vertexBase + g->h_ref_verts[hg.firstRef + r])];
            float w[3];
            (void)gi_bake_point(hg.m, a, w); // (checked finite above, or when the position / the matrix was accepted)
            for (int q = 0; q < 3; ++q) {
                hg.obj_lo[q] = fminf(hg.obj_lo[q], a[q]);
                hg.obj_hi[q] = fmaxf(hg.obj_hi[q], a[q]);
                hg.world_lo[q] = fminf(hg.world_lo[q], w[q]);
                hg.world_hi[q] = fmaxf(hg.world_hi[q], w[q]);
            }
        }
    }
    if (uc.any_tris) {
        refit_scene_box(g);
        refit_drop_sun_table(g);
    }
    // ---- enqueue ----
    const uint32_t n_ranges = (uint32_t)spans.size(), n_pool = (uint32_t)(g->h_pos.size() / 3);
    const uint8_t* src = base;
    GI_HIP(ctx, update_record_init(uc));
    if (g->deform_stage == 1) {
        GI_HIP(ctx, hipMemcpyAsync(g->d_vstage, base, bytes, hipMemcpyHostToDevice, uc.stream));
        src = (const uint8_t*)g->d_vstage;
    }
    hipLaunchKernelGGL(deform_scatter_kernel<false>, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)src, n_ranges,
                       (const float*)(src + head), lane, n_pool, g->n_geoms, uc.call, g->d_pos, const_cast<float*>(g->view.normals),
                       const_cast<float*>(g->view.tangents), g->d_geom_epoch, (const GiState::DeformSource*)nullptr, (const uint32_t*)nullptr,
                       g->d_deform_dirty);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream));
    return update_finish(uc, any_attr);
}

int neb_gi_update_vertices_device(neb_ctx* ctx, const neb_vertex_update* updates, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_update_vertices_device";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_vertices_device: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_vertices_device: null pointer");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything the HOST can refuse the call for comes before anything changes (the vertices themselves: deform_check_kernel) ----
    std::vector<VertexSpan> spans;
    size_t n_lanes, n_nrm, n_tan;
    if (int rc = collect_vertex_spans(ctx, g, updates, n, who, true, spans, n_lanes, n_nrm, n_tan); rc != NEB_OK)
        return rc;
    if (spans.empty())
        return NEB_OK; // every range is empty: nothing moves, nothing is enqueued, the sun table stays
    GI_GUARD(ctx);
    for (const VertexSpan& sp : spans) { // a host pointer handed in by mistake would fault the device: every source is looked up first
        const neb_vertex_update& u = updates[sp.k];
        const size_t last = (size_t)sp.count - 1u;
        if (!device_readable(ctx, u.positions, last * u.positionStride + 12u) || (u.normals && !device_readable(ctx, u.normals, last * u.normalStride + 12u)) ||
            (u.tangents && !device_readable(ctx, u.tangents, last * u.tangentStride + 16u)))
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_vertices_device: a source is not memory this context's device can read (or the range leaves its allocation)");
    }
    GI_HIP(ctx, results_prepare(g));
    // ---- the staging slot: pinned host memory, here {ranges | sources} only ----
    const size_t head = (spans.size() * sizeof(GiState::DeformRange) + 15u) & ~(size_t)15u;
    const size_t bytes = head + spans.size() * sizeof(GiState::DeformSource);
    GI_HIP(ctx, vstage_reserve(g, bytes, bytes));
    UpdateCall uc{ctx, g, (hipStream_t)stream_, true};
    if (int rc = update_begin(uc, true); rc != NEB_OK)
        return rc;
    // ---- commit the host side: the slot; h_pos is left behind (host_stale), the boxes follow with the result record ----
    uint8_t* base = (uint8_t*)g->h_vstage + (size_t)uc.slot * g->vstage_cap;
    GiState::DeformRange* ranges = (GiState::DeformRange*)base;
    GiState::DeformSource* sources = (GiState::DeformSource*)(base + head);
    uint32_t lane = 0;
    bool any_attr = false;
    for (size_t i = 0; i < spans.size(); ++i) {
        const VertexSpan& sp = spans[i];
        const neb_vertex_update& u = updates[sp.k];
        GiState::DeformRange& r = ranges[i];
        r.first_lane = lane, r.count = sp.count, r.dst = g->h_geoms[sp.geom].vertexBase + sp.first, r.geom = sp.geom, r.pad = 0;
        roll_mark(g, sp.geom, sp.first, sp.count); // (the host cannot know of a refusal on the device: the roll then copies equal values)
        r.pos_off = 0;
        r.nrm_off = u.normals ? 0u : GiState::kNoStream; // (device sources: only "has the stream" is read)
        r.tan_off = u.tangents ? 0u : GiState::kNoStream;
        sources[i] = {(const uint8_t*)u.positions, (const uint8_t*)u.normals, (const uint8_t*)u.tangents, u.positionStride, u.normalStride, u.tangentStride, 0u};
        lane += sp.count;
        any_attr = any_attr || u.normals || u.tangents;
        update_touch(uc, sp.geom);
    }
    if (uc.any_tris)
        refit_drop_sun_table(g);
    // ---- enqueue: check, scatter, bake, records, boxes, levels, quantise, the record back ----
    const uint32_t n_ranges = (uint32_t)spans.size(), n_pool = (uint32_t)(g->h_pos.size() / 3);
    uint32_t* refused = result_refusal_word(g, uc.slot);
    GI_HIP(ctx, update_record_init(uc));
    hipLaunchKernelGGL(deform_check_kernel, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)ranges, n_ranges,
                       (const GiState::DeformSource*)sources, lane, g->n_geoms, (const float*)g->d_xf, refused);
    hipLaunchKernelGGL(deform_scatter_kernel<true>, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)ranges, n_ranges,
                       (const float*)nullptr, lane, n_pool, g->n_geoms, uc.call, g->d_pos, const_cast<float*>(g->view.normals),
                       const_cast<float*>(g->view.tangents), g->d_geom_epoch, (const GiState::DeformSource*)sources, (const uint32_t*)refused,
                       g->d_deform_dirty);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream));
    return update_finish(uc, any_attr);
}

// ---- skinned submeshes ----
int neb_gi_set_skin(neb_ctx* ctx, const neb_skin_desc* skins, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_set_skin";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_set_skin: no scene (call neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!skins)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: null pointer");
    if (n > g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: more entries than geometries (an index is out of range or named twice)");
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t stamp = ++g->seen_stamp;
    uint32_t n_skins = g->n_skins, n_joints = g->skin_joints;
    std::vector<size_t> block_bytes(n, 0); // (64 bytes per vertex: GiState::Skin)
    for (uint32_t k = 0; k < n; ++k) {
        const neb_skin_desc& d = skins[k];
        if (int rc = geometry_named_once(ctx, g, stamp, d.geometry, who, NEB_ERR_INVALID_ARG); rc != NEB_OK)
            return rc;
        if (!g->skins.empty() && g->skins[d.geometry].n_joints)
            n_skins -= 1u, n_joints -= g->skins[d.geometry].n_joints;
        if (!d.joints)
            continue; // (remove)
        if (d.numJoints == 0 || d.numJoints > 65535u)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: numJoints must be 1 .. 65535");
        if (!d.weights)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: joints without weights");
        if (d.jointStride < 8u || d.weightStride < 16u)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: a stride is smaller than its element");
        n_skins += 1u, n_joints += d.numJoints;
        const uint32_t nv = g->h_geoms[d.geometry].n_verts;
        block_bytes[k] = std::max<size_t>(64, (size_t)64 * nv);
        for (uint32_t v = 0; v < nv; ++v) {
            uint16_t j4[4];
            float w4[4];
            memcpy(j4, (const uint8_t*)d.joints + (size_t)v * d.jointStride, 8);
            memcpy(w4, (const uint8_t*)d.weights + (size_t)v * d.weightStride, 16);
            for (int q = 0; q < 4; ++q) {
                if (j4[q] >= d.numJoints) // (an influence of weight zero counts: the kernel reads its matrix)
                    return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_skin: a joint index is not below numJoints");
                if (!std::isfinite(w4[q]))
                    return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_set_skin: a weight is not a finite number");
            }
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    // the fresh blocks: joints and weights repacked tight, and the bind pose from the pools (the buffer of arguments is shared with the morph calls)
    std::vector<void*> fresh;
    std::vector<uint16_t> hj;
    std::vector<float> hw;
    const auto fill = [&](uint32_t k, uint8_t* b) {
        const neb_skin_desc& d = skins[k];
        const GiState::HostGeom& hg = g->h_geoms[d.geometry];
        const size_t nv = hg.n_verts;
        if (!nv)
            return hipSuccess;
        hj.resize(4 * nv), hw.resize(4 * nv);
        for (size_t v = 0; v < nv; ++v) {
            memcpy(&hj[4 * v], (const uint8_t*)d.joints + v * d.jointStride, 8);
            memcpy(&hw[4 * v], (const uint8_t*)d.weights + v * d.weightStride, 16);
        }
        hipError_t e = hipMemcpy(b, hw.data(), 16 * nv, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(b + 32 * nv, hj.data(), 8 * nv, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b + 40 * nv, g->d_pos + 3 * (size_t)hg.vertexBase, 12 * nv, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b + 52 * nv, g->view.normals + 3 * (size_t)hg.vertexBase, 12 * nv, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b + 16 * nv, g->view.tangents + 4 * (size_t)hg.vertexBase, 16 * nv, hipMemcpyDeviceToDevice, stream);
        return e;
    };
    if (int rc = setup_fresh_blocks(ctx, g, stream, who, block_bytes, GiState::args_capacity(n_skins, n_joints, g->n_morphs, g->morph_targets), fresh, fill);
        rc != NEB_OK)
        return rc;
    // ---- commit: nothing below can fail ----
    if (g->skins.empty())
        g->skins.resize(g->n_geoms);
    g->n_skins = n_skins, g->skin_joints = n_joints;
    for (uint32_t k = 0; k < n; ++k) {
        GiState::Skin& sk = rebind_block(g->skins, skins[k].geometry, fresh[k]);
        if (fresh[k])
            sk.n_joints = skins[k].numJoints;
    }
    return NEB_OK;
}

int neb_gi_skin_vertices(neb_ctx* ctx, const neb_skin_update* updates, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_skin_vertices";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_skin_vertices: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_skin_vertices: null pointer");
    if (n > g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_skin_vertices: more entries than geometries (an index is out of range or named twice)");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything the HOST can refuse the call for comes before anything changes (the skinned vertices themselves: skin_check_kernel) ----
    const uint32_t stamp = ++g->seen_stamp;
    struct Span { uint32_t geom, k; };
    std::vector<Span> spans;
    spans.reserve(n);
    size_t n_lanes = 0, n_mats = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_skin_update& u = updates[k];
        if (int rc = geometry_named_once(ctx, g, stamp, u.geometry, who, NEB_ERR_INVALID_ARG); rc != NEB_OK)
            return rc;
        if (!u.jointMatrices)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_skin_vertices: null jointMatrices");
        if (g->skins.empty() || !g->skins[u.geometry].n_joints)
            return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_skin_vertices: the geometry has no skin (neb_gi_set_skin first)");
    }
    for (uint32_t k = 0; k < n; ++k) {
        const neb_skin_update& u = updates[k];
        const uint32_t nj = g->skins[u.geometry].n_joints;
        if (!palette_finite(u.jointMatrices, nj))
            return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_skin_vertices: a joint matrix entry (columns 0-2) is not a finite number");
        if (g->h_geoms[u.geometry].n_verts == 0)
            continue; // (no lane: a range is never empty)
        spans.push_back({u.geometry, k});
        n_lanes += g->h_geoms[u.geometry].n_verts;
        n_mats += nj;
    }
    if (n_lanes > 0xffffffffull / 10u) // (the bound of neb_gi_update_vertices: lanes are 32-bit)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_skin_vertices: too many vertices in one call");
    if (spans.empty())
        return NEB_OK;
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.geom < b.geom; });
    GI_GUARD(ctx);
    GI_HIP(ctx, results_prepare(g));
    // ---- the staging slot: pinned host memory, {ranges | sources | palettes}, copied to the palette buffer in one piece ----
    const size_t head = spans.size() * sizeof(GiState::DeformRange), src_bytes = spans.size() * sizeof(GiState::SkinSource);
    const size_t bytes = head + src_bytes + 64u * n_mats;
    static_assert(sizeof(GiState::DeformRange) == 32 && sizeof(GiState::SkinSource) == 32, "64 bytes of ranges per bound geometry (neb_gi_set_skin)");
    if (bytes > g->skin_args_cap)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_skin_vertices: the palette buffer is smaller than the call (internal)");
    GI_HIP(ctx, vstage_reserve(g, bytes, std::max(bytes, g->skin_args_cap))); // (at once for a call that names every skin)
    UpdateCall uc{ctx, g, (hipStream_t)stream_, true};
    if (int rc = update_begin(uc, true); rc != NEB_OK)
        return rc;
    // ---- commit the host side: the slot; h_pos is left behind (host_stale), the boxes follow with the result record ----
    uint8_t* base = (uint8_t*)g->h_vstage + (size_t)uc.slot * g->vstage_cap;
    GiState::DeformRange* ranges = (GiState::DeformRange*)base;
    GiState::SkinSource* sources = (GiState::SkinSource*)(base + head);
    float* palette = (float*)(base + head + src_bytes);
    uint32_t lane = 0, mat = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        const uint32_t gi = spans[i].geom;
        const GiState::HostGeom& hg = g->h_geoms[gi];
        const GiState::Skin& sk = g->skins[gi];
        ranges[i] = {lane, hg.n_verts, hg.vertexBase, gi, 0u, hg.valid ? 0u : GiState::kNoStream, hg.valid ? 0u : GiState::kNoStream, 0u};
        sources[i] = {(const uint8_t*)sk.d_block, hg.n_verts, mat, sk.n_joints, hg.valid ? 1u : 0u, {0u, 0u}};
        memcpy(palette + 16 * (size_t)mat, updates[spans[i].k].jointMatrices, 64 * (size_t)sk.n_joints);
        roll_mark(g, gi, 0, hg.n_verts); // (the host cannot know of a refusal on the device: the roll then copies equal values)
        lane += hg.n_verts, mat += sk.n_joints;
        update_touch(uc, gi);
    }
    if (uc.any_tris)
        refit_drop_sun_table(g);
    // ---- enqueue: arguments, check, skin, bake, records, boxes, levels, quantise, the record back ----
    const uint32_t n_ranges = (uint32_t)spans.size(), n_pool = (uint32_t)(g->h_pos.size() / 3);
    uint32_t* refused = result_refusal_word(g, uc.slot);
    const uint8_t* d_args = (const uint8_t*)g->d_skin_args;
    GI_HIP(ctx, update_record_init(uc));
    GI_HIP(ctx, hipMemcpyAsync(g->d_skin_args, base, bytes, hipMemcpyHostToDevice, uc.stream));
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream)); // (the copy was the slot's last reader: the kernels read the device buffer)
    hipLaunchKernelGGL(skin_check_kernel, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)d_args, n_ranges,
                       (const GiState::SkinSource*)(d_args + head), (const float*)(d_args + head + src_bytes), lane, g->n_geoms, (const float*)g->d_xf,
                       refused);
    hipLaunchKernelGGL(skin_scatter_kernel, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)d_args, n_ranges,
                       (const GiState::SkinSource*)(d_args + head), (const float*)(d_args + head + src_bytes), lane, n_pool, g->n_geoms, uc.call, g->d_pos,
                       const_cast<float*>(g->view.normals), const_cast<float*>(g->view.tangents), g->d_geom_epoch, (const uint32_t*)refused,
                       g->d_deform_dirty);
    GI_HIP(ctx, hipGetLastError());
    return update_finish(uc, true);
}

// ---- morph targets ----
int neb_gi_set_morph_targets(neb_ctx* ctx, const neb_morph_desc* descs, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_set_morph_targets";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_set_morph_targets: no scene (call neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!descs)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: null pointer");
    if (n > g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: more entries than geometries (an index is out of range or named twice)");
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t stamp = ++g->seen_stamp;
    uint32_t n_morphs = g->n_morphs, n_targets = g->morph_targets;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_morph_desc& d = descs[k];
        if (int rc = geometry_named_once(ctx, g, stamp, d.geometry, who, NEB_ERR_INVALID_ARG); rc != NEB_OK)
            return rc;
        if (!g->morphs.empty() && g->morphs[d.geometry].n_targets)
            n_morphs -= 1u, n_targets -= g->morphs[d.geometry].n_targets;
        if (d.numTargets == 0)
            continue; // (remove)
        if (d.numTargets > 65535u)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: numTargets must be 0 .. 65535");
        if (!d.positionDeltas)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: null positionDeltas");
        if ((d.normalDeltas || d.tangentDeltas) && !g->h_geoms[d.geometry].valid)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: normal or tangent deltas for a geometry that was set without its attribute streams");
        if (d.positionStride < 12u || (d.normalDeltas && d.normalStride < 12u) || (d.tangentDeltas && d.tangentStride < 12u))
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: a stride is smaller than its element");
        for (uint32_t t = 0; t < d.numTargets; ++t)
            if (!d.positionDeltas[t] || (d.normalDeltas && !d.normalDeltas[t]) || (d.tangentDeltas && !d.tangentDeltas[t]))
                return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_morph_targets: a null target pointer");
        n_morphs += 1u, n_targets += d.numTargets;
    }
    // the deltas repacked tight and target-major, {positions | normals | tangents}, and looked at on the way
    std::vector<std::vector<float>> packed(n);
    std::vector<size_t> block_bytes(n, 0); // (the rest pose, 40 bytes per vertex, then the deltas: GiState::Morph)
    for (uint32_t k = 0; k < n; ++k) {
        const neb_morph_desc& d = descs[k];
        if (d.numTargets == 0)
            continue;
        const size_t nv = g->h_geoms[d.geometry].n_verts;
        const void* const* streams[3] = {d.positionDeltas, d.normalDeltas, d.tangentDeltas};
        const uint32_t strides[3] = {d.positionStride, d.normalStride, d.tangentStride};
        std::vector<float>& out = packed[k];
        out.resize(3 * nv * d.numTargets * (1u + (d.normalDeltas ? 1u : 0u) + (d.tangentDeltas ? 1u : 0u)));
        block_bytes[k] = std::max<size_t>(64, (size_t)40 * nv + out.size() * sizeof(float));
        float* dst = out.data();
        for (int q = 0; q < 3; ++q) {
            if (!streams[q])
                continue;
            for (uint32_t t = 0; t < d.numTargets; ++t)
                for (size_t v = 0; v < nv; ++v, dst += 3) {
                    memcpy(dst, (const uint8_t*)streams[q][t] + v * strides[q], 12);
                    if (!(std::isfinite(dst[0]) && std::isfinite(dst[1]) && std::isfinite(dst[2])))
                        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_set_morph_targets: a delta is not a finite number");
                }
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    // the fresh blocks: the deltas, and the rest pose from the pools
    std::vector<void*> fresh;
    const auto fill = [&](uint32_t k, uint8_t* b) {
        const GiState::HostGeom& hg = g->h_geoms[descs[k].geometry];
        const size_t nv = hg.n_verts;
        if (!nv)
            return hipSuccess;
        hipError_t e = hipMemcpy(b + 40 * nv, packed[k].data(), packed[k].size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b, g->view.tangents + 4 * (size_t)hg.vertexBase, 16 * nv, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b + 16 * nv, g->d_pos + 3 * (size_t)hg.vertexBase, 12 * nv, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b + 28 * nv, g->view.normals + 3 * (size_t)hg.vertexBase, 12 * nv, hipMemcpyDeviceToDevice, stream);
        return e;
    };
    if (int rc = setup_fresh_blocks(ctx, g, stream, who, block_bytes, GiState::args_capacity(g->n_skins, g->skin_joints, n_morphs, n_targets), fresh, fill);
        rc != NEB_OK)
        return rc;
    // ---- commit: nothing below can fail ----
    if (g->morphs.empty())
        g->morphs.resize(g->n_geoms);
    g->n_morphs = n_morphs, g->morph_targets = n_targets;
    for (uint32_t k = 0; k < n; ++k) {
        GiState::Morph& mo = rebind_block(g->morphs, descs[k].geometry, fresh[k]);
        if (fresh[k]) {
            mo.n_targets = descs[k].numTargets;
            mo.has_n = descs[k].normalDeltas != nullptr, mo.has_t = descs[k].tangentDeltas != nullptr;
        }
    }
    return NEB_OK;
}

int neb_gi_morph_vertices(neb_ctx* ctx, const neb_morph_update* updates, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_morph_vertices";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_morph_vertices: no built scene (neb_gi_set_scene + neb_gi_build_bvh first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_morph_vertices: null pointer");
    if (n > g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_morph_vertices: more entries than geometries (an index is out of range or named twice)");
    GI_HIP(ctx, gi_harvest_results(g, false));
    // ---- everything the HOST can refuse the call for comes before anything changes (the blended vertices themselves: morph_check_kernel) ----
    const uint32_t stamp = ++g->seen_stamp;
    struct Span { uint32_t geom, k; };
    std::vector<Span> spans;
    spans.reserve(n);
    size_t n_lanes = 0, n_mats = 0, n_active = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_morph_update& u = updates[k];
        if (int rc = geometry_named_once(ctx, g, stamp, u.geometry, who, NEB_ERR_INVALID_ARG); rc != NEB_OK)
            return rc;
        if (!u.weights)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_morph_vertices: null weights");
        if (g->morphs.empty() || !g->morphs[u.geometry].n_targets)
            return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_morph_vertices: the geometry has no targets (neb_gi_set_morph_targets first)");
        if (u.jointMatrices && (g->skins.empty() || !g->skins[u.geometry].n_joints))
            return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_morph_vertices: jointMatrices for a geometry without a skin (neb_gi_set_skin first)");
    }
    for (uint32_t k = 0; k < n; ++k) {
        const neb_morph_update& u = updates[k];
        const uint32_t nt = g->morphs[u.geometry].n_targets, nj = u.jointMatrices ? g->skins[u.geometry].n_joints : 0u;
        uint32_t active = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            if (!std::isfinite(u.weights[t]))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_morph_vertices: a weight is not a finite number");
            active += u.weights[t] != 0.f ? 1u : 0u; // (+0 and -0 both drop out)
        }
        if (!palette_finite(u.jointMatrices, nj))
            return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_morph_vertices: a joint matrix entry (columns 0-2) is not a finite number");
        if (g->h_geoms[u.geometry].n_verts == 0)
            continue; // (no lane: a range is never empty)
        spans.push_back({u.geometry, k});
        n_lanes += g->h_geoms[u.geometry].n_verts;
        n_mats += nj;
        n_active += active;
    }
    if (n_lanes > 0xffffffffull / 10u) // (the bound of neb_gi_update_vertices: lanes are 32-bit)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_morph_vertices: too many vertices in one call");
    if (spans.empty())
        return NEB_OK;
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.geom < b.geom; });
    GI_GUARD(ctx);
    GI_HIP(ctx, results_prepare(g));
    // ---- the staging slot: pinned host memory, {ranges | sources | active lists | palettes}, copied to the argument buffer in one piece ----
    static_assert(sizeof(GiState::DeformRange) == 32 && sizeof(GiState::MorphSource) == 48 && sizeof(GiState::MorphPair) == 8,
                  "80 bytes of ranges per bound geometry, 8 per target (GiState::args_capacity)");
    const size_t head = spans.size() * sizeof(GiState::DeformRange), src_bytes = spans.size() * sizeof(GiState::MorphSource);
    const size_t act_bytes = (n_active * sizeof(GiState::MorphPair) + 15u) & ~(size_t)15u; // (the palette is read in 16-byte pieces)
    const size_t bytes = head + src_bytes + act_bytes + 64u * n_mats;
    if (bytes > g->skin_args_cap)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_morph_vertices: the argument buffer is smaller than the call (internal)");
    GI_HIP(ctx, vstage_reserve(g, bytes, std::max(bytes, g->skin_args_cap))); // (at once for a call that names every geometry)
    UpdateCall uc{ctx, g, (hipStream_t)stream_, true};
    if (int rc = update_begin(uc, true); rc != NEB_OK)
        return rc;
    // ---- commit the host side: the slot; h_pos is left behind (host_stale), the boxes follow with the result record ----
    uint8_t* base = (uint8_t*)g->h_vstage + (size_t)uc.slot * g->vstage_cap;
    GiState::DeformRange* ranges = (GiState::DeformRange*)base;
    GiState::MorphSource* sources = (GiState::MorphSource*)(base + head);
    GiState::MorphPair* pairs = (GiState::MorphPair*)(base + head + src_bytes);
    float* palette = (float*)(base + head + src_bytes + act_bytes);
    uint32_t lane = 0, mat = 0, act = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        const uint32_t gi = spans[i].geom;
        const neb_morph_update& u = updates[spans[i].k];
        const GiState::HostGeom& hg = g->h_geoms[gi];
        const GiState::Morph& mo = g->morphs[gi];
        const uint32_t nj = u.jointMatrices ? g->skins[gi].n_joints : 0u, act_first = act;
        for (uint32_t t = 0; t < mo.n_targets; ++t)
            if (u.weights[t] != 0.f)
                pairs[act++] = {t, u.weights[t]};
        ranges[i] = {lane, hg.n_verts, hg.vertexBase, gi, 0u, hg.valid ? 0u : GiState::kNoStream, hg.valid ? 0u : GiState::kNoStream, 0u};
        sources[i] = {(const uint8_t*)mo.d_block, nj ? (const uint8_t*)g->skins[gi].d_block : nullptr, hg.n_verts, mo.n_targets, act_first, act - act_first,
                      mat, nj, (hg.valid ? GiState::kMorphAttrs : 0u) | (mo.has_n ? GiState::kMorphNormals : 0u) | (mo.has_t ? GiState::kMorphTangents : 0u), 0u};
        if (nj)
            memcpy(palette + 16 * (size_t)mat, u.jointMatrices, 64 * (size_t)nj);
        roll_mark(g, gi, 0, hg.n_verts); // (the host cannot know of a refusal on the device: the roll then copies equal values)
        lane += hg.n_verts, mat += nj;
        update_touch(uc, gi);
    }
    if (act_bytes > (size_t)act * sizeof(GiState::MorphPair))
        pairs[act] = {0u, 0.f}; // (the padding travels too)
    if (uc.any_tris)
        refit_drop_sun_table(g);
    // ---- enqueue: arguments, check, blend, bake, records, boxes, levels, quantise, the record back ----
    const uint32_t n_ranges = (uint32_t)spans.size(), n_pool = (uint32_t)(g->h_pos.size() / 3);
    uint32_t* refused = result_refusal_word(g, uc.slot);
    const uint8_t* d_args = (const uint8_t*)g->d_skin_args;
    GI_HIP(ctx, update_record_init(uc));
    GI_HIP(ctx, hipMemcpyAsync(g->d_skin_args, base, bytes, hipMemcpyHostToDevice, uc.stream));
    GI_HIP(ctx, stage_slot_release(g, uc.slot, uc.stream)); // (the copy was the slot's last reader: the kernels read the device buffer)
    hipLaunchKernelGGL(morph_check_kernel, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)d_args, n_ranges,
                       (const GiState::MorphSource*)(d_args + head), (const uint2*)(d_args + head + src_bytes),
                       (const float*)(d_args + head + src_bytes + act_bytes), lane, g->n_geoms, (const float*)g->d_xf, refused);
    hipLaunchKernelGGL(morph_scatter_kernel, dim3((lane + 255) / 256), dim3(256), 0, uc.stream, (const GiState::DeformRange*)d_args, n_ranges,
                       (const GiState::MorphSource*)(d_args + head), (const uint2*)(d_args + head + src_bytes),
                       (const float*)(d_args + head + src_bytes + act_bytes), lane, n_pool, g->n_geoms, uc.call, g->d_pos,
                       const_cast<float*>(g->view.normals), const_cast<float*>(g->view.tangents), g->d_geom_epoch, (const uint32_t*)refused,
                       g->d_deform_dirty);
    GI_HIP(ctx, hipGetLastError());
    return update_finish(uc, true);
}

int neb_gi_download_vertices(neb_ctx* ctx, uint32_t geometry, uint32_t firstVertex, uint32_t numVertices, float* positions, float* normals,
                             float* tangents, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_download_vertices: no scene (call neb_gi_set_scene first)");
    if (geometry >= g->n_geoms)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_download_vertices: geometry index out of range");
    const GiState::HostGeom& hg = g->h_geoms[geometry];
    if ((uint64_t)firstVertex + numVertices > hg.n_verts)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_download_vertices: vertex range beyond the geometry's numVertices");
    if (numVertices == 0)
        return NEB_OK;
    if (!positions)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_download_vertices: null positions");
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    GI_HIP(ctx, gi_scene_reader(g, stream)); // a rewrite enqueued on another stream comes first; a later one waits for these copies
    const size_t v = (size_t)hg.vertexBase + firstVertex;
    GI_HIP(ctx, hipMemcpyAsync(positions, g->d_pos + 3 * v, 12 * (size_t)numVertices, hipMemcpyDeviceToHost, stream));
    if (normals)
        GI_HIP(ctx, hipMemcpyAsync(normals, g->view.normals + 3 * v, 12 * (size_t)numVertices, hipMemcpyDeviceToHost, stream));
    if (tangents)
        GI_HIP(ctx, hipMemcpyAsync(tangents, g->view.tangents + 4 * v, 16 * (size_t)numVertices, hipMemcpyDeviceToHost, stream));
    GI_HIP(ctx, hipStreamSynchronize(stream));
    return NEB_OK;
}

int neb_gi_update_status(neb_ctx* ctx, uint64_t out[2])
{
    if (!ctx || !out)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_status: no scene (call neb_gi_set_scene first)");
    GI_GUARD(ctx);
    GI_HIP(ctx, gi_harvest_results(g, true));
    out[0] = g->device_updates_accepted, out[1] = g->device_updates_refused;
    return NEB_OK;
}

int neb_gi_scene_box(neb_ctx* ctx, float lo[3], float hi[3])
{
    if (!ctx || !lo || !hi)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_scene_box: no scene (call neb_gi_set_scene first)");
    GI_GUARD(ctx);
    GI_HIP(ctx, gi_harvest_results(g, true));
    memcpy(lo, g->scene_min, 12);
    memcpy(hi, g->scene_max, 12);
    return NEB_OK;
}

} // extern "C"
