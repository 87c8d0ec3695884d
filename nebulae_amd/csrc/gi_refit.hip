// gi_refit.hip -- moving submeshes: new instance transforms, the tree kept (neb_gi_update_transforms).
//
// Reference: RTAccelerationStructureBuilder::CreateTlas with a valid updateTlas (src/nri/raytracing/RTAccelerationStructureBuilder.cpp:100-130):
// the build re-runs with PERFORM_UPDATE, new instance transforms replace the old ones in place, the BLASes are not touched.  Here the
// acceleration structure is ONE tree over world-space triangles, so the counterpart is: bake the moved submeshes' triangles again on the
// device (same operation order as the host bake of neb_gi_set_scene, same bits), refit the boxes of the 128-byte nodes bottom-up, one
// launch per level, and quantise the 64-byte nodes again.  Topology, node numbering, leaf order and depth stay.
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

// one lane per leaf-order triangle slot: a slot of a moved geometry gets its triangle baked again, {geom, prim} stay
__global__ void rebake_kernel(float4* __restrict__ tris, uint32_t n_slots, uint32_t n_geoms, uint32_t epoch, const uint32_t* __restrict__ geom_epoch,
                              const DevGeom* __restrict__ geoms, const uint32_t* __restrict__ indices, const float* __restrict__ pos,
                              const float* __restrict__ xf)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots)
        return;
    const float4 ids = tris[3 * (size_t)i + 2];
    const uint32_t gi = __float_as_uint(ids.y), prim = __float_as_uint(ids.z);
    if (gi >= n_geoms || geom_epoch[gi] != epoch)
        return;
    const uint32_t first = geoms[gi].firstIndex + 3u * prim, vb = geoms[gi].vertexBase;
    const float* m = xf + 16 * (size_t)gi;
    const float3 w0 = bake_point(m, pos + 3 * (size_t)(vb + indices[first]));
    const float3 w1 = bake_point(m, pos + 3 * (size_t)(vb + indices[first + 1]));
    const float3 w2 = bake_point(m, pos + 3 * (size_t)(vb + indices[first + 2]));
    tris[3 * (size_t)i] = make_float4(w0.x, w0.y, w0.z, __fsub_rn(w1.x, w0.x));
    tris[3 * (size_t)i + 1] = make_float4(__fsub_rn(w1.y, w0.y), __fsub_rn(w1.z, w0.z), __fsub_rn(w2.x, w0.x), __fsub_rn(w2.y, w0.y));
    tris[3 * (size_t)i + 2] = make_float4(__fsub_rn(w2.z, w0.z), ids.y, ids.z, ids.w);
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

// One level of the tree, four lanes per node, one per child slot.  A leaf one of whose triangles moved takes the exact bounds of
// its triangles -- the whole triangle also where the slot holds a clipped reference of the splitting pass: conservative.  An inner
// child below which something changed takes the exact min / max of that node's four boxes (its level was refitted by the launch
// before: unused slots are inverted boxes and drop out of min / max by themselves).  Everything else keeps its bits.
__global__ void refit_level_kernel(Bvh4Node* __restrict__ nodes, uint32_t first, uint32_t count, uint32_t n_nodes, const float4* __restrict__ tris,
                                   uint32_t n_slots, uint32_t n_geoms, uint32_t epoch, const uint32_t* __restrict__ geom_epoch,
                                   uint32_t* __restrict__ node_epoch)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4u * count)
        return;
    const uint32_t i = first + (t >> 2), q = t & 3u;
    float* nf = reinterpret_cast<float*>(nodes + i);
    if (!(nf[q] <= nf[16 + q]))
        return; // unused slot (inverted box)
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

} // namespace neb

using namespace neb;

extern "C" {

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
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t call = g->epoch + 1u;
    const uint32_t stamp = ++g->seen_stamp; // (one per call, accepted or not: h_seen needs no clearing)
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gi = geometry_indices[k];
        if (gi >= g->n_geoms)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_transforms: geometry index out of range");
        if (g->h_seen[gi] == stamp)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_transforms: a geometry is named twice");
        g->h_seen[gi] = stamp;
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
        if (!changed[k])
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
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    // ---- the argument slot: pinned host memory the first kernel reads ----
    const int slot = (int)(call % (uint32_t)GiState::kStageSlots);
    if (!g->stage_ev[slot])
        GI_HIP(ctx, hipEventCreateWithFlags(&g->stage_ev[slot], hipEventDisableTiming));
    if (g->stage_used[slot])
        GI_HIP(ctx, hipEventSynchronize(g->stage_ev[slot])); // (the update kStageSlots calls ago: long done unless the host runs that far ahead)
    // ---- order: behind the last rewrite, and behind every stream that may still be reading what is about to be rewritten ----
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
    // ---- commit the host side ----
    g->epoch = call;
    GiState::StageEntry* st = g->h_stage + (size_t)slot * g->n_geoms;
    uint32_t ns = 0;
    bool any_tris = false;
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
        if (hg.n_tris) {
            hg.dirty = true;
            any_tris = true;
            memcpy(hg.world_lo, boxes[k].lo, 12);
            memcpy(hg.world_hi, boxes[k].hi, 12);
        }
    }
    if (any_tris) { // the scene box: the union of the geometries' exact boxes, as neb_gi_set_scene folds it
        float smin[3] = {3.4e38f, 3.4e38f, 3.4e38f}, smax[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
        for (const GiState::HostGeom& hg : g->h_geoms)
            if (hg.n_tris)
                for (int q = 0; q < 3; ++q) {
                    smin[q] = fminf(smin[q], hg.world_lo[q]);
                    smax[q] = fmaxf(smax[q], hg.world_hi[q]);
                }
        memcpy(g->scene_min, smin, sizeof(smin));
        memcpy(g->scene_max, smax, sizeof(smax));
    }
    // The sun table as after a scene change: the flags in the records are those of the old positions and are ignored from here on (state 2); the hold
    // policy of gi_sun_table_update decides when the next table is built -- and looks at the new scene box when it does.
    if (any_tris && g->sun_table_state != 0) {
        if (g->sun_table_state == 1)
            g->sun_hold = g->sun_hold_option > 0 ? (uint32_t)g->sun_hold_option : (g->sun_table_age < 32u ? 32u : 2u); // (kSunTableLife, kSunHoldAfterShortLife)
        g->sun_table_state = 2;
        g->sun_table_stale = true;
        g->sun_seen = 0;
    }
    // ---- enqueue ----
    const uint32_t n_slots = g->view.n_tris;
    hipLaunchKernelGGL(refit_apply_kernel, dim3((ns + 63) / 64), dim3(64), 0, stream, (const GiState::StageEntry*)st, ns, g->n_geoms, call, g->d_xf,
                       const_cast<DevGeom*>(g->view.geoms), const_cast<ShadeHeader*>(g->shade_heads), g->d_geom_epoch);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, hipEventRecord(g->stage_ev[slot], stream));
    g->stage_used[slot] = true;
    if (any_tris && n_slots) {
        hipLaunchKernelGGL(rebake_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, stream, const_cast<float4*>(g->view.tris), n_slots, g->n_geoms, call,
                           (const uint32_t*)g->d_geom_epoch, g->view.geoms, g->view.indices, g->d_pos, (const float*)g->d_xf);
        for (size_t lv = g->level_first.size(); lv-- > 1;) { // deepest level first
            const uint32_t first = g->level_first[lv - 1], count = g->level_first[lv] - first;
            if (count)
                hipLaunchKernelGGL(refit_level_kernel, dim3((4u * count + 255) / 256), dim3(256), 0, stream, const_cast<Bvh4Node*>(g->view.nodes), first, count,
                                   g->n_nodes, g->view.tris, n_slots, g->n_geoms, call, (const uint32_t*)g->d_geom_epoch, g->d_node_epoch);
        }
        GI_HIP(ctx, hipGetLastError());
        GI_HIP(ctx, gi_quantise_nodes(g->view.nodes, g->n_nodes, const_cast<Bvh4NodeQ*>(g->view.qnodes), stream));
    }
    GI_HIP(ctx, mark_rewrite(g, stream));
    return NEB_OK;
}

} // extern "C"
