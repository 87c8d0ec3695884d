// gi_probe_visibility.hip -- what a probe knows of the geometry around it, and the gather that asks: neb_gi_bake_visibility
// walks the rays of neb_gi_probe_rays once and filters their distances into an 8 x 8 octahedral map of (mean distance, mean squared
// distance) per probe, neb_gi_accumulate_visibility keeps a weight-weighted running mean of such maps, and neb_gi_gather_probes_visible /
// neb_gi_probe_indirect_visible are the gather and the fused frame pass of gi_probe_volume.hip with DDGI's Chebyshev factor per corner:
// a probe behind a wall thinner than a cell no longer lights the point.
//
// The records of neb_gi_bake_probes, every call that exists and every kernel of the other files are left as they are: the maps live in
// a buffer of their own, parallel to the records.  The gather itself is probe_device.h's gather_blend, the text the plain gather runs,
// with its VISIBLE arm.  The arithmetic is the sequence include/nebulae_hip.h writes down, one IEEE operation per step.
#include "probe_device.h" // (the shared probe arithmetic; turns floating-point contraction off for this file: see gi_device.h)

namespace neb {

namespace {

static_assert(sizeof(neb_probe_visibility) == 768 && offsetof(neb_probe_visibility, weight) == 512 && sizeof(neb_probe_visibility) == kVisibilityFloat2 * 8,
              "neb_probe_visibility: 64 texels of two moments, then their 64 weights");
constexpr uint32_t kVisibilityMaxSamples = 4096, kVisibilityMaxRays = 1u << 28; // neb_gi_bake_probes' limits

// ------------------------------------------------------------------------------------------------
// neb_gi_bake_visibility
// ------------------------------------------------------------------------------------------------
// One wave per probe, one wave per workgroup, ray_query_kernel's LDS stack; lane k is texel k = i + 8 j of the map.  Round r gives lane
// l sample s = 64 r + l: the lane builds the sample's direction (probe_direction, what neb_gi_probe_rays writes for ray p * S + s),
// walks it once to the closest hit over the probe's (tmin, tmax) and puts (direction, distance) into 1 KB of LDS.  Then every lane
// folds the round's 64 samples into its own three sums IN SAMPLE ORDER (64 broadcast reads of 16 bytes): a texel's sums are plain
// sequential sums over s = 0 .. S - 1, no butterfly, no atomics.  Three 4-byte-per-lane-coalesced stores at the end (8 + 4 bytes a lane).
// A probe that is not baked costs one test and the same stores.
__global__ __launch_bounds__(64) void visibility_bake_kernel(SceneView S, const float4* __restrict__ probes, uint32_t samples, uint32_t frame_index,
                                                             float max_distance, float* __restrict__ out)
{
    __shared__ int stack_mem[kLdsStack * 64];
    __shared__ float4 sample_mem[64]; // {direction, distance} of the round's samples
    const uint32_t lane = threadIdx.x;
    int* stack = stack_mem + lane;
    const uint32_t p = blockIdx.x;
    const float4 p0 = probes[2 * (size_t)p], p1 = probes[2 * (size_t)p + 1]; // {position, tmin} {normal, tmax}: the same for every lane
    float* rec = out + 192 * (size_t)p;
    float2 moments = make_float2(max_distance, __fmul_rn(max_distance, max_distance));
    float weight = 0.0f;
    // (the same for every lane: read as a scalar, so that the branch is one)
    if (__builtin_amdgcn_readfirstlane((int)probe_baked<NEB_BAKE_SH>(p0, p1))) {
        // the texel's direction: the centre of texel (i, j) in -1 .. 1 (exact: odd multiples of 1/8), unfolded and normalised
        const float ex = __fsub_rn(rounded_mul(__fadd_rn((float)(lane & 7u), 0.5f) / 8.0f, 2.0f), 1.0f);
        const float ey = __fsub_rn(rounded_mul(__fadd_rn((float)(lane >> 3), 0.5f) / 8.0f, 2.0f), 1.0f);
        float vx = ex, vy = ey;
        const float vz = __fsub_rn(__fsub_rn(1.0f, fabsf(ex)), fabsf(ey));
        if (vz < 0.0f) {
            vx = rounded_mul(__fsub_rn(1.0f, fabsf(ey)), ex >= 0.0f ? 1.0f : -1.0f);
            vy = rounded_mul(__fsub_rn(1.0f, fabsf(ex)), ey >= 0.0f ? 1.0f : -1.0f);
        }
        const float vl = sqrtf(rounded_square_length(vx, vy, vz));
        const float nx = vx / vl, ny = vy / vl, nz = vz / vl;
        const float3 o = f3(p0.x, p0.y, p0.z);
        float A = 0.0f, M1 = 0.0f, M2 = 0.0f;
        for (uint32_t round = 0u; round < samples / 64u; ++round) {
            const uint32_t s = 64u * round + lane;
            const float3 dir = probe_direction<NEB_BAKE_SH>(p * samples + s, s, samples, frame_index, f3(0.0f, 0.0f, 0.0f));
            Hit h;
            const bool found = traverse(S, o, dir, p0.w, p1.w, false, stack, h);
            sample_mem[lane] = make_float4(dir.x, dir.y, dir.z, found ? fminf(h.t, max_distance) : max_distance);
            __syncthreads(); // (one wave: orders the 64 writes before the reads)
            for (uint32_t q = 0u; q < 64u; ++q) {
                const float4 sm = sample_mem[q];
                const float c = __fadd_rn(__fadd_rn(rounded_mul(nx, sm.x), rounded_mul(ny, sm.y)), rounded_mul(nz, sm.z));
                if (c < 0.25f) // (keeps the filter free of denormals: 0.25^32 = 2^-64)
                    continue;
                float g = c;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    g = rounded_mul(g, g); // c^32 by five squarings
                A = __fadd_rn(A, g);
                M1 = __fadd_rn(M1, rounded_mul(g, sm.w));
                M2 = __fadd_rn(M2, rounded_mul(g, rounded_mul(sm.w, sm.w)));
            }
            __syncthreads(); // (the reads before the next round's writes)
        }
        if (A > 0.0f) {
            moments = make_float2(M1 / A, M2 / A);
            weight = A;
        }
    }
    reinterpret_cast<float2*>(rec)[lane] = moments;
    rec[128u + lane] = weight;
}

// ------------------------------------------------------------------------------------------------
// neb_gi_accumulate_visibility: one lane per texel, a pure stream (read acc, read add, write acc: 36 bytes a texel)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void visibility_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ add, size_t n_texels)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n_texels)
        return;
    const size_t base = 192 * (t >> 6);
    const uint32_t k = (uint32_t)t & 63u;
    float2* const am = reinterpret_cast<float2*>(acc + base) + k;
    float* const aw = acc + base + 128u + k;
    const float wa = *aw, wb = add[base + 128u + k];
    if (wb == 0.0f)
        return; // acc keeps all its bits
    const float2 b = reinterpret_cast<const float2*>(add + base)[k];
    if (wa == 0.0f) {
        *am = b;
        *aw = wb;
        return;
    }
    const float2 a = *am;
    const float W = __fadd_rn(wa, wb);
    const float fa = wa / W, fb = wb / W;
    *am = make_float2(__fadd_rn(rounded_mul(a.x, fa), rounded_mul(b.x, fb)), __fadd_rn(rounded_mul(a.y, fa), rounded_mul(b.y, fb)));
    *aw = W;
}

// ------------------------------------------------------------------------------------------------
// neb_gi_gather_probes_visible / neb_gi_probe_indirect_visible: probe_gather_kernel and probe_indirect_kernel (gi_probe_volume.hip), their
// shape and their text, over gather_blend's VISIBLE arm
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_gather_visible_kernel(neb_probe_grid G, const float4* __restrict__ records, const float2* __restrict__ visibility,
                                                                   float normal_bias, const float4* __restrict__ points, uint32_t n, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n;
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = p0;
    if (live) {
        p0 = points[2 * (size_t)i]; // {position, -} {normal, -}
        p1 = points[2 * (size_t)i + 1];
    }
    GatherPoint P;
    const bool usable = locate_point(G, p0, p1, live, P);

    float3 E;
    float W;
    uint32_t corners;
    gather_wave<true>(G, records, P, usable, E, W, corners, visibility, normal_bias);
    if (!live)
        return;
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint4 r1 = make_uint4(0u, 0u, NEB_GATHER_NOT_GATHERED, 0u);
    if (usable) {
        r0 = make_float4(E.x, E.y, E.z, W);
        r1 = make_uint4(corners, P.cell, P.flags | (W > 0.0f ? 0u : NEB_GATHER_NO_PROBE), 0u);
    }
    out[2 * (size_t)i] = r0;
    *reinterpret_cast<uint4*>(out + 2 * (size_t)i + 1) = r1;
}

// A wave per 8 x 8 pixel tile, four tiles a block; `records`, `visibility` and `radiance` are parameters of their own, __restrict__, so
// that the store at the end is known not to reach a record and the record loads stay scalar.
__global__ __launch_bounds__(256) void probe_indirect_visible_kernel(IndirectArgs a, const float4* __restrict__ records, const float2* __restrict__ visibility,
                                                                     float normal_bias, float4* __restrict__ radiance)
{
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
    const uint32_t x = tile_x * 8u + (lane & 7u), y = a.row0 + tile_y * 8u + (lane >> 3);
    const bool live = tile < a.n_tiles && x < a.F.W && y < a.row1;
    const size_t i = live ? (size_t)(y - a.row_begin) * a.F.W + x : 0;
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = p0;
    if (live)
        pixel_point(a.F, i, p0, p1);
    GatherPoint P;
    const bool usable = locate_point(a.G, p0, p1, live, P);
    float3 E;
    float W;
    uint32_t corners;
    gather_wave<true>(a.G, records, P, usable, E, W, corners, visibility, normal_bias);
    if (!usable || !(W > 0.0f))
        return;
    add_indirect_term(a, i, p0, p1, E, radiance);
}

// What the two visible calls check of the visibility pointer before it is looked up.
int visibility_pointer(neb_ctx* ctx, const char* who, const neb_probe_visibility* visibility)
{
    if (!visibility)
        return fail(ctx, who, "null visibility");
    if ((uintptr_t)visibility & 31u)
        return fail(ctx, who, "misaligned pointer (visibility: 32 bytes)");
    return NEB_OK;
}

} // namespace

} // namespace neb

using namespace neb;

extern "C" int neb_gi_bake_visibility(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t frame_index, float max_distance,
                                      neb_probe_visibility* out, neb_stream stream_)
{
    static const char who[] = "neb_gi_bake_visibility";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_bake_visibility: scene/BVH not ready");
    if (samples < 64u || samples > kVisibilityMaxSamples || (samples & 63u))
        return fail(ctx, who, "samples must be a multiple of 64 in 64..4096");
    if ((uint64_t)n * samples > kVisibilityMaxRays)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_bake_visibility: more than 2^28 samples (n * samples) in one call");
    if (!(std::isfinite(max_distance) && max_distance > 0.0f))
        return fail(ctx, who, "max_distance must be finite and > 0");
    if (n == 0)
        return NEB_OK;
    const size_t probe_bytes = (size_t)n * sizeof(neb_probe), out_bytes = (size_t)n * sizeof(neb_probe_visibility);
    if (!probes || !out)
        return fail(ctx, who, "null probes or out");
    if (((uintptr_t)probes & 15u) || ((uintptr_t)out & 31u))
        return fail(ctx, who, "misaligned pointer (probes: 16 bytes; out: 32 bytes)");
    if (spans_overlap(probes, probe_bytes, out, out_bytes))
        return fail(ctx, who, "out overlaps probes");
    GI_GUARD(ctx);
    if (!device_readable(ctx, probes, probe_bytes))
        return fail(ctx, who, "probes is not memory this context's device reads, or n probes leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return fail(ctx, who, "out is not memory this context's device reads, or n records leave its allocation");
    hipStream_t stream = (hipStream_t)stream_;
    GI_HIP(ctx, gi_scene_reader(g, stream)); // behind any update enqueued on another stream; a later update waits for this stream
    hipLaunchKernelGGL(visibility_bake_kernel, dim3(n), dim3(64), 0, stream, g->view, reinterpret_cast<const float4*>(probes), samples, frame_index, max_distance,
                       reinterpret_cast<float*>(out));
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_accumulate_visibility(neb_ctx* ctx, neb_probe_visibility* acc, const neb_probe_visibility* add, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_accumulate_visibility";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    if (n == 0)
        return NEB_OK;
    const size_t bytes = (size_t)n * sizeof(neb_probe_visibility);
    if (!acc || !add)
        return fail(ctx, who, "null acc or add");
    if (((uintptr_t)acc & 31u) || ((uintptr_t)add & 31u))
        return fail(ctx, who, "misaligned pointer (acc, add: 32 bytes)");
    if (spans_overlap(acc, bytes, add, bytes))
        return fail(ctx, who, "add overlaps acc");
    GI_GUARD(ctx);
    if (!device_readable(ctx, acc, bytes))
        return fail(ctx, who, "acc is not memory this context's device reads, or n records leave its allocation");
    if (!device_readable(ctx, add, bytes))
        return fail(ctx, who, "add is not memory this context's device reads, or n records leave its allocation");
    const size_t n_texels = 64 * (size_t)n;
    hipLaunchKernelGGL(visibility_accumulate_kernel, dim3((uint32_t)((n_texels + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_,
                       reinterpret_cast<float*>(acc), reinterpret_cast<const float*>(add), n_texels);
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_gather_probes_visible(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_probe_visibility* visibility,
                                            float normal_bias, const neb_probe* points, uint32_t n, neb_probe_gather* out, neb_stream stream_)
{
    static const char who[] = "neb_gi_gather_probes_visible";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    uint32_t count = 0;
    if (int rc = grid_shape(ctx, who, grid, &count))
        return rc;
    if (!(std::isfinite(normal_bias) && normal_bias >= 0.0f))
        return fail(ctx, who, "normal_bias must be finite and >= 0");
    if (n == 0)
        return NEB_OK;
    const size_t record_bytes = (size_t)count * sizeof(neb_probe_record), visibility_bytes = (size_t)count * sizeof(neb_probe_visibility),
                 point_bytes = (size_t)n * sizeof(neb_probe), out_bytes = (size_t)n * sizeof(neb_probe_gather);
    if (!records || !points || !out)
        return fail(ctx, who, "null records, points or out");
    if (((uintptr_t)records & 31u) || ((uintptr_t)points & 15u) || ((uintptr_t)out & 31u))
        return fail(ctx, who, "misaligned pointer (records, out: 32 bytes; points: 16 bytes)");
    if (int rc = visibility_pointer(ctx, who, visibility))
        return rc;
    if (spans_overlap(out, out_bytes, points, point_bytes))
        return fail(ctx, who, "out overlaps points");
    if (spans_overlap(out, out_bytes, records, record_bytes))
        return fail(ctx, who, "out overlaps records");
    if (spans_overlap(out, out_bytes, visibility, visibility_bytes))
        return fail(ctx, who, "out overlaps visibility");
    GI_GUARD(ctx);
    if (!device_readable(ctx, records, record_bytes))
        return fail(ctx, who, "records is not memory this context's device reads, or the grid's records leave its allocation");
    if (!device_readable(ctx, visibility, visibility_bytes))
        return fail(ctx, who, "visibility is not memory this context's device reads, or the grid's records leave its allocation");
    if (!device_readable(ctx, points, point_bytes))
        return fail(ctx, who, "points is not memory this context's device reads, or n points leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return fail(ctx, who, "out is not memory this context's device reads, or n records leave its allocation");
    hipLaunchKernelGGL(probe_gather_visible_kernel, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_, *grid,
                       reinterpret_cast<const float4*>(records), reinterpret_cast<const float2*>(visibility), normal_bias,
                       reinterpret_cast<const float4*>(points), n, reinterpret_cast<float4*>(out));
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_probe_indirect_visible_rows(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records,
                                                  const neb_probe_visibility* visibility, float normal_bias, const neb_gi_constants* constants, uint32_t flags,
                                                  uint32_t row0, uint32_t row1, neb_stream stream_)
{
    static const char who[] = "neb_gi_probe_indirect_visible";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    uint32_t count = 0;
    if (int rc = grid_shape(ctx, who, grid, &count))
        return rc;
    if (flags & ~NEB_INDIRECT_FRAME_WEIGHT)
        return fail(ctx, who, "unknown flags (NEB_INDIRECT_FRAME_WEIGHT is the only one)");
    if ((flags & NEB_INDIRECT_FRAME_WEIGHT) && !constants)
        return fail(ctx, who, "null constants with NEB_INDIRECT_FRAME_WEIGHT (cameraWorldPos is read)");
    if (!(std::isfinite(normal_bias) && normal_bias >= 0.0f))
        return fail(ctx, who, "normal_bias must be finite and >= 0");
    if (int rc = rows_resident(ctx, who, row0, row1))
        return rc;
    const size_t record_bytes = (size_t)count * sizeof(neb_probe_record), visibility_bytes = (size_t)count * sizeof(neb_probe_visibility);
    if (!records)
        return fail(ctx, who, "null records");
    if ((uintptr_t)records & 31u)
        return fail(ctx, who, "misaligned pointer (records: 32 bytes)");
    if (int rc = visibility_pointer(ctx, who, visibility))
        return rc;
    const size_t npx = (size_t)ctx->W * (ctx->row_end - ctx->row_begin);
    if (spans_overlap(records, record_bytes, ctx->planes[NEB_PLANE_RADIANCE][ctx->cur], npx * sizeof(float4)))
        return fail(ctx, who, "records overlaps the radiance plane");
    if (spans_overlap(visibility, visibility_bytes, ctx->planes[NEB_PLANE_RADIANCE][ctx->cur], npx * sizeof(float4)))
        return fail(ctx, who, "visibility overlaps the radiance plane");
    if (int rc = svgf_flush_pending(ctx)) // (a held-back temporal pass reads the plane this call writes)
        return rc;
    GI_GUARD(ctx);
    if (!device_readable(ctx, records, record_bytes))
        return fail(ctx, who, "records is not memory this context's device reads, or the grid's records leave its allocation");
    if (!device_readable(ctx, visibility, visibility_bytes))
        return fail(ctx, who, "visibility is not memory this context's device reads, or the grid's records leave its allocation");
    IndirectArgs a;
    a.G = *grid;
    a.F = frame_planes(ctx);
    for (int q = 0; q < 3; ++q)
        a.camera[q] = (flags & NEB_INDIRECT_FRAME_WEIGHT) ? constants->cameraWorldPos[q] : 0.0f;
    a.row_begin = ctx->row_begin;
    a.row0 = row0;
    a.row1 = row1;
    a.tiles_x = (ctx->W + 7u) / 8u;
    a.n_tiles = a.tiles_x * ((row1 - row0 + 7u) / 8u);
    a.frame_weight = flags & NEB_INDIRECT_FRAME_WEIGHT;
    hipLaunchKernelGGL(probe_indirect_visible_kernel, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, (hipStream_t)stream_, a,
                       reinterpret_cast<const float4*>(records), reinterpret_cast<const float2*>(visibility), normal_bias,
                       (float4*)ctx->planes[NEB_PLANE_RADIANCE][ctx->cur]);
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_probe_indirect_visible(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_probe_visibility* visibility,
                                             float normal_bias, const neb_gi_constants* constants, uint32_t flags, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    return neb_gi_probe_indirect_visible_rows(ctx, grid, records, visibility, normal_bias, constants, flags, ctx->row_begin, ctx->row_end, stream_);
}
