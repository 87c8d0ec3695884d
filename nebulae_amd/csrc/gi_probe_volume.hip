// gi_probe_volume.hip -- what a host does with the records of neb_gi_bake_probes without taking them off the device:
// neb_gi_probe_grid writes the probes of a regular grid, neb_gi_accumulate_probes keeps a sample-weighted running mean of bakes, and
// neb_gi_gather_probes blends the eight records around each point into the irradiance for the point's normal.
//
// None of the three needs a scene or a frame, and none touches a plane, a counter or the sun table.  The arithmetic is the sequence
// include/nebulae_hip.h writes down, one IEEE operation per step: every product that feeds a sum is rounded by itself (rounded_mul).
// A file of its own, so that the kernels of gi_query.hip keep their device text and their register figures.
#include "probe_device.h" // (the shared probe arithmetic; turns floating-point contraction off for this file: see gi_device.h)

namespace neb {

namespace {

static_assert(sizeof(neb_probe_grid) == 40 && offsetof(neb_probe_grid, spacing) == 12 && offsetof(neb_probe_grid, dims) == 24
                  && offsetof(neb_probe_grid, backface_limit) == 36,
              "neb_probe_grid");
static_assert(sizeof(neb_probe_gather) == 32 && offsetof(neb_probe_gather, weight) == 12 && offsetof(neb_probe_gather, corners) == 16
                  && offsetof(neb_probe_gather, cell) == 20 && offsetof(neb_probe_gather, flags) == 24 && offsetof(neb_probe_gather, reserved) == 28,
              "neb_probe_gather");
static_assert(sizeof(neb_probe) == 32 && sizeof(neb_probe_record) == 128 && offsetof(neb_probe_record, samples) == 108
                  && offsetof(neb_probe_record, hits) == 112 && offsetof(neb_probe_record, flags) == 124,
              "the records of neb_gi_bake_probes: samples is the last word of a record's seventh float4, the eighth holds hits, backfaces, "
              "segments, flags");

// ------------------------------------------------------------------------------------------------
// neb_gi_probe_grid: one lane per probe, two 16-byte stores
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_grid_kernel(neb_probe_grid G, uint32_t count, float tmin, float tmax, float4* __restrict__ probes)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t x = i % G.dims[0], yz = i / G.dims[0], y = yz % G.dims[1], z = yz / G.dims[1];
    probes[2 * (size_t)i] = make_float4(grid_coordinate(G.origin[0], G.spacing[0], x), grid_coordinate(G.origin[1], G.spacing[1], y),
                                        grid_coordinate(G.origin[2], G.spacing[2], z), tmin);
    probes[2 * (size_t)i + 1] = make_float4(0.0f, 0.0f, 1.0f, tmax);
}

// ------------------------------------------------------------------------------------------------
// neb_gi_accumulate_probes: one lane per 16 bytes, eight lanes per probe, a pure stream (read acc, read add, write acc: 384 B a probe)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t saturating_sum(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s < a ? 0xffffffffu : s;
}

// Lane j of a probe's eight holds words 4 j .. 4 j + 3 of both records.  `samples` is the last word of lane 6, which the other seven
// read through a shuffle (eight lanes of one probe never straddle a wave: 64 is a multiple of 8, and so is the number of lanes).
__global__ __launch_bounds__(256) void probe_accumulate_kernel(float4* __restrict__ acc, const float4* __restrict__ add, size_t n_lanes)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_lanes;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (live) {
        a = acc[i];
        b = add[i];
    }
    const uint32_t j = threadIdx.x & 7u, holder = (threadIdx.x & 56u) | 6u; // (the lane within its wave that holds `samples`)
    const uint32_t sa = (uint32_t)__shfl((int)__float_as_uint(a.w), (int)holder, 64), sb = (uint32_t)__shfl((int)__float_as_uint(b.w), (int)holder, 64);
    if (!live || sb == 0u)
        return; // acc keeps all its bits
    if (sa == 0u) {
        acc[i] = b;
        return;
    }
    const uint32_t total = sa + sb;
    if (total < sa) { // does not fit 32 bits: only the flags word changes
        if (j == 7u) {
            a.w = __uint_as_float(__float_as_uint(a.w) | NEB_PROBE_SATURATED);
            acc[i] = a;
        }
        return;
    }
    const float wa = (float)((double)sa / (double)total), wb = (float)((double)sb / (double)total);
    float4 r;
    if (j == 7u) {
        r.x = __uint_as_float(saturating_sum(__float_as_uint(a.x), __float_as_uint(b.x)));
        r.y = __uint_as_float(saturating_sum(__float_as_uint(a.y), __float_as_uint(b.y)));
        r.z = __uint_as_float(saturating_sum(__float_as_uint(a.z), __float_as_uint(b.z)));
        r.w = __uint_as_float((__float_as_uint(a.w) | __float_as_uint(b.w)) & ~NEB_PROBE_NOT_BAKED);
    } else {
        r.x = __fadd_rn(rounded_mul(a.x, wa), rounded_mul(b.x, wb));
        r.y = __fadd_rn(rounded_mul(a.y, wa), rounded_mul(b.y, wb));
        r.z = __fadd_rn(rounded_mul(a.z, wa), rounded_mul(b.z, wb));
        r.w = j == 6u ? __uint_as_float(total) : __fadd_rn(rounded_mul(a.w, wa), rounded_mul(b.w, wb));
    }
    acc[i] = r;
}

// ------------------------------------------------------------------------------------------------
// neb_gi_gather_probes
// ------------------------------------------------------------------------------------------------
// One lane per point.  A lane whose point is usable finds its cell from the point alone; then one ballot asks whether every such lane
// of the wave has the cell of the first of them.  Pixels and lightmap texels mostly do: that wave takes the UNIFORM arm of gather_blend,
// lanes without a usable point riding along (their loads are the wave's, their result is not stored).  Any other wave takes the
// per-lane arm with those lanes masked off.  No LDS, no atomics; the answer of a point is the same bits on both arms, since both
// perform gather_blend's operations on the same operands.
__global__ __launch_bounds__(256) void probe_gather_kernel(neb_probe_grid G, const float4* __restrict__ records, const float4* __restrict__ points, uint32_t n,
                                                           float4* __restrict__ out)
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
    gather_wave(G, records, P, usable, E, W, corners);
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

// ------------------------------------------------------------------------------------------------
// neb_gbuffer_points / neb_gi_probe_indirect: a frame's pixels as the gather's points
// ------------------------------------------------------------------------------------------------
// One lane per pixel of rows first / W .. : two 16-byte stores.
__global__ __launch_bounds__(256) void gbuffer_points_kernel(FramePlanes F, size_t first, uint32_t n, float4* __restrict__ points)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    float4 p0, p1;
    pixel_point(F, first + i, p0, p1);
    points[2 * (size_t)i] = p0;
    points[2 * (size_t)i + 1] = p1;
}

// The fused pass: a wave owns an 8 x 8 pixel tile (gi.hip's gi_pixel), so that its pixels mostly share their grid cell and the wave takes
// gather_blend's scalar-load arm; decode -> locate -> gather -> weight -> radiance += , no point or gather record in memory.  Four tiles
// a block.  A pixel that is not gathered, or finds no probe, stores nothing.  No LDS, no atomics.  `records` and `radiance` are parameters
// of their own, __restrict__: only then does the compiler know that the store at the end cannot reach a record, and keeps the scalar loads.
__global__ __launch_bounds__(256) void probe_indirect_kernel(IndirectArgs a, const float4* __restrict__ records, float4* __restrict__ radiance)
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
    gather_wave(a.G, records, P, usable, E, W, corners);
    if (!usable || !(W > 0.0f))
        return;
    add_indirect_term(a, i, p0, p1, E, radiance);
}

} // namespace

} // namespace neb

using namespace neb;

extern "C" int neb_gi_probe_grid(neb_ctx* ctx, const neb_probe_grid* grid, float tmin, float tmax, neb_probe* probes, neb_stream stream_)
{
    static const char who[] = "neb_gi_probe_grid";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    uint32_t count = 0;
    if (int rc = grid_shape(ctx, who, grid, &count))
        return rc;
    const size_t probe_bytes = (size_t)count * sizeof(neb_probe);
    if (!probes)
        return fail(ctx, who, "null probes");
    if ((uintptr_t)probes & 15u)
        return fail(ctx, who, "misaligned pointer (probes: 16 bytes)");
    GI_GUARD(ctx);
    if (!device_readable(ctx, probes, probe_bytes))
        return fail(ctx, who, "probes is not memory this context's device reads, or the grid's probes leave its allocation");
    hipLaunchKernelGGL(probe_grid_kernel, dim3((count + 255u) / 256u), dim3(256), 0, (hipStream_t)stream_, *grid, count, tmin, tmax,
                       reinterpret_cast<float4*>(probes));
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_accumulate_probes(neb_ctx* ctx, neb_probe_record* acc, const neb_probe_record* add, uint32_t n, neb_stream stream_)
{
    static const char who[] = "neb_gi_accumulate_probes";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    if (n == 0)
        return NEB_OK;
    const size_t bytes = (size_t)n * sizeof(neb_probe_record);
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
    const size_t n_lanes = 8 * (size_t)n;
    hipLaunchKernelGGL(probe_accumulate_kernel, dim3((uint32_t)((n_lanes + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_,
                       reinterpret_cast<float4*>(acc), reinterpret_cast<const float4*>(add), n_lanes);
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_gather_probes(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_probe* points, uint32_t n,
                                    neb_probe_gather* out, neb_stream stream_)
{
    static const char who[] = "neb_gi_gather_probes";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    uint32_t count = 0;
    if (int rc = grid_shape(ctx, who, grid, &count))
        return rc;
    if (n == 0)
        return NEB_OK;
    const size_t record_bytes = (size_t)count * sizeof(neb_probe_record), point_bytes = (size_t)n * sizeof(neb_probe),
                 out_bytes = (size_t)n * sizeof(neb_probe_gather);
    if (!records || !points || !out)
        return fail(ctx, who, "null records, points or out");
    if (((uintptr_t)records & 31u) || ((uintptr_t)points & 15u) || ((uintptr_t)out & 31u))
        return fail(ctx, who, "misaligned pointer (records, out: 32 bytes; points: 16 bytes)");
    if (spans_overlap(out, out_bytes, points, point_bytes))
        return fail(ctx, who, "out overlaps points");
    if (spans_overlap(out, out_bytes, records, record_bytes))
        return fail(ctx, who, "out overlaps records");
    GI_GUARD(ctx);
    if (!device_readable(ctx, records, record_bytes))
        return fail(ctx, who, "records is not memory this context's device reads, or the grid's records leave its allocation");
    if (!device_readable(ctx, points, point_bytes))
        return fail(ctx, who, "points is not memory this context's device reads, or n points leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return fail(ctx, who, "out is not memory this context's device reads, or n records leave its allocation");
    hipLaunchKernelGGL(probe_gather_kernel, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_, *grid,
                       reinterpret_cast<const float4*>(records), reinterpret_cast<const float4*>(points), n, reinterpret_cast<float4*>(out));
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gbuffer_points(neb_ctx* ctx, uint32_t row0, uint32_t row1, neb_probe* points, neb_stream stream_)
{
    static const char who[] = "neb_gbuffer_points";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    if (int rc = rows_resident(ctx, who, row0, row1))
        return rc;
    const size_t n = (size_t)(row1 - row0) * ctx->W, point_bytes = n * sizeof(neb_probe);
    if (n > 0xffffffffull)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gbuffer_points: more than 2^32 - 1 pixels");
    if (!points)
        return fail(ctx, who, "null points");
    if ((uintptr_t)points & 15u)
        return fail(ctx, who, "misaligned pointer (points: 16 bytes)");
    const size_t npx = (size_t)ctx->W * (ctx->row_end - ctx->row_begin);
    const int read[3][2] = {{NEB_PLANE_WORLDPOS, 0}, {NEB_PLANE_NORMAL, ctx->cur}, {NEB_PLANE_DEPTH, ctx->cur}};
    for (const auto& pl : read)
        if (spans_overlap(points, point_bytes, ctx->planes[pl[0]][pl[1]], npx * kPlaneInfo[pl[0]].bytes_per_px))
            return fail(ctx, who, "points overlaps a G-buffer plane the call reads");
    if (int rc = svgf_flush_pending(ctx)) // (a held-back temporal pass is submitted before anything that follows it on the planes)
        return rc;
    GI_GUARD(ctx);
    if (!device_readable(ctx, points, point_bytes))
        return fail(ctx, who, "points is not memory this context's device reads, or the rows' points leave its allocation");
    hipLaunchKernelGGL(gbuffer_points_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_, frame_planes(ctx),
                       (size_t)(row0 - ctx->row_begin) * ctx->W, (uint32_t)n, reinterpret_cast<float4*>(points));
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_probe_indirect_rows(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_gi_constants* constants,
                                          uint32_t flags, uint32_t row0, uint32_t row1, neb_stream stream_)
{
    static const char who[] = "neb_gi_probe_indirect";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    uint32_t count = 0;
    if (int rc = grid_shape(ctx, who, grid, &count))
        return rc;
    if (flags & ~NEB_INDIRECT_FRAME_WEIGHT)
        return fail(ctx, who, "unknown flags (NEB_INDIRECT_FRAME_WEIGHT is the only one)");
    if ((flags & NEB_INDIRECT_FRAME_WEIGHT) && !constants)
        return fail(ctx, who, "null constants with NEB_INDIRECT_FRAME_WEIGHT (cameraWorldPos is read)");
    if (int rc = rows_resident(ctx, who, row0, row1))
        return rc;
    const size_t record_bytes = (size_t)count * sizeof(neb_probe_record);
    if (!records)
        return fail(ctx, who, "null records");
    if ((uintptr_t)records & 31u)
        return fail(ctx, who, "misaligned pointer (records: 32 bytes)");
    const size_t npx = (size_t)ctx->W * (ctx->row_end - ctx->row_begin);
    if (spans_overlap(records, record_bytes, ctx->planes[NEB_PLANE_RADIANCE][ctx->cur], npx * sizeof(float4)))
        return fail(ctx, who, "records overlaps the radiance plane");
    if (int rc = svgf_flush_pending(ctx)) // (a held-back temporal pass reads the plane this call writes)
        return rc;
    GI_GUARD(ctx);
    if (!device_readable(ctx, records, record_bytes))
        return fail(ctx, who, "records is not memory this context's device reads, or the grid's records leave its allocation");
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
    hipLaunchKernelGGL(probe_indirect_kernel, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, (hipStream_t)stream_, a, reinterpret_cast<const float4*>(records),
                       (float4*)ctx->planes[NEB_PLANE_RADIANCE][ctx->cur]);
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

extern "C" int neb_gi_probe_indirect(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_gi_constants* constants,
                                     uint32_t flags, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    return neb_gi_probe_indirect_rows(ctx, grid, records, constants, flags, ctx->row_begin, ctx->row_end, stream_);
}
