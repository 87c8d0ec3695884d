// gi_probe_volume.hip -- what a host does with the records of neb_gi_bake_probes without taking them off the device:
// neb_gi_probe_grid writes the probes of a regular grid, neb_gi_accumulate_probes keeps a sample-weighted running mean of bakes, and
// neb_gi_gather_probes blends the eight records around each point into the irradiance for the point's normal.
//
// None of the three needs a scene or a frame, and none touches a plane, a counter or the sun table.  The arithmetic is the sequence
// include/nebulae_hip.h writes down, one IEEE operation per step: every product that feeds a sum is rounded by itself (rounded_mul).
// A file of its own, so that the kernels of gi_query.hip keep their device text and their register figures.
#include "gi_device.h" // (turns floating-point contraction off for this file: see there)

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
constexpr uint32_t kGridMaxProbes = 1u << 24;

// A product rounded by itself: the back end fuses a product into the sum that takes it whatever a pragma says (gi_query.hip's
// rounded_mul, gi_refit.hip's rounded_product); the empty statement is what the optimiser cannot see through.
__device__ __forceinline__ float rounded_mul(float a, float b)
{
    float p = __fmul_rn(a, b);
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ float rounded_square_length(float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(rounded_mul(x, x), rounded_mul(y, y)), rounded_mul(z, z));
}
// Where probe k of an axis sits: the one product and the one sum of include/nebulae_hip.h.  neb_gi_probe_grid and the gather both call
// this, which is why a point copied from a probe has vv == 0 against it.
__device__ __forceinline__ float grid_coordinate(float origin, float spacing, uint32_t k) { return __fadd_rn(origin, rounded_mul((float)k, spacing)); }

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
constexpr float kY00 = 0.282095f, kY1 = 0.488603f, kY2a = 1.092548f, kY20 = 0.315392f, kY22 = 0.546274f; // the bake's basis constants
constexpr float kA0 = 3.14159265f, kA1 = 2.0943951f, kA2 = 0.78539816f;                                  // pi, 2 pi / 3, pi / 4

// What a point has of its own before any record is looked at.
struct GatherPoint {
    float3 p, N;
    uint32_t base[3];
    float f[3];
    uint32_t cell, flags;
};

// The blend of one point.  UNIFORM = true: every lane of the wave that gathers at all has the cell `cell`, which is then a scalar: the
// record addresses are the same for every lane, the loads are scalar loads, a cell's eight records are fetched once for the wave, and
// "is this corner valid" is a scalar branch.  UNIFORM = false: the lane's own cell, vector loads.  The arithmetic is the same text.
// Two passes: the counters of the eight corners (each record's last 32-byte sector) give the weights and their sum; then the first
// seven float4 of the corners that count are blended with w / W.
template <bool UNIFORM>
__device__ __forceinline__ void gather_blend(const neb_probe_grid& G, const float4* __restrict__ records, const GatherPoint& P, uint32_t cell, float3& E,
                                             float& W, uint32_t& corners)
{
    const uint32_t nx = G.dims[0], ny = G.dims[1], nz = G.dims[2];
    float w[8];
    uint32_t valid = 0u; // corners whose record exists and passes the validity rule
    W = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
        const uint32_t cx = c & 1u, cy = (c >> 1) & 1u, cz = c >> 2;
        w[c] = 0.0f;
        if ((cx && nx < 2u) || (cy && ny < 2u) || (cz && nz < 2u)) // (the same for every lane)
            continue;
        const size_t probe = (size_t)cell + cx + (size_t)nx * (cy + (size_t)ny * cz);
        const float4 s6 = records[8 * probe + 6], s7 = records[8 * probe + 7];
        const uint32_t samples = __float_as_uint(s6.w), backfaces = __float_as_uint(s7.y), rflags = __float_as_uint(s7.w);
        const bool ok = samples != 0u && !(rflags & NEB_PROBE_NOT_BAKED) && !((float)backfaces > __fmul_rn(G.backface_limit, (float)samples));
        const float wx = cx ? P.f[0] : __fsub_rn(1.0f, P.f[0]), wy = cy ? P.f[1] : __fsub_rn(1.0f, P.f[1]), wz = cz ? P.f[2] : __fsub_rn(1.0f, P.f[2]);
        const float w_tri = __fmul_rn(__fmul_rn(wx, wy), wz);
        const float vx = __fsub_rn(grid_coordinate(G.origin[0], G.spacing[0], P.base[0] + cx), P.p.x);
        const float vy = __fsub_rn(grid_coordinate(G.origin[1], G.spacing[1], P.base[1] + cy), P.p.y);
        const float vz = __fsub_rn(grid_coordinate(G.origin[2], G.spacing[2], P.base[2] + cz), P.p.z);
        const float vv = rounded_square_length(vx, vy, vz);
        float d = 0.0f;
        if (vv > 0.0f)
            d = __fadd_rn(__fadd_rn(rounded_mul(vx, P.N.x), rounded_mul(vy, P.N.y)), rounded_mul(vz, P.N.z)) / sqrtf(vv);
        const float h = rounded_mul(__fadd_rn(d, 1.0f), 0.5f);
        const float w_n = __fadd_rn(rounded_mul(h, h), 0.2f);
        if (ok) {
            valid |= 1u << c;
            w[c] = __fmul_rn(w_tri, w_n);
            W = __fadd_rn(W, w[c]);
        }
    }
    float blend[27];
#pragma unroll
    for (int k = 0; k < 27; ++k)
        blend[k] = 0.0f;
    corners = 0u;
    const float r = 1.0f / W; // (W == 0: no corner below counts, r is not used)
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
        const uint32_t cx = c & 1u, cy = (c >> 1) & 1u, cz = c >> 2;
        const bool counts = w[c] > 0.0f;
        // (UNIFORM: a scalar branch on the record's validity, and the lanes whose own weight is 0 pass the words by; else the lane's own)
        if (UNIFORM ? (valid >> c) & 1u : counts) {
            const size_t probe = (size_t)cell + cx + (size_t)nx * (cy + (size_t)ny * cz);
            const float wn = __fmul_rn(w[c], r);
            float s[28];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const float4 v = records[8 * probe + q];
                s[4 * q] = v.x, s[4 * q + 1] = v.y, s[4 * q + 2] = v.z, s[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                const float sum = __fadd_rn(blend[k], rounded_mul(wn, s[k]));
                blend[k] = counts ? sum : blend[k];
            }
            corners |= counts ? 1u << c : 0u;
        }
    }
    E = f3(0.0f, 0.0f, 0.0f);
    if (!(W > 0.0f)) {
        W = 0.0f;
        return;
    }
    const float x = P.N.x, y = P.N.y, z = P.N.z;
    float K[9]; // A_l * Y_lm(N), the basis by the projection's formulas
    K[0] = __fmul_rn(kA0, kY00);
    K[1] = __fmul_rn(kA1, __fmul_rn(kY1, y));
    K[2] = __fmul_rn(kA1, __fmul_rn(kY1, z));
    K[3] = __fmul_rn(kA1, __fmul_rn(kY1, x));
    K[4] = __fmul_rn(kA2, __fmul_rn(kY2a, __fmul_rn(x, y)));
    K[5] = __fmul_rn(kA2, __fmul_rn(kY2a, __fmul_rn(y, z)));
    K[6] = __fmul_rn(kA2, __fmul_rn(kY20, __fsub_rn(rounded_mul(__fmul_rn(3.0f, z), z), 1.0f)));
    K[7] = __fmul_rn(kA2, __fmul_rn(kY2a, __fmul_rn(x, z)));
    K[8] = __fmul_rn(kA2, __fmul_rn(kY22, __fsub_rn(rounded_mul(x, x), rounded_mul(y, y))));
    float e[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            e[ch] = __fadd_rn(e[ch], rounded_mul(blend[3 * q + ch], K[q]));
    E = f3(fmaxf(0.0f, e[0]), fmaxf(0.0f, e[1]), fmaxf(0.0f, e[2]));
}

// A point's own part of the gather: is it usable, its unit normal, and per axis the cell's base probe and the fraction inside the cell.
// p0 = {position, -}, p1 = {normal, -}; `live`: the lane has a point at all.  Both gather kernels call this, so a pixel's point is located
// by the operations a point read from a buffer is.
__device__ __forceinline__ bool locate_point(const neb_probe_grid& G, const float4& p0, const float4& p1, bool live, GatherPoint& P)
{
    const float inf = __builtin_inff();
    const float nn = rounded_square_length(p1.x, p1.y, p1.z);
    const bool usable = live && rounded_square_length(p0.x, p0.y, p0.z) < inf && nn > 0.0f && nn < inf;
    P.p = f3(p0.x, p0.y, p0.z);
    const float nl = sqrtf(nn);
    P.N = f3(p1.x / nl, p1.y / nl, p1.z / nl);
    P.flags = 0u;
    const float pos[3] = {p0.x, p0.y, p0.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = __fsub_rn(pos[a], G.origin[a]) / G.spacing[a];
        const float tc = fminf(fmaxf(t, 0.0f), (float)(G.dims[a] - 1u));
        if (tc != t)
            P.flags |= NEB_GATHER_CLAMPED;
        const uint32_t top = G.dims[a] > 1u ? G.dims[a] - 2u : 0u;
        const uint32_t b = usable ? min((uint32_t)floorf(tc), top) : 0u; // (a lane without a usable point: any base inside the grid)
        P.base[a] = b;
        P.f[a] = __fsub_rn(tc, (float)b);
    }
    P.cell = P.base[0] + G.dims[0] * (P.base[1] + G.dims[1] * P.base[2]);
    return usable;
}

// The choice between gather_blend's two arms, made once per wave (every lane of the wave calls this).
__device__ __forceinline__ void gather_wave(const neb_probe_grid& G, const float4* __restrict__ records, const GatherPoint& P, bool usable, float3& E, float& W,
                                            uint32_t& corners)
{
    E = f3(0.0f, 0.0f, 0.0f);
    W = 0.0f;
    corners = 0u;
    const unsigned long long gathering = __ballot(usable);
    if (gathering != 0ull) {
        const uint32_t leader = (uint32_t)__ffsll(gathering) - 1u;
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)P.cell, (int)leader);
        if (__ballot(usable && P.cell != first) == 0ull)
            gather_blend<true>(G, records, P, first, E, W, corners);
        else if (usable)
            gather_blend<false>(G, records, P, P.cell, E, W, corners);
    }
}

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
struct FramePlanes {
    const uint2* world_pos;    // 4 x fp16: xyz read
    const uint32_t* normal;    // 2 words a pixel: word 1 holds the oct-packed shading normal (.zw), the only one read
    const uint32_t* depth;     // D24 | stencil << 24: stencil 0 is sky
    const uint32_t* albedo;    // R11G11B10
    const uint32_t* rough_metal; // 2 x fp16: the high half is metalness
    uint32_t W;
};

// The point gi_raygen shades at pixel i, by its expressions (gi.hip: worldPos, SN): p0 = {position, 0.01}, p1 = {shading normal, +inf}.
// A sky pixel has position 0 and normal 0, which the gather's usability rule turns away by itself.
__device__ __forceinline__ void pixel_point(const FramePlanes& F, size_t i, float4& p0, float4& p1)
{
    float3 worldPos = f3(0.0f, 0.0f, 0.0f), SN = worldPos;
    if (F.depth[i] >> 24) {
        const uint2 wp = F.world_pos[i];
        worldPos = f3(half_bits_to_float(wp.x & 0xffffu), half_bits_to_float(wp.x >> 16), half_bits_to_float(wp.y & 0xffffu));
        const uint32_t nzw = F.normal[2 * i + 1];
        SN = oct_unpack(half_bits_to_float(nzw & 0xffffu), half_bits_to_float(nzw >> 16));
    }
    p0 = make_float4(worldPos.x, worldPos.y, worldPos.z, 0.01f);
    p1 = make_float4(SN.x, SN.y, SN.z, __builtin_inff());
}

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

struct IndirectArgs {
    neb_probe_grid G;
    FramePlanes F;
    float camera[3];
    uint32_t row_begin, row0, row1, tiles_x, n_tiles, frame_weight;
};

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
    const float3 albedo = unpack_r11g11b10(a.F.albedo[i]);
    const float metalness = half_bits_to_float(a.F.rough_metal[i] >> 16);
    float3 k = albedo * (1.0f - metalness); // gi_raygen's throughput (:474)
    if (a.frame_weight) {
        // what gi_raygen's draw does to that throughput on average: with probability pd it is divided by pd, else kept, so the
        // expectation of the factor is pd * (1 / pd) + (1 - pd) = 2 - pd; a pd that is not > 0 never passes `Rand < pd`: the factor is 1
        const float3 worldPos = f3(p0.x, p0.y, p0.z), SN = f3(p1.x, p1.y, p1.z);
        const float3 V = f3(a.camera[0], a.camera[1], a.camera[2]) - worldPos; // :431
        const float3 F0 = specular_f0(albedo, metalness);
        const float pd = 1.0f - specular_probability(saturate1(dot3(normalize3(V), SN)), F0, albedo);
        const float factor = pd > 0.0f ? __fsub_rn(2.0f, pd) : 1.0f;
        k = f3(rounded_mul(k.x, factor), rounded_mul(k.y, factor), rounded_mul(k.z, factor));
    }
    float4 r = radiance[i];
    r.x = __fadd_rn(r.x, rounded_mul(rounded_mul(k.x, E.x), kPiInv));
    r.y = __fadd_rn(r.y, rounded_mul(rounded_mul(k.y, E.y), kPiInv));
    r.z = __fadd_rn(r.z, rounded_mul(rounded_mul(k.z, E.z), kPiInv));
    radiance[i] = r;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
bool spans_overlap(const void* a, size_t na, const void* b, size_t nb) // (gi_query.hip's ranges_overlap, which is local to that file)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int fail(neb_ctx* ctx, const char* who, const char* what)
{
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return gi_fail(ctx, NEB_ERR_INVALID_ARG, msg);
}

// What the grid calls check of the grid before anything else, with the caller's name in front -> the number of probes in `count`.
int grid_shape(neb_ctx* ctx, const char* who, const neb_probe_grid* grid, uint32_t* count)
{
    if (!grid)
        return fail(ctx, who, "null grid");
    uint64_t probes = 1;
    for (int a = 0; a < 3; ++a) {
        if (grid->dims[a] == 0u)
            return fail(ctx, who, "a dims of 0 (each axis has at least one probe)");
        if (grid->dims[a] > kGridMaxProbes)
            return fail(ctx, who, "more than 2^24 probes (dims[0] * dims[1] * dims[2])");
        probes *= grid->dims[a];
        if (probes > kGridMaxProbes)
            return fail(ctx, who, "more than 2^24 probes (dims[0] * dims[1] * dims[2])");
        if (!std::isfinite(grid->origin[a]))
            return fail(ctx, who, "origin is not finite");
        if (!(std::isfinite(grid->spacing[a]) && grid->spacing[a] > 0.0f))
            return fail(ctx, who, "spacing must be finite and > 0");
    }
    if (!(grid->backface_limit >= 0.0f && grid->backface_limit <= 1.0f))
        return fail(ctx, who, "backface_limit outside 0..1");
    *count = (uint32_t)probes;
    return NEB_OK;
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

namespace neb {
namespace {

int rows_resident(neb_ctx* ctx, const char* who, uint32_t row0, uint32_t row1)
{
    if (row0 < ctx->row_begin || row1 > ctx->row_end || row1 <= row0) {
        char msg[256];
        snprintf(msg, sizeof(msg), "%s: rows [%u, %u) are empty or not among the context's rows [%u, %u)", who, row0, row1, ctx->row_begin, ctx->row_end);
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, msg);
    }
    return NEB_OK;
}

FramePlanes frame_planes(const neb_ctx* ctx)
{
    FramePlanes F;
    F.world_pos = (const uint2*)ctx->planes[NEB_PLANE_WORLDPOS][0];
    F.normal = (const uint32_t*)ctx->planes[NEB_PLANE_NORMAL][ctx->cur];
    F.depth = (const uint32_t*)ctx->planes[NEB_PLANE_DEPTH][ctx->cur];
    F.albedo = (const uint32_t*)ctx->planes[NEB_PLANE_ALBEDO][0];
    F.rough_metal = (const uint32_t*)ctx->planes[NEB_PLANE_ROUGH_METAL][0];
    F.W = ctx->W;
    return F;
}

} // namespace
} // namespace neb

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
