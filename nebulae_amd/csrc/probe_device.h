// probe_device.h -- what the probe kernels of more than one file share (DESIGN.md 3.8c .. 3.8f): the rounded arithmetic, the bake's
// directions and its "is this probe baked" rule (gi_query.hip, gi_probe_visibility.hip), and the gather of a point with the checks the
// grid calls make on the host (gi_probe_volume.hip, gi_probe_visibility.hip).  One text, so that the files cannot drift apart; every
// function is local to the file that includes it, as it was when it stood there.
#pragma once
#include "gi_device.h" // (turns floating-point contraction off: see there)

namespace neb {

namespace {

// A product rounded by itself.  HIP's __fmul_rn is a plain operator, and the back end fuses a product into the sum that takes it
// whatever a pragma says (gi_refit.hip's rounded_product): the empty statement is what the optimiser cannot see through.
__device__ __forceinline__ float rounded_mul(float a, float b)
{
    float p = __fmul_rn(a, b);
    asm volatile("" : "+v"(p));
    return p;
}
// (x x + y y) + z z, every product and sum rounded by itself: the same bits as a float32 restatement, at the boundaries of 0 and overflow too
__device__ __forceinline__ float rounded_square_length(float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(rounded_mul(x, x), rounded_mul(y, y)), rounded_mul(z, z));
}

// ------------------------------------------------------------------------------------------------
// the bake's probes and directions (neb_gi_probe_rays, neb_gi_bake_probes, neb_gi_bake_visibility)
// ------------------------------------------------------------------------------------------------
// The interval the walk assumes: the triangle screen of intersect_tri_regs takes tmin >= 0 for granted, and an empty interval holds
// no hit.  Written so that a NaN on either side says no.
__device__ __forceinline__ bool interval_ok(float tmin, float tmax) { return tmin >= 0.0f && tmax > tmin; }

// Whether a probe is baked (include/nebulae_hip.h): a position whose squared length is finite -- ray_walkable's test of an origin, so
// that "not baked" and "no sample could be walked" are the same probes --, an interval in order (interval_ok: a NaN on either side says
// no) and, where the normal is used, one whose squared length is positive and finite.
template <uint32_t WHAT> __device__ __forceinline__ bool probe_baked(float4 p0, float4 p1)
{
    const float inf = __builtin_inff();
    bool ok = rounded_square_length(p0.x, p0.y, p0.z) < inf && interval_ok(p0.w, p1.w);
    if (WHAT == NEB_BAKE_IRRADIANCE) {
        const float nn = rounded_square_length(p1.x, p1.y, p1.z);
        ok = ok && nn > 0.0f && nn < inf;
    }
    return ok;
}

// The direction of sample s of S, ray index i = p * S + s: the sequence of include/nebulae_hip.h, one IEEE operation per line of it, under
// both shade policies.  Its two draws come from a stream of their own, so that they are independent of the path's.  `nrm` is
// normalize3<false>(normal) (IRRADIANCE; unused otherwise).
template <uint32_t WHAT> __device__ __forceinline__ float3 probe_direction(uint32_t i, uint32_t s, uint32_t samples, uint32_t frame_index, float3 nrm)
{
    uint32_t rng_d = jenkins(~i ^ jenkins(frame_index + 0x9E3779B9u));
    const float r0 = rand01(rng_d), r1 = rand01(rng_d);
    const float u0 = __fadd_rn((float)s, r0) / (float)samples, u1 = r1; // (one stratum of [0, 1] per sample in u0)
    if (WHAT == NEB_BAKE_IRRADIANCE)
        return cosine_hemisphere_aligned<false>(u0, u1, nrm);
    const float z = __fsub_rn(1.0f, rounded_mul(2.0f, u0));
    const float rho = sqrtf(fmaxf(0.0f, __fsub_rn(1.0f, rounded_mul(z, z)))); // (sqrtf and `/` are the correctly rounded forms in this build;
                                                                             //  __fsqrt_rn is ocml's native, 1-ulp root)
    float sn, cs;
    det_sincosf(rounded_mul(kPiTwo, u1), sn, cs);
    const float x = rounded_mul(rho, cs), y = rounded_mul(rho, sn);
    const float l = sqrtf(rounded_square_length(x, y, z)); // normalize3<false>, its roundings spelled out
    return f3(x / l, y / l, z / l);
}

// ------------------------------------------------------------------------------------------------
// the grid and the gather of one point (neb_gi_probe_grid, neb_gi_gather_probes, neb_gi_probe_indirect and their _visible forms)
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kGridMaxProbes = 1u << 24;

// Where probe k of an axis sits: the one product and the one sum of include/nebulae_hip.h.  neb_gi_probe_grid and the gather both call
// this, which is why a point copied from a probe has vv == 0 against it.
__device__ __forceinline__ float grid_coordinate(float origin, float spacing, uint32_t k) { return __fadd_rn(origin, rounded_mul((float)k, spacing)); }

constexpr float kY00 = 0.282095f, kY1 = 0.488603f, kY2a = 1.092548f, kY20 = 0.315392f, kY22 = 0.546274f; // the bake's basis constants
constexpr float kA0 = 3.14159265f, kA1 = 2.0943951f, kA2 = 0.78539816f;                                  // pi, 2 pi / 3, pi / 4

// What a point has of its own before any record is looked at.
struct GatherPoint {
    float3 p, N;
    uint32_t base[3];
    float f[3];
    uint32_t cell, flags;
};

// The visibility records of neb_gi_bake_visibility as the gather reads them: 96 float2 a probe, the first 64 the texels' moments.
constexpr uint32_t kVisibilityFloat2 = 96;

// A tap of the 8 x 8 octahedral map that may lie one texel outside it -> its texel's index.  Leaving the map across an edge enters it
// again across the same edge, mirrored about the edge's middle: the index on the axis that left is clamped, the other becomes 7 - b; x
// first, then y, so that a corner tap such as (-1, -1) lands on (7, 7).
__device__ __forceinline__ int oct_tap_index(int a, int b)
{
    if (a < 0 || a > 7) {
        a = min(max(a, 0), 7);
        b = 7 - b;
    }
    if (b < 0 || b > 7) {
        b = min(max(b, 0), 7);
        a = 7 - a;
    }
    return a + 8 * b;
}

// The Chebyshev factor of one corner (include/nebulae_hip.h, "VISIBLE GATHER"): u = the biased point minus the probe, `moments` the
// probe's 64 texels.  Four 8-byte loads a lane.  The clamp of tx and ty changes no number the contract can produce (|ox| + |oy| <= 1
// puts them in -0.5 .. 7.5); it keeps the taps inside the record for a lane that rides along with a position that is not finite.
__device__ __forceinline__ float corner_visibility(const float2* __restrict__ moments, float ux, float uy, float uz)
{
    const float rr = rounded_square_length(ux, uy, uz);
    if (rr == 0.0f)
        return 1.0f;
    const float r = sqrtf(rr);
    const float s = __fadd_rn(__fadd_rn(fabsf(ux), fabsf(uy)), fabsf(uz));
    float ox = ux / s, oy = uy / s;
    if (uz < 0.0f) {
        const float fx = rounded_mul(__fsub_rn(1.0f, fabsf(oy)), ox >= 0.0f ? 1.0f : -1.0f);
        const float fy = rounded_mul(__fsub_rn(1.0f, fabsf(ox)), oy >= 0.0f ? 1.0f : -1.0f);
        ox = fx, oy = fy;
    }
    const float tx = fminf(fmaxf(__fadd_rn(rounded_mul(ox, 4.0f), 3.5f), -0.5f), 7.5f);
    const float ty = fminf(fmaxf(__fadd_rn(rounded_mul(oy, 4.0f), 3.5f), -0.5f), 7.5f);
    const float flx = floorf(tx), fly = floorf(ty);
    const int ix = (int)flx, iy = (int)fly;
    const float fx = __fsub_rn(tx, flx), fy = __fsub_rn(ty, fly);
    const float2 t00 = moments[oct_tap_index(ix, iy)], t10 = moments[oct_tap_index(ix + 1, iy)];
    const float2 t01 = moments[oct_tap_index(ix, iy + 1)], t11 = moments[oct_tap_index(ix + 1, iy + 1)];
    const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
    const float m1 = __fadd_rn(rounded_mul(__fadd_rn(rounded_mul(gx, t00.x), rounded_mul(fx, t10.x)), gy),
                               rounded_mul(__fadd_rn(rounded_mul(gx, t01.x), rounded_mul(fx, t11.x)), fy));
    const float m2 = __fadd_rn(rounded_mul(__fadd_rn(rounded_mul(gx, t00.y), rounded_mul(fx, t10.y)), gy),
                               rounded_mul(__fadd_rn(rounded_mul(gx, t01.y), rounded_mul(fx, t11.y)), fy));
    // (the floor is relative: m2 - m1 m1 cancels to a few ulp of m2 where the variance is small, and 2^-10 m2 stays above that)
    const float var = fmaxf(__fsub_rn(m2, rounded_mul(m1, m1)), rounded_mul(0.0009765625f, m2));
    float cheb = 1.0f;
    if (r > m1) {
        const float over = __fsub_rn(r, m1);
        cheb = var / __fadd_rn(var, rounded_mul(over, over));
    }
    return fmaxf(0.05f, rounded_mul(rounded_mul(cheb, cheb), cheb));
}

// The blend of one point.  UNIFORM = true: every lane of the wave that gathers at all has the cell `cell`, which is then a scalar: the
// record addresses are the same for every lane, the loads are scalar loads, a cell's eight records are fetched once for the wave, and
// "is this corner valid" is a scalar branch.  UNIFORM = false: the lane's own cell, vector loads.  The arithmetic is the same text.
// Two passes: the counters of the eight corners (each record's last 32-byte sector) give the weights and their sum; then the first
// seven float4 of the corners that count are blended with w / W.
// VISIBLE = true (neb_gi_gather_probes_visible): a valid corner's weight takes corner_visibility as one more factor, from the probe's
// record in `visibility` and the point moved by normal_bias along its normal; the per-lane taps go out from a scalar base under UNIFORM.
template <bool UNIFORM, bool VISIBLE = false>
__device__ __forceinline__ void gather_blend(const neb_probe_grid& G, const float4* __restrict__ records, const GatherPoint& P, uint32_t cell, float3& E,
                                             float& W, uint32_t& corners, const float2* __restrict__ visibility = nullptr, float normal_bias = 0.0f)
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
            if constexpr (VISIBLE) {
                const float ux = __fsub_rn(__fadd_rn(P.p.x, rounded_mul(normal_bias, P.N.x)), grid_coordinate(G.origin[0], G.spacing[0], P.base[0] + cx));
                const float uy = __fsub_rn(__fadd_rn(P.p.y, rounded_mul(normal_bias, P.N.y)), grid_coordinate(G.origin[1], G.spacing[1], P.base[1] + cy));
                const float uz = __fsub_rn(__fadd_rn(P.p.z, rounded_mul(normal_bias, P.N.z)), grid_coordinate(G.origin[2], G.spacing[2], P.base[2] + cz));
                const float vis = corner_visibility(visibility + kVisibilityFloat2 * probe, ux, uy, uz);
                w[c] = rounded_mul(w[c], vis);
                // A corner that is seen whole (vis == 1, w unchanged) enters W as the plain arm's does.  There the back end fuses the
                // product into the sum below (v_fma_f32 in probe_gather_kernel's text: W takes w_tri * w_n unrounded, an ulp from the
                // header's sum now and then), and only the same operation gives neb_gi_gather_probes' bits where nothing is hidden.
                W = vis == 1.0f ? __fmaf_rn(w_tri, w_n, W) : __fadd_rn(W, w[c]);
            } else
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
// p0 = {position, -}, p1 = {normal, -}; `live`: the lane has a point at all.  Every gather kernel calls this, so a pixel's point is
// located by the operations a point read from a buffer is.
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
template <bool VISIBLE = false>
__device__ __forceinline__ void gather_wave(const neb_probe_grid& G, const float4* __restrict__ records, const GatherPoint& P, bool usable, float3& E, float& W,
                                            uint32_t& corners, const float2* __restrict__ visibility = nullptr, float normal_bias = 0.0f)
{
    E = f3(0.0f, 0.0f, 0.0f);
    W = 0.0f;
    corners = 0u;
    const unsigned long long gathering = __ballot(usable);
    if (gathering != 0ull) {
        const uint32_t leader = (uint32_t)__ffsll(gathering) - 1u;
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)P.cell, (int)leader);
        if (__ballot(usable && P.cell != first) == 0ull)
            gather_blend<true, VISIBLE>(G, records, P, first, E, W, corners, visibility, normal_bias);
        else if (usable)
            gather_blend<false, VISIBLE>(G, records, P, P.cell, E, W, corners, visibility, normal_bias);
    }
}

// ------------------------------------------------------------------------------------------------
// a frame's pixels as the gather's points
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

struct IndirectArgs {
    neb_probe_grid G;
    FramePlanes F;
    float camera[3];
    uint32_t row_begin, row0, row1, tiles_x, n_tiles, frame_weight;
};

// What the fused passes do with a gathered pixel i whose point is (p0, p1): the irradiance E weighted as the frame's diffuse term and
// added to the pixel's radiance (include/nebulae_hip.h, "INDIRECT TERM").
__device__ __forceinline__ void add_indirect_term(const IndirectArgs& a, size_t i, const float4& p0, const float4& p1, float3 E, float4* __restrict__ radiance)
{
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
