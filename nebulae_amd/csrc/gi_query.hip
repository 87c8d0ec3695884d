// gi_query.hip -- the caller's own rays against the scene the context holds: neb_gi_cast_rays and neb_gi_shade_rays
// (3.8a), which walks the same way and then shades the hit as the frame's shade pass would.
//
// Rays and answers live in device buffers of the caller.  One lane per ray walks the tree the frame's kernels walk, with the
// traverser they use (traverse, gi_device.h: same boxes, same triangle test, same barycentrics), closest hit or first hit; with
// NEB_RAYS_SORT the rays are visited in the order of a 16-bit key (direction octant above the origin's Morton bits, bounce_sort_key)
// and every answer still lands at its ray's own index.  A ray's walk depends on the ray and the tree alone, so the order changes
// no answer.  Nothing of the frame is touched: no plane, no ray counter, no statistics, no sun table.
#include "probe_device.h" // (the shared probe arithmetic; turns floating-point contraction off for this file: see gi_device.h)

namespace neb {

namespace {

constexpr uint32_t kQueryMaxRays = 1u << 28; // 8 GiB of rays; the sort's indices and raysort.hip's tile counts stay far inside 32 bits
constexpr uint32_t kNoId = 0xffffffffu;
constexpr uint32_t kUnwalkableKey = (1u << kSortBits) - 1u; // above every key of bounce_sort_key: such rays gather at the end

// One lane per ray, one wave per workgroup, the LDS stack of gbuffer_kernel.  Lane j takes ray j, or ray order[j] (SORTED), reads it
// as two float4 and writes its answer AT THE RAY'S OWN INDEX: a hit record as two 16-byte stores of one 32-byte sector (ANY_HIT =
// false), or one word, 1 = something lies in (tmin, tmax) (ANY_HIT = true).
// A ray that cannot be walked reports a miss without entering the tree: traverse_t keeps a zero or non-finite direction and a
// non-finite origin out (its `walkable`), and a ray whose interval is not in order is handed to it with a zero direction.
template <bool ANY_HIT, bool SORTED>
__global__ __launch_bounds__(64) void ray_query_kernel(SceneView S, const float4* __restrict__ rays, uint32_t n, const uint32_t* __restrict__ order,
                                                       void* __restrict__ out)
{
    __shared__ int stack_mem[kLdsStack * 64];
    const uint32_t lane = threadIdx.x;
    int* stack = stack_mem + lane;
    const uint32_t j = blockIdx.x * 64u + lane;
    if (j >= n)
        return;
    const uint32_t i = SORTED ? order[j] : j;
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1]; // {origin, tmin} {direction, tmax}
    const float tmin = r0.w, tmax = r1.w;
    const float3 o = f3(r0.x, r0.y, r0.z);
    const float3 d = interval_ok(tmin, tmax) ? f3(r1.x, r1.y, r1.z) : f3(0.0f, 0.0f, 0.0f);
    Hit h;
    const bool found = traverse(S, o, d, tmin, tmax, ANY_HIT, stack, h);
    if constexpr (ANY_HIT) {
        static_cast<uint32_t*>(out)[i] = found ? 1u : 0u;
    } else {
        float4 a = make_float4(__builtin_inff(), 0.0f, 0.0f, __uint_as_float(kNoId)); // {t, u, v, geometry}
        uint4 b = make_uint4(kNoId, 0u, 0u, 0u);                                      // {primitive, reserved x 3}
        if (found) {
            const float4 ids = S.tris[3 * h.tri + 2]; // {e2.z, geometry, primitive, -}
            a = make_float4(h.t, h.u, h.v, ids.y);
            b.x = __float_as_uint(ids.z);
        }
        float4* rec = static_cast<float4*>(out) + 2 * (size_t)i;
        rec[0] = a;
        *reinterpret_cast<uint4*>(rec + 1) = b;
    }
}

// ------------------------------------------------------------------------------------------------
// neb_gi_shade_rays: the walk above, then the surface at the hit (NEB_SHADE_SURFACE) or what the frame's path adds there (NEB_SHADE_RADIANCE)
// ------------------------------------------------------------------------------------------------
// What the RADIANCE kernel reads of the constants: the sun frame of the dispatch (sun_frame, on the host, as neb_gi_trace), the
// radiances and the seed of the disk draws.
static_assert(sizeof(neb_ray_surface) == 96 && offsetof(neb_ray_surface, flags) == 88 && sizeof(neb_ray_radiance) == 32, "records of neb_gi_shade_rays");
struct ShadeSun {
    float L[3], B[3], T[3];
    float radiance[3], sky[3];
    float tan_half;
    uint32_t frame_index;
};

// traverse_t's guard and interval_ok in one: the rays ray_query_key_kernel gives the largest key.  (The walk kernels need not ask --
// the traverser refuses such a ray by itself -- but the shade kernel has to tell "not walked" from "walked and missed".)
__device__ __forceinline__ bool ray_walkable(float3 o, float3 d, float tmin, float tmax)
{
    const float dd = dot3(d, d), oo = dot3(o, o);
    return dd > 0.0f && dd < __builtin_inff() && oo < __builtin_inff() && interval_ok(tmin, tmax);
}

// ray_query_kernel's shape: one lane per ray, one wave per workgroup, its LDS stack; lane j takes ray j or order[j] and answers at
// the ray's own index with 16-byte stores, six for a neb_ray_surface, two for a neb_ray_radiance.  After the closest-hit walk a lane
// that hit loads the triangle's shading record and its geometry's shade header -- the two lines the shade pass reads for that hit --
// and runs the halves of reconstruct_surface<FAST> on them.  RADIANCE then builds shade_pixel's sun-disk shadow ray (its exact-
// arithmetic sequence under both policies) and walks it any-hit on the same stack; a lane that has no shadow ray hands the traverser
// a zero direction, which it refuses without entering the tree.  The BRDF runs where the walk found nothing.
template <uint32_t WHAT, bool SORTED, bool FAST>
__global__ __launch_bounds__(64) void ray_shade_kernel(SceneView S, const ShadeHeader* __restrict__ heads, const float4* __restrict__ rays, uint32_t n,
                                                       const uint32_t* __restrict__ order, ShadeSun sun, float4* __restrict__ out)
{
    __shared__ int stack_mem[kLdsStack * 64];
    const uint32_t lane = threadIdx.x;
    int* stack = stack_mem + lane;
    const uint32_t j = blockIdx.x * 64u + lane;
    if (j >= n)
        return;
    const uint32_t i = SORTED ? order[j] : j;
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1]; // {origin, tmin} {direction, tmax}
    const float tmin = r0.w, tmax = r1.w;
    const float3 o = f3(r0.x, r0.y, r0.z), dir = f3(r1.x, r1.y, r1.z);
    const bool walked = ray_walkable(o, dir, tmin, tmax);
    Hit h;
    const bool found = traverse(S, o, walked ? dir : f3(0.0f, 0.0f, 0.0f), tmin, tmax, false, stack, h);

    uint32_t flags = walked ? 0u : (uint32_t)NEB_HIT_NOT_WALKED;
    float t = __builtin_inff(), bu = 0.0f, bv = 0.0f, tex_u = 0.0f, tex_v = 0.0f;
    uint32_t geometry = kNoId, primitive = kNoId;
    int32_t material = -1;
    float3 hitP = f3(0.0f, 0.0f, 0.0f);
    Surface surf;
    surf.GN = surf.SN = surf.albedo = f3(0.0f, 0.0f, 0.0f);
    surf.roughness = surf.metalness = 0.0f;
    if (found) {
        const float4 ids = S.tris[3 * h.tri + 2]; // {e2.z, geometry, primitive, -}: the words neb_gi_cast_rays reports
        const TriShade ts = load_tri_shade(S, h.tri);
        const ShadeHead head = load_shade_header(heads, ts.geom);
        t = h.t, bu = h.u, bv = h.v;
        geometry = __float_as_uint(ids.y), primitive = __float_as_uint(ids.z);
        hitP = o + dir * h.t;
        flags |= NEB_HIT_FOUND;
        // reconstruct_surface, its two halves called as it calls them: the uv between them is part of the record
        const bool shaded = reconstruct_geometry<FAST>(head, ts, h.u, h.v, surf, tex_u, tex_v);
        if (head.valid) {
            flags |= NEB_HIT_ATTRIBUTES | (dot3(surf.GN, dir) > 0.0f ? (uint32_t)NEB_HIT_BACKFACE : 0u);
            surf.SN = surf.GN; // (a geometry without a material; the material half replaces it)
        }
        if (shaded) {
            MapSamples maps;
            sample_material_maps<FAST>(S, head.mat, tex_u, tex_v, maps);
            reconstruct_material<FAST>(head.mat, ts, h.u, h.v, maps, surf);
            flags |= NEB_HIT_MATERIAL;
            material = head.material;
        }
    }
    if constexpr (WHAT == NEB_SHADE_SURFACE) {
        float4* rec = out + 6 * (size_t)i;
        rec[0] = make_float4(hitP.x, hitP.y, hitP.z, t);
        rec[1] = make_float4(surf.GN.x, surf.GN.y, surf.GN.z, __uint_as_float(geometry));
        rec[2] = make_float4(surf.SN.x, surf.SN.y, surf.SN.z, __uint_as_float(primitive));
        rec[3] = make_float4(surf.albedo.x, surf.albedo.y, surf.albedo.z, surf.roughness);
        rec[4] = make_float4(surf.metalness, tex_u, tex_v, __uint_as_float((uint32_t)material));
        rec[5] = make_float4(bu, bv, __uint_as_float(flags), 0.0f);
    } else {
        const bool shaded = (flags & NEB_HIT_MATERIAL) != 0;
        // shade_pixel's shadow ray (gi.hip; pathtracer.hlsl:546-557), the draws seeded by the ray's index in the caller's array
        uint32_t rng = jenkins(i ^ jenkins(sun.frame_index));
        const float a0 = rand01(rng), a1 = rand01(rng);
        const float angle = a0 * 2.0f * 3.1415926535f, dist = fsqrt<false>(a1);
        const float3 L = f3(sun.L[0], sun.L[1], sun.L[2]), Bv = f3(sun.B[0], sun.B[1], sun.B[2]), T = f3(sun.T[0], sun.T[1], sun.T[2]);
        float sn_a, cs_a;
        det_sincosf(angle, sn_a, cs_a);
        const float3 inc = normalize3<false>(L + (Bv * sn_a + T * cs_a) * sun.tan_half * dist);
        const bool transition = dot3(surf.GN, inc) <= 0.0f;
        const float3 so = hitP + (transition ? -surf.GN : surf.GN) * 1e-2f;
        Hit sh;
        const bool occluded = traverse(S, so, shaded ? inc : f3(0.0f, 0.0f, 0.0f), 0.001f, kTraceMax, true, stack, sh);
        float3 rgb = f3(0.0f, 0.0f, 0.0f);
        if (walked && !found)
            rgb = f3(sun.sky[0], sun.sky[1], sun.sky[2]); // :508
        if (shaded && !occluded) {
            const float3 V = normalize3<FAST>(-dir); // :522
            rgb = evaluate_direct_brdf<FAST>(surf, V, L) * f3(sun.radiance[0], sun.radiance[1], sun.radiance[2]); // :573-574
            flags |= NEB_HIT_SUN_VISIBLE;
        }
        float4* rec = out + 2 * (size_t)i;
        rec[0] = make_float4(rgb.x, rgb.y, rgb.z, t);
        rec[1] = make_float4(__uint_as_float(geometry), __uint_as_float(primitive), __uint_as_float(flags), 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------
// neb_gi_trace_paths: the frame's bounce loop (shade_pixel, gi.hip; pathtracer.hlsl:495-621) along the caller's ray
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(neb_ray_path) == 32 && offsetof(neb_ray_path, segments) == 28 && sizeof(neb_path_vertex) == 96 && offsetof(neb_path_vertex, tmax) == 80,
              "records of neb_gi_trace_paths");

// ray_shade_kernel's shape -- one lane per ray, one wave per workgroup, its LDS stack, the answer at the ray's own index in 16-byte
// stores -- with the segment loop inside: per segment k = 1 .. max_vertices - 1 the closest-hit walk, RADIANCE's reconstruction and
// shadow ray, and shade_pixel's next bounce (the draws of EvaluateIndirectBRDF from a copy of the stream, the throughput rule of
// :613-618).  Both walks of an iteration are entered by the whole wave: a lane whose path has ended hands the traverser a zero
// direction, which it refuses without entering the tree, and the loop is left when no lane of the wave is alive.  Vertex 1 ASSIGNS the
// sum and later vertices add to it, so that with max_vertices = 2 the record is NEB_SHADE_RADIANCE's, bit for bit.
// VERTICES: record i * (max_vertices - 1) + (k - 1) describes segment k of ray i, six 16-byte stores; a record past the path's end is
// written as zeroes.
// The loop itself is path_segments.h, one text that probe_bake_kernel (below) includes too.
// TAIL (neb_gi_trace_paths_tail): 0 = none, the kernel of neb_gi_trace_paths; 1 / 2 = the path's last vertex ends in the
// probe grid of `tail`, gathered plain / with visibility after the loop.  The grid arrives as a parameter pack of one TailArgs, which is
// empty for TAIL = 0: that kernel's signature, and with it its kernel arguments, are neb_gi_trace_paths' own.
struct TailArgs { // neb_probe_tail as the kernels read it
    neb_probe_grid G;
    const float4* records;
    const float2* visibility;
    float normal_bias;
    uint32_t frame_weight;
};
struct NoTail {};
__device__ __forceinline__ NoTail the_tail() { return NoTail{}; }
__device__ __forceinline__ const TailArgs& the_tail(const TailArgs& t) { return t; }

template <bool SORTED, bool FAST, bool VERTICES, int TAIL = 0, typename... Tail>
__global__ __launch_bounds__(64) void ray_path_kernel(SceneView S, const ShadeHeader* __restrict__ heads, const float4* __restrict__ rays, uint32_t n,
                                                      const uint32_t* __restrict__ order, ShadeSun sun, uint32_t max_vertices, float4* __restrict__ out,
                                                      float4* __restrict__ vertices, Tail... tail_pack)
{
    static_assert(sizeof...(Tail) == (TAIL != 0), "one TailArgs exactly where TAIL is set");
    [[maybe_unused]] const auto& tail = the_tail(tail_pack...);
    __shared__ int stack_mem[kLdsStack * 64];
    const uint32_t lane = threadIdx.x;
    int* stack = stack_mem + lane;
    const uint32_t j = blockIdx.x * 64u + lane;
    if (j >= n)
        return;
    const uint32_t i = SORTED ? order[j] : j;
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1]; // {origin, tmin} {direction, tmax}
    float tmin = r0.w, tmax = r1.w;
    float3 o = f3(r0.x, r0.y, r0.z), dir = f3(r1.x, r1.y, r1.z);
    const float3 L = f3(sun.L[0], sun.L[1], sun.L[2]), Bv = f3(sun.B[0], sun.B[1], sun.B[2]), T = f3(sun.T[0], sun.T[1], sun.T[2]);
    const uint32_t last = max_vertices - 1u; // segments a path can have
    float4* vrec = VERTICES ? vertices + 6 * ((size_t)i * last) : nullptr;

#include "path_segments.h" // -> sum, first_t, first_geometry, first_primitive, path_flags, segments
    float4* rec = out + 2 * (size_t)i;
    rec[0] = make_float4(sum.x, sum.y, sum.z, first_t);
    rec[1] = make_float4(__uint_as_float(first_geometry), __uint_as_float(first_primitive), __uint_as_float(path_flags), __uint_as_float(segments));
}

// ------------------------------------------------------------------------------------------------
// neb_gi_probe_rays / neb_gi_bake_probes: S path samples per probe, generated, followed and reduced on the device
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(neb_probe) == 32 && sizeof(neb_probe_record) == 128 && offsetof(neb_probe_record, samples) == 108 && offsetof(neb_probe_record, flags) == 124,
              "records of neb_gi_bake_probes");
constexpr uint32_t kProbeMaxSamples = 4096;
// Waves per SIMD asked of probe_bake_kernel: ray_path_kernel's five under the default policy, four under the exact one.
// -DNEB_PROBE_BAKE_FOUR_WAVES holds every instantiation to four: the A/B arm of DESIGN.md 3.8c's table, not a product build.
#ifdef NEB_PROBE_BAKE_FOUR_WAVES
#define NEB_PROBE_BAKE_OCCUPANCY amdgpu_waves_per_eu(4, 4)
#else
#define NEB_PROBE_BAKE_OCCUPANCY amdgpu_waves_per_eu(TAIL ? 4 : FAST ? 5 : 4)
#endif

// One lane per ray: ray p * S + s is sample s of probe p, origin and interval the probe's own bits; a probe that is not baked gets S
// rays of zeroes, which every query reports as NEB_HIT_NOT_WALKED.
template <uint32_t WHAT>
__global__ __launch_bounds__(256) void probe_rays_kernel(const float4* __restrict__ probes, uint32_t n_rays, uint32_t samples, uint32_t frame_index,
                                                         float4* __restrict__ rays)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rays)
        return;
    const uint32_t p = i / samples, s = i - p * samples;
    const float4 p0 = probes[2 * (size_t)p], p1 = probes[2 * (size_t)p + 1]; // {position, tmin} {normal, tmax}
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (probe_baked<WHAT>(p0, p1)) {
        const float3 nrm = WHAT == NEB_BAKE_IRRADIANCE ? normalize3<false>(f3(p1.x, p1.y, p1.z)) : f3(0.0f, 0.0f, 0.0f);
        const float3 d = probe_direction<WHAT>(i, s, samples, frame_index, nrm);
        a = p0;
        b = make_float4(d.x, d.y, d.z, p1.w);
    }
    rays[2 * (size_t)i] = a;
    rays[2 * (size_t)i + 1] = b;
}

// One wave per probe, one wave per workgroup, ray_path_kernel's LDS stack.  Round r = 0 .. S / 64 - 1 gives lane l sample s = 64 r + l:
// the lane builds the sample's direction (probe_direction), follows ray_path_kernel's path for ray index p * S + s (path_segments.h,
// the same text) and forms its words L.c * Y_lm(d) -- 27 under NEB_BAKE_SH, the three L.c under NEB_BAKE_IRRADIANCE.  A butterfly over
// the lane masks 32, 16, 8, 4, 2, 1 (v = v + v[lane ^ m]: both partners add the same two numbers, so every lane ends with the same sum)
// reduces each word over the wave, and lane 0 adds the round's sums to the running totals IN ROUND ORDER.  The totals live in 128 bytes
// of LDS, not in registers: they are no loop-carried state of the segment loop.  The counters are ballots and popcounts of the round,
// which lane 0 adds to the record's words in LDS as well.  After the last round lane 0 multiplies the totals once by `scale` and lanes 0..7 write the record, one 16-byte store
// each.  Every multiplication and addition of the projection is written with its rounding (no fused multiply-add anywhere in it).
// A probe that is not baked costs one test and the same eight stores.
// TAIL (neb_gi_bake_probes_tail): ray_path_kernel's.  All 64 lanes of the wave are in every round, so the round's gather is converged.
template <uint32_t WHAT, bool FAST, int TAIL = 0, typename... Tail>
__global__ __launch_bounds__(64) __attribute__((NEB_PROBE_BAKE_OCCUPANCY)) void probe_bake_kernel(
    SceneView S, const ShadeHeader* __restrict__ heads, const float4* __restrict__ probes, uint32_t samples, ShadeSun sun, uint32_t max_vertices, float scale,
    float4* __restrict__ out, Tail... tail_pack)
{
    static_assert(sizeof...(Tail) == (TAIL != 0), "one TailArgs exactly where TAIL is set");
    [[maybe_unused]] const auto& tail = the_tail(tail_pack...);
    constexpr bool VERTICES = false;
    constexpr int kWords = WHAT == NEB_BAKE_SH ? 27 : 3;
    __shared__ int stack_mem[kLdsStack * 64];
    __shared__ float4 record[8]; // the probe's record: the running totals in words 0 .. 26
    float* total = reinterpret_cast<float*>(record);
    const uint32_t lane = threadIdx.x;
    int* stack = stack_mem + lane;
    const uint32_t p = blockIdx.x;
    const float4 p0 = probes[2 * (size_t)p], p1 = probes[2 * (size_t)p + 1]; // {position, tmin} {normal, tmax}: the same for every lane
    float4* rec = out + 8 * (size_t)p;
    // (the same for every lane: read as a scalar, so that the branch is one and no execution mask is kept through the kernel)
    if (!__builtin_amdgcn_readfirstlane((int)probe_baked<WHAT>(p0, p1))) {
        if (lane < 8u)
            rec[lane] = make_float4(0.0f, 0.0f, 0.0f, lane == 7u ? __uint_as_float(NEB_PROBE_NOT_BAKED) : 0.0f);
        return;
    }
    if (lane < 32u)
        total[lane] = 0.0f;
    __syncthreads(); // (one wave: orders these writes before lane 0's additions)
    uint32_t* const counter = reinterpret_cast<uint32_t*>(record) + 28; // hits, backfaces, segments: lane 0 adds to them too
    const float3 L = f3(sun.L[0], sun.L[1], sun.L[2]), Bv = f3(sun.B[0], sun.B[1], sun.B[2]), T = f3(sun.T[0], sun.T[1], sun.T[2]);
    const uint32_t last = max_vertices - 1u; // segments a path can have
    float4* const vrec = nullptr;
    for (uint32_t round = 0u; round < samples / 64u; ++round) {
        // The probe again, two scalar loads per round, so that its eight words are not carried through the segment loop in scalar
        // registers the kernel does not have.  (The empty statement keeps the compiler from hoisting the loads.)
        const float4* probe = probes + 2 * (size_t)p;
        asm volatile("" : "+s"(probe));
        const float4 q0 = probe[0], q1 = probe[1];
        const uint32_t s = 64u * round + lane, i = p * samples + s;
        const float3 nrm = WHAT == NEB_BAKE_IRRADIANCE ? normalize3<false>(f3(q1.x, q1.y, q1.z)) : f3(0.0f, 0.0f, 0.0f);
        float tmin = q0.w, tmax = q1.w;
        float3 o = f3(q0.x, q0.y, q0.z), dir = probe_direction<WHAT>(i, s, samples, sun.frame_index, nrm);
#include "path_segments.h" // -> sum, first_t, first_geometry, first_primitive, path_flags, segments
        (void)first_t, (void)first_geometry, (void)first_primitive;
        float w[kWords];
        if constexpr (WHAT == NEB_BAKE_SH) {
            // The direction again, from the lane's number alone: three registers fewer to carry through the segment loop.  (The empty
            // statement keeps the compiler from seeing that it is the value it had before the loop.)
            uint32_t s2 = 64u * round + lane;
            asm volatile("" : "+v"(s2));
            const float3 d = probe_direction<WHAT>(p * samples + s2, s2, samples, sun.frame_index, nrm);
            float Y[9]; // the real basis, (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2)
            Y[0] = 0.282095f;
            Y[1] = __fmul_rn(0.488603f, d.y);
            Y[2] = __fmul_rn(0.488603f, d.z);
            Y[3] = __fmul_rn(0.488603f, d.x);
            Y[4] = __fmul_rn(1.092548f, __fmul_rn(d.x, d.y));
            Y[5] = __fmul_rn(1.092548f, __fmul_rn(d.y, d.z));
            Y[6] = __fmul_rn(0.315392f, __fsub_rn(rounded_mul(__fmul_rn(3.0f, d.z), d.z), 1.0f));
            Y[7] = __fmul_rn(1.092548f, __fmul_rn(d.x, d.z));
            Y[8] = __fmul_rn(0.546274f, __fsub_rn(rounded_mul(d.x, d.x), rounded_mul(d.y, d.y)));
#pragma unroll
            for (int q = 0; q < 9; ++q) { // (rounded before the butterfly adds them)
                w[3 * q] = rounded_mul(sum.x, Y[q]);
                w[3 * q + 1] = rounded_mul(sum.y, Y[q]);
                w[3 * q + 2] = rounded_mul(sum.z, Y[q]);
            }
        } else {
            w[0] = sum.x, w[1] = sum.y, w[2] = sum.z;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < kWords; ++q)
                w[q] = __fadd_rn(w[q], __shfl_xor(w[q], m, 64));
        const bool hit = (path_flags & NEB_HIT_FOUND) != 0u;
        const uint32_t round_hits = (uint32_t)__popcll(__ballot(hit)), round_backfaces = (uint32_t)__popcll(__ballot(hit && (path_flags & NEB_HIT_BACKFACE) != 0u));
        const uint32_t round_segments = (uint32_t)__popcll(__ballot((segments & 1u) != 0u)) + 2u * (uint32_t)__popcll(__ballot((segments & 2u) != 0u))
                                        + 4u * (uint32_t)__popcll(__ballot((segments & 4u) != 0u)); // (segments <= 7)
        if (lane == 0u) {
#pragma unroll
            for (int q = 0; q < kWords; ++q)
                total[q] = __fadd_rn(total[q], w[q]);
            counter[0] += round_hits, counter[1] += round_backfaces, counter[2] += round_segments;
        }
    }
    if (lane == 0u) {
#pragma unroll
        for (int q = 0; q < kWords; ++q)
            total[q] = __fmul_rn(total[q], scale);
        counter[-1] = samples;
    }
    __syncthreads(); // (one wave: orders lane 0's LDS writes before the other lanes' reads)
    if (lane < 8u)
        rec[lane] = record[lane];
}

struct QueryBox {
    float smin[3], sinv[3]; // the scene box the dispatches sort by (neb_gi_trace)
};

// One lane per ray: (key, index) for ray_sort_pairs.  Rays the walk kernel will not walk get the largest key.
__global__ __launch_bounds__(256) void ray_query_key_kernel(const float4* __restrict__ rays, uint32_t n, QueryBox box, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    const float3 o = f3(r0.x, r0.y, r0.z), d = f3(r1.x, r1.y, r1.z);
    const float dd = dot3(d, d), oo = dot3(o, o);
    const bool walkable = dd > 0.0f && dd < __builtin_inff() && oo < __builtin_inff() && interval_ok(r0.w, r1.w); // (traverse_t's guard)
    keys[i] = walkable ? bounce_sort_key(o, d, box.smin, box.sinv) : kUnwalkableKey;
    vals[i] = i;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// The sort block of a call of n rays, ordered behind the sorted call before it (GiState::d_query_sort).  Only a call larger than any
// before it gets past the first test: it waits for the last sorted call on the host, frees and allocates.
hipError_t query_sort_block(GiState* g, size_t bytes, hipStream_t stream)
{
    if (!g->query_ev)
        if (hipError_t e = hipEventCreateWithFlags(&g->query_ev, hipEventDisableTiming); e != hipSuccess)
            return e;
    if (bytes > g->query_sort_cap) {
        if (g->query_ev_pending)
            if (hipError_t e = hipEventSynchronize(g->query_ev); e != hipSuccess)
                return e;
        g->query_ev_pending = false;
        if (g->d_query_sort)
            (void)hipFree(g->d_query_sort);
        g->d_query_sort = nullptr;
        g->query_sort_cap = 0;
        if (hipError_t e = hipMalloc(&g->d_query_sort, bytes); e != hipSuccess)
            return e;
        g->query_sort_cap = bytes;
    } else if (g->query_ev_pending && g->query_stream != stream) {
        if (hipError_t e = hipStreamWaitEvent(stream, g->query_ev, 0); e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The walk order of a sorted call into the block query_sort_block has made room for: keys, the radix sort -> the sorted indices.
hipError_t enqueue_ray_order(GiState* g, const float4* r4, uint32_t n, hipStream_t stream, const uint32_t*& order)
{
    uint32_t* keys = static_cast<uint32_t*>(g->d_query_sort);
    uint32_t *vals = keys + n, *keys_tmp = keys + 2 * (size_t)n, *vals_tmp = keys + 3 * (size_t)n;
    QueryBox box;
    for (int q = 0; q < 3; ++q) {
        box.smin[q] = g->scene_min[q];
        box.sinv[q] = 1.0f / fmaxf(g->scene_max[q] - g->scene_min[q], 1e-20f);
    }
    hipLaunchKernelGGL(ray_query_key_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, r4, n, box, keys, vals);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (hipError_t e = ray_sort_pairs(keys, vals, keys_tmp, vals_tmp, vals, n, kSortBits, keys + 4 * (size_t)n, stream); e != hipSuccess)
        return e;
    order = vals;
    return hipSuccess;
}

size_t query_sort_bytes(uint32_t n) { return 4 * (size_t)n * sizeof(uint32_t) + ray_sort_scratch_bytes(n); }

} // namespace

} // namespace neb

using namespace neb;

extern "C" int neb_gi_cast_rays(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, void* out, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_cast_rays: scene/BVH not ready");
    if (flags & ~(NEB_RAYS_ANY_HIT | NEB_RAYS_SORT))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: unknown flag bits");
    if (n == 0)
        return NEB_OK;
    if (n > kQueryMaxRays)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_cast_rays: more than 2^28 rays in one call");
    const bool any_hit = (flags & NEB_RAYS_ANY_HIT) != 0, sorted = (flags & NEB_RAYS_SORT) != 0;
    const size_t ray_bytes = (size_t)n * sizeof(neb_ray), out_bytes = (size_t)n * (any_hit ? sizeof(uint32_t) : sizeof(neb_ray_hit));
    if (!rays || !out)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: null rays or out");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)out & (any_hit ? 3u : 31u)))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: misaligned pointer (rays: 16 bytes; out: 32 bytes for hit records, 4 for any-hit words)");
    if (ranges_overlap(rays, ray_bytes, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: out overlaps rays");
    GI_GUARD(ctx);
    if (!device_readable(ctx, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: rays is not memory this context's device reads, or n rays leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_cast_rays: out is not memory this context's device reads, or n answers leave its allocation");
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t* order = nullptr;
    if (sorted) { // (before anything is enqueued: a failed allocation leaves the stream as it was)
        GI_HIP(ctx, query_sort_block(g, query_sort_bytes(n), stream));
    }
    GI_HIP(ctx, gi_scene_reader(g, stream)); // behind any update enqueued on another stream; a later update waits for this stream
    const float4* r4 = reinterpret_cast<const float4*>(rays);
    auto enqueue = [&]() -> hipError_t {
        if (sorted)
            if (hipError_t e = enqueue_ray_order(g, r4, n, stream, order); e != hipSuccess)
                return e;
        const dim3 grid((n + 63u) / 64u), block(64);
        if (any_hit) {
            if (sorted)
                hipLaunchKernelGGL((ray_query_kernel<true, true>), grid, block, 0, stream, g->view, r4, n, order, out);
            else
                hipLaunchKernelGGL((ray_query_kernel<true, false>), grid, block, 0, stream, g->view, r4, n, order, out);
        } else {
            if (sorted)
                hipLaunchKernelGGL((ray_query_kernel<false, true>), grid, block, 0, stream, g->view, r4, n, order, out);
            else
                hipLaunchKernelGGL((ray_query_kernel<false, false>), grid, block, 0, stream, g->view, r4, n, order, out);
        }
        return hipGetLastError();
    };
    const hipError_t launched = enqueue();
    if (sorted) { // (also behind a chain that broke off half way: whatever of it was enqueued uses the block)
        GI_HIP(ctx, hipEventRecord(g->query_ev, stream));
        g->query_stream = stream;
        g->query_ev_pending = true;
    }
    GI_HIP(ctx, launched);
    return NEB_OK;
}

extern "C" int neb_gi_shade_rays(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t what, uint32_t flags, const neb_gi_constants* constants, void* out,
                                 neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_shade_rays: scene/BVH not ready");
    if (what != NEB_SHADE_SURFACE && what != NEB_SHADE_RADIANCE)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: unknown `what` (NEB_SHADE_SURFACE or NEB_SHADE_RADIANCE)");
    if (flags & ~NEB_RAYS_SORT)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, flags & NEB_RAYS_ANY_HIT ? "neb_gi_shade_rays: NEB_RAYS_ANY_HIT is not a flag of this call (a first hit has no surface to report)"
                                                                          : "neb_gi_shade_rays: unknown flag bits");
    const bool radiance = what == NEB_SHADE_RADIANCE, sorted = (flags & NEB_RAYS_SORT) != 0;
    if (n == 0)
        return NEB_OK;
    if (n > kQueryMaxRays)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_shade_rays: more than 2^28 rays in one call");
    if (radiance && !constants)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: NEB_SHADE_RADIANCE needs constants (null)");
    const size_t ray_bytes = (size_t)n * sizeof(neb_ray), out_bytes = (size_t)n * (radiance ? sizeof(neb_ray_radiance) : sizeof(neb_ray_surface));
    if (!rays || !out)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: null rays or out");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)out & 31u))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: misaligned pointer (rays: 16 bytes; out: 32 bytes)");
    if (ranges_overlap(rays, ray_bytes, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: out overlaps rays");
    GI_GUARD(ctx);
    if (!device_readable(ctx, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: rays is not memory this context's device reads, or n rays leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_shade_rays: out is not memory this context's device reads, or n records leave its allocation");
    hipStream_t stream = (hipStream_t)stream_;
    ShadeSun sun = {};
    if (radiance) { // (neb_gi_trace refuses no value of the sun fields, so none is refused here: they act as they act on the frame)
        sun_frame(constants->sunLightDirection, sun.L, sun.B, sun.T);
        for (int q = 0; q < 3; ++q) {
            sun.radiance[q] = constants->sunLightRadiance[q];
            sun.sky[q] = constants->skyColor[q];
        }
        sun.tan_half = constants->sunTanHalfAngle;
        sun.frame_index = constants->frameIndex;
    }
    if (sorted) // (before anything is enqueued: a failed allocation leaves the stream as it was)
        GI_HIP(ctx, query_sort_block(g, query_sort_bytes(n), stream));
    GI_HIP(ctx, gi_scene_reader(g, stream)); // behind any update enqueued on another stream; a later update waits for this stream
    const float4* r4 = reinterpret_cast<const float4*>(rays);
    auto enqueue = [&]() -> hipError_t {
        const uint32_t* order = nullptr;
        if (sorted)
            if (hipError_t e = enqueue_ray_order(g, r4, n, stream, order); e != hipSuccess)
                return e;
        // {what, sorted, fast}: the arithmetic policy is the shade pass's ("gi_exact_shade")
        using Kernel = void (*)(SceneView, const ShadeHeader*, const float4*, uint32_t, const uint32_t*, ShadeSun, float4*);
        static const Kernel kernels[2][2][2] = {
            {{ray_shade_kernel<NEB_SHADE_SURFACE, false, false>, ray_shade_kernel<NEB_SHADE_SURFACE, false, true>},
             {ray_shade_kernel<NEB_SHADE_SURFACE, true, false>, ray_shade_kernel<NEB_SHADE_SURFACE, true, true>}},
            {{ray_shade_kernel<NEB_SHADE_RADIANCE, false, false>, ray_shade_kernel<NEB_SHADE_RADIANCE, false, true>},
             {ray_shade_kernel<NEB_SHADE_RADIANCE, true, false>, ray_shade_kernel<NEB_SHADE_RADIANCE, true, true>}}};
        hipLaunchKernelGGL(kernels[radiance][sorted][!g->exact_shade], dim3((n + 63u) / 64u), dim3(64), 0, stream, g->view, g->shade_heads, r4, n, order, sun,
                           static_cast<float4*>(out));
        return hipGetLastError();
    };
    const hipError_t launched = enqueue();
    if (sorted) { // (also behind a chain that broke off half way: whatever of it was enqueued uses the block)
        GI_HIP(ctx, hipEventRecord(g->query_ev, stream));
        g->query_stream = stream;
        g->query_ev_pending = true;
    }
    GI_HIP(ctx, launched);
    return NEB_OK;
}

namespace {

// What the two tail calls check of a non-null neb_probe_tail before any pointer is looked up (`who` in front): the grid, the flags, the
// two pointers, the bias, and that nothing the call writes or reads as its own input (`spans`) overlaps the grid's buffers.
struct TailSpan {
    const void* p;
    size_t bytes;
    const char* name;
};
int tail_shape(neb_ctx* ctx, const char* who, const neb_probe_tail* tail, const TailSpan* spans, int n_spans, uint32_t* count)
{
    if (int rc = grid_shape(ctx, who, &tail->grid, count))
        return rc;
    if (tail->flags & ~NEB_TAIL_FRAME_WEIGHT)
        return fail(ctx, who, "unknown tail flag bits (0 or NEB_TAIL_FRAME_WEIGHT)");
    if (!tail->records)
        return fail(ctx, who, "null tail records");
    if (((uintptr_t)tail->records & 31u) || ((uintptr_t)tail->visibility & 31u))
        return fail(ctx, who, "misaligned pointer (tail records, visibility: 32 bytes)");
    if (tail->visibility && !(std::isfinite(tail->normal_bias) && tail->normal_bias >= 0.0f))
        return fail(ctx, who, "normal_bias must be finite and >= 0");
    const size_t record_bytes = (size_t)*count * sizeof(neb_probe_record), visibility_bytes = (size_t)*count * sizeof(neb_probe_visibility);
    char msg[160];
    for (int q = 0; q < n_spans; ++q) {
        if (!spans[q].p)
            continue;
        if (spans_overlap(tail->records, record_bytes, spans[q].p, spans[q].bytes)) {
            snprintf(msg, sizeof(msg), "tail records overlap %s (bake into a second buffer, then accumulate)", spans[q].name);
            return fail(ctx, who, msg);
        }
        if (tail->visibility && spans_overlap(tail->visibility, visibility_bytes, spans[q].p, spans[q].bytes)) {
            snprintf(msg, sizeof(msg), "tail visibility overlaps %s", spans[q].name);
            return fail(ctx, who, msg);
        }
    }
    return NEB_OK;
}
// ... and after GI_GUARD: that the device reads them.
int tail_readable(neb_ctx* ctx, const char* who, const neb_probe_tail* tail, uint32_t count)
{
    if (!device_readable(ctx, tail->records, (size_t)count * sizeof(neb_probe_record)))
        return fail(ctx, who, "tail records is not memory this context's device reads, or the grid's records leave its allocation");
    if (tail->visibility && !device_readable(ctx, tail->visibility, (size_t)count * sizeof(neb_probe_visibility)))
        return fail(ctx, who, "tail visibility is not memory this context's device reads, or the grid's records leave its allocation");
    return NEB_OK;
}
TailArgs tail_args(const neb_probe_tail* tail)
{
    TailArgs a;
    a.G = tail->grid;
    a.records = reinterpret_cast<const float4*>(tail->records);
    a.visibility = reinterpret_cast<const float2*>(tail->visibility);
    a.normal_bias = tail->visibility ? tail->normal_bias : 0.0f;
    a.frame_weight = (tail->flags & NEB_TAIL_FRAME_WEIGHT) ? 1u : 0u;
    return a;
}

// neb_gi_trace_paths (tail == nullptr: its kernels, its bits) and neb_gi_trace_paths_tail.
int trace_paths(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants, const neb_probe_tail* tail, void* out,
                void* vertices, neb_stream stream_)
{
    static const char who_tail[] = "neb_gi_trace_paths_tail";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_trace_paths: scene/BVH not ready");
    if (flags & ~NEB_RAYS_SORT)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, flags & NEB_RAYS_ANY_HIT ? "neb_gi_trace_paths: NEB_RAYS_ANY_HIT is not a flag of this call (a path follows closest hits)"
                                                                          : "neb_gi_trace_paths: unknown flag bits");
    const bool sorted = (flags & NEB_RAYS_SORT) != 0;
    if (n == 0)
        return NEB_OK;
    if (n > kQueryMaxRays)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_trace_paths: more than 2^28 rays in one call");
    if (!constants)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: null constants");
    const uint32_t max_vertices = constants->maxPathVertices;
    if (max_vertices < 2u || max_vertices > 8u)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: maxPathVertices outside 2..8");
    const size_t ray_bytes = (size_t)n * sizeof(neb_ray), out_bytes = (size_t)n * sizeof(neb_ray_path);
    const size_t vertex_bytes = (size_t)n * (max_vertices - 1u) * sizeof(neb_path_vertex);
    if (!rays || !out)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: null rays or out");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)out & 31u) || ((uintptr_t)vertices & 31u))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: misaligned pointer (rays: 16 bytes; out, vertices: 32 bytes)");
    if (ranges_overlap(rays, ray_bytes, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: out overlaps rays");
    if (vertices && (ranges_overlap(rays, ray_bytes, vertices, vertex_bytes) || ranges_overlap(out, out_bytes, vertices, vertex_bytes)))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: vertices overlaps rays or out");
    uint32_t tail_count = 0;
    if (tail) {
        const TailSpan spans[3] = {{out, out_bytes, "out"}, {vertices, vertex_bytes, "vertices"}, {rays, ray_bytes, "rays"}};
        if (int rc = tail_shape(ctx, who_tail, tail, spans, 3, &tail_count))
            return rc;
    }
    GI_GUARD(ctx);
    if (!device_readable(ctx, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: rays is not memory this context's device reads, or n rays leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: out is not memory this context's device reads, or n records leave its allocation");
    if (vertices && !device_readable(ctx, vertices, vertex_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG,
                       "neb_gi_trace_paths: vertices is not memory this context's device reads, or n * (maxPathVertices - 1) records leave its allocation");
    if (tail)
        if (int rc = tail_readable(ctx, who_tail, tail, tail_count))
            return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ShadeSun sun = {}; // (neb_gi_trace refuses no value of the sun fields, so none is refused here: they act as they act on the frame)
    sun_frame(constants->sunLightDirection, sun.L, sun.B, sun.T);
    for (int q = 0; q < 3; ++q) {
        sun.radiance[q] = constants->sunLightRadiance[q];
        sun.sky[q] = constants->skyColor[q];
    }
    sun.tan_half = constants->sunTanHalfAngle;
    sun.frame_index = constants->frameIndex;
    if (sorted) // (before anything is enqueued: a failed allocation leaves the stream as it was)
        GI_HIP(ctx, query_sort_block(g, query_sort_bytes(n), stream));
    GI_HIP(ctx, gi_scene_reader(g, stream)); // behind any update enqueued on another stream; a later update waits for this stream
    const float4* r4 = reinterpret_cast<const float4*>(rays);
    auto enqueue = [&]() -> hipError_t {
        const uint32_t* order = nullptr;
        if (sorted)
            if (hipError_t e = enqueue_ray_order(g, r4, n, stream, order); e != hipSuccess)
                return e;
        // {sorted, fast, vertices}: the arithmetic policy is the shade pass's ("gi_exact_shade")
        using Kernel = void (*)(SceneView, const ShadeHeader*, const float4*, uint32_t, const uint32_t*, ShadeSun, uint32_t, float4*, float4*);
        static const Kernel kernels[2][2][2] = {{{ray_path_kernel<false, false, false>, ray_path_kernel<false, false, true>},
                                                 {ray_path_kernel<false, true, false>, ray_path_kernel<false, true, true>}},
                                                {{ray_path_kernel<true, false, false>, ray_path_kernel<true, false, true>},
                                                 {ray_path_kernel<true, true, false>, ray_path_kernel<true, true, true>}}};
        if (!tail) {
            hipLaunchKernelGGL(kernels[sorted][!g->exact_shade][vertices != nullptr], dim3((n + 63u) / 64u), dim3(64), 0, stream, g->view, g->shade_heads, r4, n,
                               order, sun, max_vertices, static_cast<float4*>(out), static_cast<float4*>(vertices));
            return hipGetLastError();
        }
        // {visible, sorted, fast, vertices}
        using TailKernel = void (*)(SceneView, const ShadeHeader*, const float4*, uint32_t, const uint32_t*, ShadeSun, uint32_t, float4*, float4*, TailArgs);
        static const TailKernel tail_kernels[2][2][2][2] = {{{{ray_path_kernel<false, false, false, 1, TailArgs>, ray_path_kernel<false, false, true, 1, TailArgs>},
                                                              {ray_path_kernel<false, true, false, 1, TailArgs>, ray_path_kernel<false, true, true, 1, TailArgs>}},
                                                             {{ray_path_kernel<true, false, false, 1, TailArgs>, ray_path_kernel<true, false, true, 1, TailArgs>},
                                                              {ray_path_kernel<true, true, false, 1, TailArgs>, ray_path_kernel<true, true, true, 1, TailArgs>}}},
                                                            {{{ray_path_kernel<false, false, false, 2, TailArgs>, ray_path_kernel<false, false, true, 2, TailArgs>},
                                                              {ray_path_kernel<false, true, false, 2, TailArgs>, ray_path_kernel<false, true, true, 2, TailArgs>}},
                                                             {{ray_path_kernel<true, false, false, 2, TailArgs>, ray_path_kernel<true, false, true, 2, TailArgs>},
                                                              {ray_path_kernel<true, true, false, 2, TailArgs>, ray_path_kernel<true, true, true, 2, TailArgs>}}}};
        hipLaunchKernelGGL(tail_kernels[tail->visibility != nullptr][sorted][!g->exact_shade][vertices != nullptr], dim3((n + 63u) / 64u), dim3(64), 0, stream,
                           g->view, g->shade_heads, r4, n, order, sun, max_vertices, static_cast<float4*>(out), static_cast<float4*>(vertices), tail_args(tail));
        return hipGetLastError();
    };
    const hipError_t launched = enqueue();
    if (sorted) { // (also behind a chain that broke off half way: whatever of it was enqueued uses the block)
        GI_HIP(ctx, hipEventRecord(g->query_ev, stream));
        g->query_stream = stream;
        g->query_ev_pending = true;
    }
    GI_HIP(ctx, launched);
    return NEB_OK;
}

} // namespace

extern "C" int neb_gi_trace_paths(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants, void* out, void* vertices,
                                  neb_stream stream)
{
    return trace_paths(ctx, rays, n, flags, constants, nullptr, out, vertices, stream);
}

extern "C" int neb_gi_trace_paths_tail(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants,
                                       const neb_probe_tail* tail, void* out, void* vertices, neb_stream stream)
{
    return trace_paths(ctx, rays, n, flags, constants, tail, out, vertices, stream);
}

namespace {

// What the two probe calls check of `what` and `samples` before anything else, with the caller's name in front.
int probe_shape(neb_ctx* ctx, const char* who, uint32_t what, uint32_t samples, uint32_t n)
{
    char msg[160];
    if (what != NEB_BAKE_SH && what != NEB_BAKE_IRRADIANCE) {
        snprintf(msg, sizeof(msg), "%s: unknown `what` (NEB_BAKE_SH or NEB_BAKE_IRRADIANCE)", who);
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, msg);
    }
    if (samples < 64u || samples > kProbeMaxSamples || (samples & 63u)) {
        snprintf(msg, sizeof(msg), "%s: samples must be a multiple of 64 in 64..4096", who);
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, msg);
    }
    if ((uint64_t)n * samples > kQueryMaxRays) {
        snprintf(msg, sizeof(msg), "%s: more than 2^28 samples (n * samples) in one call", who);
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, msg);
    }
    return NEB_OK;
}

} // namespace

extern "C" int neb_gi_probe_rays(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t frame_index, neb_ray* rays,
                                 neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    if (int rc = probe_shape(ctx, "neb_gi_probe_rays", what, samples, n))
        return rc;
    if (n == 0)
        return NEB_OK;
    const size_t probe_bytes = (size_t)n * sizeof(neb_probe), ray_bytes = (size_t)n * samples * sizeof(neb_ray);
    if (!probes || !rays)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_probe_rays: null probes or rays");
    if (((uintptr_t)probes & 15u) || ((uintptr_t)rays & 15u))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_probe_rays: misaligned pointer (probes, rays: 16 bytes)");
    if (ranges_overlap(probes, probe_bytes, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_probe_rays: rays overlaps probes");
    GI_GUARD(ctx);
    if (!device_readable(ctx, probes, probe_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_probe_rays: probes is not memory this context's device reads, or n probes leave its allocation");
    if (!device_readable(ctx, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_probe_rays: rays is not memory this context's device reads, or n * samples rays leave its allocation");
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t n_rays = n * samples;
    const float4* p4 = reinterpret_cast<const float4*>(probes);
    float4* r4 = reinterpret_cast<float4*>(rays);
    if (what == NEB_BAKE_SH)
        hipLaunchKernelGGL(probe_rays_kernel<NEB_BAKE_SH>, dim3((n_rays + 255u) / 256u), dim3(256), 0, stream, p4, n_rays, samples, frame_index, r4);
    else
        hipLaunchKernelGGL(probe_rays_kernel<NEB_BAKE_IRRADIANCE>, dim3((n_rays + 255u) / 256u), dim3(256), 0, stream, p4, n_rays, samples, frame_index, r4);
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

namespace {

// neb_gi_bake_probes (tail == nullptr: its kernels, its bits) and neb_gi_bake_probes_tail.
int bake_probes(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags, const neb_gi_constants* constants,
                const neb_probe_tail* tail, neb_probe_record* out, neb_stream stream_)
{
    static const char who_tail[] = "neb_gi_bake_probes_tail";
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g || !g->built)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_bake_probes: scene/BVH not ready");
    if (flags)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, flags & NEB_RAYS_SORT ? "neb_gi_bake_probes: NEB_RAYS_SORT is not a flag of this call (a wave's rays share their origin)"
                                                                       : "neb_gi_bake_probes: unknown flag bits (flags must be 0)");
    if (int rc = probe_shape(ctx, "neb_gi_bake_probes", what, samples, n))
        return rc;
    if (n == 0)
        return NEB_OK;
    if (!constants)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: null constants");
    const uint32_t max_vertices = constants->maxPathVertices;
    if (max_vertices < 2u || max_vertices > 8u)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: maxPathVertices outside 2..8");
    const size_t probe_bytes = (size_t)n * sizeof(neb_probe), out_bytes = (size_t)n * sizeof(neb_probe_record);
    if (!probes || !out)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: null probes or out");
    if (((uintptr_t)probes & 15u) || ((uintptr_t)out & 31u))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: misaligned pointer (probes: 16 bytes; out: 32 bytes)");
    if (ranges_overlap(probes, probe_bytes, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: out overlaps probes");
    uint32_t tail_count = 0;
    if (tail) {
        const TailSpan spans[2] = {{out, out_bytes, "out"}, {probes, probe_bytes, "probes"}};
        if (int rc = tail_shape(ctx, who_tail, tail, spans, 2, &tail_count))
            return rc;
    }
    GI_GUARD(ctx);
    if (!device_readable(ctx, probes, probe_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: probes is not memory this context's device reads, or n probes leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_bake_probes: out is not memory this context's device reads, or n records leave its allocation");
    if (tail)
        if (int rc = tail_readable(ctx, who_tail, tail, tail_count))
            return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ShadeSun sun = {}; // (as neb_gi_trace_paths: no value of the sun fields is refused)
    sun_frame(constants->sunLightDirection, sun.L, sun.B, sun.T);
    for (int q = 0; q < 3; ++q) {
        sun.radiance[q] = constants->sunLightRadiance[q];
        sun.sky[q] = constants->skyColor[q];
    }
    sun.tan_half = constants->sunTanHalfAngle;
    sun.frame_index = constants->frameIndex;
    // the one factor of the reduction: 4 pi / S over the sphere, pi / S under the cosine density, in double and rounded once
    const double pi = 3.14159265358979323846;
    const float scale = what == NEB_BAKE_SH ? (float)(4.0 * pi / (double)samples) : (float)((double)kPi / (double)samples);
    GI_HIP(ctx, gi_scene_reader(g, stream)); // behind any update enqueued on another stream; a later update waits for this stream
    // {what, fast}: the arithmetic policy is the shade pass's ("gi_exact_shade")
    using Kernel = void (*)(SceneView, const ShadeHeader*, const float4*, uint32_t, ShadeSun, uint32_t, float, float4*);
    static const Kernel kernels[2][2] = {{probe_bake_kernel<NEB_BAKE_SH, false>, probe_bake_kernel<NEB_BAKE_SH, true>},
                                         {probe_bake_kernel<NEB_BAKE_IRRADIANCE, false>, probe_bake_kernel<NEB_BAKE_IRRADIANCE, true>}};
    if (!tail) {
        hipLaunchKernelGGL(kernels[what == NEB_BAKE_IRRADIANCE][!g->exact_shade], dim3(n), dim3(64), 0, stream, g->view, g->shade_heads,
                           reinterpret_cast<const float4*>(probes), samples, sun, max_vertices, scale, reinterpret_cast<float4*>(out));
    } else { // {visible, what, fast}
        using TailKernel = void (*)(SceneView, const ShadeHeader*, const float4*, uint32_t, ShadeSun, uint32_t, float, float4*, TailArgs);
        static const TailKernel tail_kernels[2][2][2] = {
            {{probe_bake_kernel<NEB_BAKE_SH, false, 1, TailArgs>, probe_bake_kernel<NEB_BAKE_SH, true, 1, TailArgs>},
             {probe_bake_kernel<NEB_BAKE_IRRADIANCE, false, 1, TailArgs>, probe_bake_kernel<NEB_BAKE_IRRADIANCE, true, 1, TailArgs>}},
            {{probe_bake_kernel<NEB_BAKE_SH, false, 2, TailArgs>, probe_bake_kernel<NEB_BAKE_SH, true, 2, TailArgs>},
             {probe_bake_kernel<NEB_BAKE_IRRADIANCE, false, 2, TailArgs>, probe_bake_kernel<NEB_BAKE_IRRADIANCE, true, 2, TailArgs>}}};
        hipLaunchKernelGGL(tail_kernels[tail->visibility != nullptr][what == NEB_BAKE_IRRADIANCE][!g->exact_shade], dim3(n), dim3(64), 0, stream, g->view,
                           g->shade_heads, reinterpret_cast<const float4*>(probes), samples, sun, max_vertices, scale, reinterpret_cast<float4*>(out),
                           tail_args(tail));
    }
    GI_HIP(ctx, hipGetLastError());
    return NEB_OK;
}

} // namespace

extern "C" int neb_gi_bake_probes(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags,
                                  const neb_gi_constants* constants, neb_probe_record* out, neb_stream stream)
{
    return bake_probes(ctx, probes, n, samples, what, flags, constants, nullptr, out, stream);
}

extern "C" int neb_gi_bake_probes_tail(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags,
                                       const neb_gi_constants* constants, const neb_probe_tail* tail, neb_probe_record* out, neb_stream stream)
{
    return bake_probes(ctx, probes, n, samples, what, flags, constants, tail, out, stream);
}
