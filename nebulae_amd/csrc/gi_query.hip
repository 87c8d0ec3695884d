// gi_query.hip -- the caller's own rays against the scene the context holds: neb_gi_cast_rays and neb_gi_shade_rays
// (3.8a), which walks the same way and then shades the hit as the frame's shade pass would.
//
// Rays and answers live in device buffers of the caller.  One lane per ray walks the tree the frame's kernels walk, with the
// traverser they use (traverse, gi_device.h: same boxes, same triangle test, same barycentrics), closest hit or first hit; with
// NEB_RAYS_SORT the rays are visited in the order of a 16-bit key (direction octant above the origin's Morton bits, bounce_sort_key)
// and every answer still lands at its ray's own index.  A ray's walk depends on the ray and the tree alone, so the order changes
// no answer.  Nothing of the frame is touched: no plane, no ray counter, no statistics, no sun table.
#include "gi_device.h" // (turns floating-point contraction off for this file: see there)

namespace neb {

namespace {

constexpr uint32_t kQueryMaxRays = 1u << 28; // 8 GiB of rays; the sort's indices and raysort.hip's tile counts stay far inside 32 bits
constexpr uint32_t kNoId = 0xffffffffu;
constexpr uint32_t kUnwalkableKey = (1u << kSortBits) - 1u; // above every key of bounce_sort_key: such rays gather at the end

// The interval the walk assumes: the triangle screen of intersect_tri_regs takes tmin >= 0 for granted, and an empty interval holds
// no hit.  Written so that a NaN on either side says no.
__device__ __forceinline__ bool interval_ok(float tmin, float tmax) { return tmin >= 0.0f && tmax > tmin; }

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
template <bool SORTED, bool FAST, bool VERTICES>
__global__ __launch_bounds__(64) void ray_path_kernel(SceneView S, const ShadeHeader* __restrict__ heads, const float4* __restrict__ rays, uint32_t n,
                                                      const uint32_t* __restrict__ order, ShadeSun sun, uint32_t max_vertices, float4* __restrict__ out,
                                                      float4* __restrict__ vertices)
{
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

    bool alive = ray_walkable(o, dir, tmin, tmax);
    uint32_t rng = jenkins(i ^ jenkins(sun.frame_index));
    float3 throughput = f3(1.0f, 1.0f, 1.0f), sum = f3(0.0f, 0.0f, 0.0f);
    float first_t = __builtin_inff();
    uint32_t first_geometry = kNoId, first_primitive = kNoId, path_flags = alive ? 0u : (uint32_t)NEB_HIT_NOT_WALKED, segments = 0u;
    uint32_t k = 1u;
    for (; k <= last; ++k) {
        if (__ballot(alive) == 0ull)
            break;
        Hit h;
        const bool found = traverse(S, o, alive ? dir : f3(0.0f, 0.0f, 0.0f), tmin, tmax, false, stack, h);
        // (a later segment the traverser refuses -- a direction that is not finite -- is a miss, as it is one in the frame)
        uint32_t flags = alive && k > 1u && !ray_walkable(o, dir, tmin, tmax) ? (uint32_t)NEB_HIT_NOT_WALKED : 0u;
        float t = __builtin_inff(), bu = 0.0f, bv = 0.0f;
        uint32_t geometry = kNoId, primitive = kNoId;
        float3 hitP = f3(0.0f, 0.0f, 0.0f);
        Surface surf;
        surf.GN = surf.SN = surf.albedo = f3(0.0f, 0.0f, 0.0f);
        surf.roughness = surf.metalness = 0.0f;
        if (found) { // (ray_shade_kernel's reconstruction, its flags)
            const float4 ids = S.tris[3 * h.tri + 2]; // {e2.z, geometry, primitive, -}
            const TriShade ts = load_tri_shade(S, h.tri);
            const ShadeHead head = load_shade_header(heads, ts.geom);
            float tex_u = 0.0f, tex_v = 0.0f;
            t = h.t, bu = h.u, bv = h.v;
            geometry = __float_as_uint(ids.y), primitive = __float_as_uint(ids.z);
            hitP = o + dir * h.t;
            flags |= NEB_HIT_FOUND;
            const bool has_material = reconstruct_geometry<FAST>(head, ts, h.u, h.v, surf, tex_u, tex_v);
            if (head.valid)
                flags |= NEB_HIT_ATTRIBUTES | (dot3(surf.GN, dir) > 0.0f ? (uint32_t)NEB_HIT_BACKFACE : 0u);
            if (has_material) {
                MapSamples maps;
                sample_material_maps<FAST>(S, head.mat, tex_u, tex_v, maps);
                reconstruct_material<FAST>(head.mat, ts, h.u, h.v, maps, surf);
                flags |= NEB_HIT_MATERIAL;
            }
        }
        const bool shaded = (flags & NEB_HIT_MATERIAL) != 0;
        // shade_pixel's shadow ray, its exact-arithmetic sequence under both policies; the two disk draws advance the path's stream
        // where there is a surface to shade
        const uint32_t rng_in = rng;
        const float3 throughput_in = throughput;
        uint32_t rng_disk = rng;
        const float a0 = rand01(rng_disk), a1 = rand01(rng_disk);
        const float angle = a0 * 2.0f * 3.1415926535f, dist = fsqrt<false>(a1);
        float sn_a, cs_a;
        det_sincosf(angle, sn_a, cs_a);
        const float3 inc = normalize3<false>(L + (Bv * sn_a + T * cs_a) * sun.tan_half * dist);
        const bool transition = dot3(surf.GN, inc) <= 0.0f;
        const float3 so = hitP + (transition ? -surf.GN : surf.GN) * 1e-2f;
        Hit sh;
        const bool occluded = traverse(S, so, shaded ? inc : f3(0.0f, 0.0f, 0.0f), 0.001f, kTraceMax, true, stack, sh);
        float3 added = f3(0.0f, 0.0f, 0.0f);
        const float3 V = normalize3<FAST>(-dir); // :522
        if (alive && !found) { // :508
            added = f3(sun.sky[0], sun.sky[1], sun.sky[2]) * throughput;
            path_flags |= NEB_PATH_ESCAPED;
        }
        if (shaded) {
            rng = rng_disk;
            if (!occluded) {
                added = evaluate_direct_brdf<FAST>(surf, V, L) * f3(sun.radiance[0], sun.radiance[1], sun.radiance[2]) * throughput; // :573-574
                flags |= NEB_HIT_SUN_VISIBLE;
            }
        }
        if (alive) {
            sum = k == 1u ? added : sum + added;
            ++segments;
        }
        if (k == 1u) {
            first_t = t, first_geometry = geometry, first_primitive = primitive;
            path_flags |= flags;
        }
        float4 seg_o = make_float4(o.x, o.y, o.z, tmin), seg_d = make_float4(dir.x, dir.y, dir.z, t);
        const float seg_tmax = tmax;
        float pdiff = 0.0f;
        const bool bounce = shaded && k < last; // (:579-583; `shaded` implies `alive`)
        if (bounce) {
            // EvaluateIndirectBRDF (:230-259) takes rng BY VALUE: the Rand(rng) of :614 returns the same number as the first of its draws
            uint32_t rng_copy = rng;
            const float3 SNn = normalize3<FAST>(surf.SN);
            const float e0 = rand01(rng_copy), e1 = rand01(rng_copy);
            const float3 Ld = cosine_hemisphere_aligned<FAST>(e0, e1, SNn);
            pdiff = 1.0f - specular_probability<FAST>(saturate1(dot3(V, SNn)), specular_f0(surf.albedo, surf.metalness), surf.albedo);
            o = hitP + surf.GN * 1e-2f; // :607
            dir = Ld;
            tmin = 0.001f, tmax = kTraceMax;
            throughput = throughput * (surf.albedo * (1.0f - surf.metalness)); // :613
            if (rand01(rng) < pdiff) {
                throughput = f3(fdiv<FAST>(throughput.x, pdiff), fdiv<FAST>(throughput.y, pdiff), fdiv<FAST>(throughput.z, pdiff)); // :614-618
                flags |= NEB_PATH_DIVIDED;
            }
        }
        if constexpr (VERTICES) {
            float4* rec = vrec + 6 * (size_t)(k - 1u);
            if (alive) {
                rec[0] = seg_o;
                rec[1] = seg_d;
                rec[2] = make_float4(throughput_in.x, throughput_in.y, throughput_in.z, __uint_as_float(rng_in));
                rec[3] = make_float4(added.x, added.y, added.z, __uint_as_float(flags));
                rec[4] = make_float4(__uint_as_float(geometry), __uint_as_float(primitive), bu, bv);
                rec[5] = make_float4(seg_tmax, pdiff, 0.0f, 0.0f);
            } else {
                for (int q = 0; q < 6; ++q)
                    rec[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        alive = bounce;
    }
    if constexpr (VERTICES)
        for (; k <= last; ++k) // (the wave left the loop early: every record is written)
            for (int q = 0; q < 6; ++q)
                vrec[6 * (size_t)(k - 1u) + q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4* rec = out + 2 * (size_t)i;
    rec[0] = make_float4(sum.x, sum.y, sum.z, first_t);
    rec[1] = make_float4(__uint_as_float(first_geometry), __uint_as_float(first_primitive), __uint_as_float(path_flags), __uint_as_float(segments));
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

extern "C" int neb_gi_trace_paths(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants, void* out, void* vertices,
                                  neb_stream stream_)
{
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
    GI_GUARD(ctx);
    if (!device_readable(ctx, rays, ray_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: rays is not memory this context's device reads, or n rays leave its allocation");
    if (!device_readable(ctx, out, out_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_trace_paths: out is not memory this context's device reads, or n records leave its allocation");
    if (vertices && !device_readable(ctx, vertices, vertex_bytes))
        return gi_fail(ctx, NEB_ERR_INVALID_ARG,
                       "neb_gi_trace_paths: vertices is not memory this context's device reads, or n * (maxPathVertices - 1) records leave its allocation");
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
        hipLaunchKernelGGL(kernels[sorted][!g->exact_shade][vertices != nullptr], dim3((n + 63u) / 64u), dim3(64), 0, stream, g->view, g->shade_heads, r4, n, order,
                           sun, max_vertices, static_cast<float4*>(out), static_cast<float4*>(vertices));
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
