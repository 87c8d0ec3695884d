// gi_internal.h -- scene tables, BVH node layouts and the GI state shared by gi_build.hip (scene upload, BVH build)
// and gi.hip (wavefront kernels, C ABI of the trace).  Tuning knobs are -D macros with the measured defaults.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "neb_device.h"
#include "neb_internal.h"

namespace neb {


// ------------------------------------------------------------------------------------------------
// Device-side scene
// ------------------------------------------------------------------------------------------------
struct DevGeom {
    float m[9];          // upper 3x3 of surfaceToWorld (row-vector convention)
    int32_t material;
    uint32_t firstIndex; // into the uint32 index pool
    uint32_t vertexBase; // into the SoA vertex pools
    uint32_t valid;      // all four attribute streams + indices present
    uint32_t pad[3];
};
struct DevMat {
    int32_t tex[3];
    float albedo[3];
    float rough, metal;
    // When the material has all three maps and they share one size, their bilinear footprints are stored interleaved, one
    // 32-byte entry per texel position: the 4 texels of the footprint x {albedo.rgb, normal.rgb, roughness, metalness}
    // -- the three filtered fetches of a hit (same uv) are then ONE 32-byte access.  bundle_w == 0: not bundled.
    uint32_t bundle;   // first entry, in 32-byte units, into SceneView::bundles
    uint32_t bundle_w, bundle_h;
    uint32_t pad;
};
// What the shade pass takes from a geometry AND from the material it names, side by side in one 128-byte line (built where the two
// tables are, neb_gi_set_scene): the hit's record names the geometry, and one lookup -- six 16-byte loads of one line -- stands where
// geoms[geom] -> mats[material] were two that waited for one another.  Same values as the two tables (a geometry without a material
// keeps material < 0 and the fields of no material: zeros, tex = -1).
struct alignas(128) ShadeHeader {
    float m[9];        // DevGeom::m                                  q0, q1, q2.x
    uint32_t valid;    // DevGeom::valid                              q2.y
    int32_t material;  // DevGeom::material (sign kept)               q2.z
    uint32_t bundle;   // DevMat::bundle, bundle_w, bundle_h          q2.w, q3.xy
    uint32_t bundle_w, bundle_h;
    int32_t tex[3];    // DevMat::tex                                 q3.zw, q4.x
    float albedo[3];   // DevMat::albedo                              q4.yzw
    float rough, metal; //                                            q5.xy
    uint32_t pad[10];
};
static_assert(sizeof(ShadeHeader) == 128 && offsetof(ShadeHeader, rough) == 80, "shade header layout (load_shade_header, gi_device.h)");
struct DevTex {
    uint32_t offset; // in footprint entries (16 B), into the texel pool
    uint32_t w, h, pad;
};
// 64-byte BVH2 node: both children's boxes live in the parent, so one node fetch decides both.
struct BvhNode {
    float c0min[3];
    int32_t c0; // >= 0: inner node, < 0: leaf, triangle = ~c
    float c0max[3];
    int32_t c1;
    float c1min[3];
    uint32_t pad0;
    float c1max[3];
    uint32_t pad1;
};

// 128-byte BVH4 node produced by collapsing the binary SAH tree (SoA per axis: one float4 per bound and axis).
// child >= 0: inner node index; child < 0: leaf, code = ~child = (first_triangle << 2) | (count - 1), count <= 4;
// unused slots carry an inverted (never-hit) box.  The lower and the upper plane of an axis sit 64 bytes apart, so
// a ray picks its near plane with a per-ray byte offset (0 or 64 by the sign of its direction) and the far plane
// with offset ^ 64: no min / max per slab.
struct Bvh4Node {
    float4 lox, loy, loz; //  0, 16, 32
    int4 child;           // 48
    float4 hix, hiy, hiz; // 64, 80, 96
    int4 pad;             // .x: the slots the build used, bit q = slot q (refit_level_kernel tells an emptied slot from an unused one by it); no ray reads it
};
static_assert(sizeof(Bvh4Node) == 128 && offsetof(Bvh4Node, hix) == offsetof(Bvh4Node, lox) + 64, "node layout");
// The same tree in 64 bytes per node, for the rays that only ask "is anything in the way" (any-hit: sun visibility).
// The child boxes are 8-bit offsets from the node's own (padded) lower corner in units of scale = extent / 255, rounded
// OUTWARDS with margin (quantise_nodes_kernel, gi_build.hip, says exactly what is proven): a decoded box contains the exact
// one, so a ray visits the nodes an exact walk would plus possibly more, and the triangle tests behind them are the exact
// ones -- up to rays that graze a box face at the rounding level of the folded slab arithmetic, where any two fp32
// traversals may differ.  Child c of axis a: byte c of qlo[a] / qhi[a]; an unused
// slot is the inverted box 255 / 0 (scale > 0 always).  Four 16-byte loads per node visit instead of seven, and half
// the cache footprint: the traversal passes are bound by the texture-address unit.
struct Bvh4NodeQ {
    float ox, oy, oz, sx; //  0
    float sy, sz;         // 16
    uint32_t qlox, qloy;
    uint32_t qloz, qhix, qhiy, qhiz; // 32
    int4 child;           // 48: as Bvh4Node::child
};
static_assert(sizeof(Bvh4NodeQ) == 64, "quantised node layout");
#ifndef NEB_TRACE_WAVES
#define NEB_TRACE_WAVES 8 // waves per SIMD the traversal kernels are register-budgeted for
#endif
#ifndef NEB_SHADE_WAVES
#define NEB_SHADE_WAVES 4 // waves per SIMD gi_shade_kernel is register-budgeted for
#endif
#ifndef NEB_LEAF_BATCH
#define NEB_LEAF_BATCH 12
#endif
constexpr int kLeafBatch = NEB_LEAF_BATCH;
#ifndef NEB_MAX_LEAF_TRIS
#define NEB_MAX_LEAF_TRIS 2 // 1..4 (the leaf code keeps count - 1 in two bits); measured 1/2/3/4: 1407 / 1390 / 1403 / 1500 us of GI per 1080p frame
#endif
constexpr int kMaxLeafTris = NEB_MAX_LEAF_TRIS;
// The geometry word of a triangle's shading record (r6.w) carries the sun-visibility table in its two top bits
// (gi_sun_table.hip): bit kLitShift = every shadow ray leaving the triangle on its +GN side is unoccluded, bit kLitShift + 1 = -GN side.
constexpr uint32_t kLitShift = 30u, kGeomMask = (1u << kLitShift) - 1u;
// ... and r7.yzw = occluder hints: the (up to) kHints triangles most likely to shadow rays that start on this one, as 23-bit
// indices (scenes of up to 8.4 M triangles; a triangle whose index does not fit is simply no candidate: gi_sun_table.hip) + the side
// (0: +GN, 1: -GN) they were chosen for.  Bits 0-22 hint 0, 23-45 hint 1, 46-68 hint 2, 69-91 hint 3, bit 95 the side.
// (Round 4 had 21 bits: in leaf order the top of a scene -- what shadows a sun ray -- sorts LAST, so at 2.6 M triangles nearly every
// occluder was out of range and the hints answered nothing.)
constexpr int kHints = 4;
constexpr uint32_t kNoHint = 0x7fffffu;
__host__ __device__ inline void pack_hints(const uint32_t hint[kHints], uint32_t side, float4& r7)
{
    uint32_t h[kHints];
    for (int k = 0; k < kHints; ++k)
        h[k] = hint[k] < kNoHint ? hint[k] : kNoHint;
    const unsigned long long lo = (unsigned long long)h[0] | ((unsigned long long)h[1] << 23) | ((unsigned long long)(h[2] & 0x3ffffu) << 46);
    union { uint32_t u; float f; } y, z, w;
    y.u = (uint32_t)lo;
    z.u = (uint32_t)(lo >> 32);
    w.u = (h[2] >> 18) | (h[3] << 5) | (side << 31);
    r7.y = y.f, r7.z = z.f, r7.w = w.f;
}
__host__ __device__ inline void unpack_hints(const float4& r7, uint32_t hint[kHints], uint32_t& side)
{
    union { float f; uint32_t u; } y, z, w;
    y.f = r7.y, z.f = r7.z, w.f = r7.w;
    const unsigned long long lo = (unsigned long long)y.u | ((unsigned long long)z.u << 32);
    hint[0] = (uint32_t)lo & kNoHint;
    hint[1] = (uint32_t)(lo >> 23) & kNoHint;
    hint[2] = ((uint32_t)(lo >> 46) | (w.u << 18)) & kNoHint;
    hint[3] = (w.u >> 5) & kNoHint;
    side = w.u >> 31;
}

struct SceneView {
    const float4* tris;      // 3 x float4 per triangle: {v0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, geom, prim, -}
    const Bvh4Node* nodes;
    const Bvh4NodeQ* qnodes; // the 64-byte copy the any-hit rays walk
    const DevGeom* geoms;
    const DevMat* mats;
    const DevTex* texs;
    const uint32_t* indices;
    const float* normals;    // 3 per vertex
    const float* uvs;        // 2 per vertex
    const float* tangents;   // 4 per vertex
    const uint32_t* texels;  // RGBA8 bilinear footprint table: 4 texels (16 B) per texel position, see sample_texture
    const uint4* bundles;    // per-material interleaved footprints (2 x uint4 per texel position), see DevMat::bundle
    const float4* shade;     // 8 x float4 (one 128-B line) per sorted triangle: see pack_shade_records_kernel
    uint32_t n_tris;
    int32_t root;            // root node index, or a leaf code (< 0) for a single-triangle scene
    uint32_t n_qnodes;       // nodes in qnodes (breadth-first: the first ones are the top of the tree)
};

struct GiState {
    SceneView view{};
    const ShadeHeader* shade_heads = nullptr; // one per geometry, for gi_shade_kernel (the other kernels read view.geoms / view.mats)
    std::vector<void*> allocs;
    // host copies kept for the build
    std::vector<float> h_tris; // 12 floats per triangle
    float scene_min[3] = {0, 0, 0}, scene_max[3] = {0, 0, 0};
    uint32_t n_tris = 0, n_nodes = 0, bvh_depth = 0, build_passes = 0;
    float build_ms = 0.f; // wall time of the last successful neb_gi_build_bvh
    size_t texture_table_bytes = 0; // footprint tables + material bundles on the device
    uint32_t max_bvh_depth = 21; // (kLdsStack + kSpillStack) / 3: deeper trees are refused by neb_gi_build_bvh ("gi_max_bvh_depth" lowers it)
    bool built = false;
    unsigned long long* d_ray_counter = nullptr;
    neb_gi_hit* d_hits = nullptr;
    bool debug_hits = false;
    // What ONE dispatch of neb_gi_trace writes besides radiance[cur].  Two sets ("gi_defer_resolve" = 2): the GI stages of two frames may be in flight
    // on two streams, each on its own set; neb_gi_resolve retires them in the order they were traced.
    struct DispatchSet {
        float4* d_records = nullptr; // 5 float4 planes + one 4 x float4 record plane over the resident pixels (GiRecords)
        uint32_t* d_sort = nullptr;  // 4 x npx uint32: keys, vals, keys_out, vals_out
        void* d_sort_temp = nullptr;
        uint32_t* d_block_counts = nullptr; // [3][n_block_counts]: bounce rays / shadow rays / shadow rays answered by the sun table, per workgroup
        uint32_t* d_list = nullptr;  // [2][kListSegments] counters, then [kListSegments][cap] ray records
        uint32_t list_epoch = 0;     // shade launches so far: picks the counter set
        uint32_t pending_spp = 1, pending_row0 = 0, pending_row1 = 0;
        bool awaiting_resolve = false; // "gi_defer_resolve" = 1: this set's sums have not been added into radiance[cur] yet
        uint32_t resolve_seq = 0;      // ... and the order in which the sets were filled (neb_gi_resolve takes the oldest)
        neb_gi_constants split_c{}; // neb_gi_trace_begin's arguments, for its neb_gi_trace_finish
        uint32_t split_row0 = 0, split_row1 = 0;
    } sets[2];
    uint32_t resolve_seq = 0;
    uint32_t* d_tile_order = nullptr; // tuning: an explicit tile order for the closest-hit pass (neb_gi_debug_set_tile_order)
    uint32_t tile_order_n = 0, tile_order_cap = 0;
    uint32_t traces = 0, resolves = 0; // deferred dispatches issued / retired (set = count & 1 with two sets)
    uint32_t begun = 0, finished = 0;  // neb_gi_trace_begin / _finish calls (set = count & 1)
    uint32_t* d_direct_counts = nullptr; // neb_pbr_direct's own per-workgroup ray counts (it may run beside a GI dispatch)
    unsigned long long last_stats[16] = {};
    int defer_resolve = 0; // "gi_defer_resolve": 0 fused; 1 the indirect term waits in the records for neb_gi_resolve; 2 the same on two record sets
    bool exact_shade = false; // "gi_exact_shade": gi_shade_kernel<false>, the oracle's C arithmetic
    bool sort_shadow = true;  // "gi_sort_rays" bit 0
    bool sort_shadow_auto = true; // until "gi_sort_rays" is set: sort the shadow rays of dispatches of 1.5 M pixels and more only
    bool sort_bounce = false; // "gi_sort_rays" bit 1
    size_t sort_temp_bytes = 0;
    size_t n_block_counts = 0;
    // the sun-visibility table in the shading records (gi_sun_table.hip)
    bool sun_table = true;            // option "gi_sun_table"
    int sun_table_state = 0;          // 0: the records carry no flags; 1: flags of sun_table_key = this frame's sun; 2: flags of another sun (ignored)
    float sun_table_pending[4] = {0, 0, 0, 0}; // a new sun seen once: the table follows when it has been seen sun_hold times in a row
    // A build costs five frames' time and earns a tenth of a frame per dispatch: a table pays for itself after ~30 dispatches.  A new sun is built for when it
    // has held for TWO dispatches -- unless the table it replaces lived fewer than kSunTableLife dispatches (a sun that moves in steps: a build per step made
    // the frames twice as slow as no table at all), then for kSunHoldAfterShortLife.  "gi_sun_hold" = N pins the count (0 = this rule).
    uint32_t sun_hold = 2, sun_seen = 0, sun_table_age = 0;
    int sun_hold_option = 0;
    float sun_table_key[4] = {0, 0, 0, 0}; // {sunLightDirection, sunTanHalfAngle} the flags were built for
    unsigned long long* d_sun_counts = nullptr; // sides proven lit {+, -} by the last build
    uint32_t* d_sun_hint_list = nullptr;        // two-pass build: triangles whose primary side the first pass left unproven
    uint32_t sun_hint_list_cap = 0;
    uint32_t sun_table_builds = 0;
    // The flags are rewritten IN PLACE in the shading records, on the stream of the dispatch that noticed the new sun, while the host
    // state says "table valid" from the moment of the enqueue: a dispatch on ANOTHER stream ("gi_defer_resolve" = 2, or a host that
    // alternates streams) waits for this event first, or its shade pass could read the previous sun's lit bits of records the
    // 15-ms build has not reached yet.
    hipEvent_t sun_table_event = nullptr;   // recorded behind every launch that rewrites the flags
    hipEvent_t sun_build_ev[2] = {nullptr, nullptr}; // around the last build's two launches (neb_gi_sun_table_build_ms)
    hipStream_t sun_table_stream = nullptr; // ... on this stream
    bool sun_table_event_pending = false;   // not yet seen complete
    hipStream_t last_dispatch_stream = nullptr; // stream of the last dispatch that read the flags (a rewrite on another stream waits for the device)
    bool last_dispatch_stream_set = false;
    unsigned long long table_rays = 0; // shadow rays answered by the table as of the last neb_gi_ray_count
    int sun_hints = 4;                // option "gi_sun_hints": occluder hints the shade pass tries per hit (0, 2 or 4)
    bool compact_shadow = true;       // with the table on: the rays it leaves are compacted into lists by the shade pass ("gi_sun_table" = 2: off)
    // Which pass takes the rays the table leaves is MEASURED once per table build ("gi_sun_table" = 1, the default): the first dispatch with a new table
    // runs the compacted lists between two events, the second the sorted pass (same bits), a later one reads both times and keeps the faster -- the lists
    // win for most suns (0.51 against 0.58 ms of GI on the bench frame), the sorted pass where the table leaves many long rays (a sun straight overhead:
    // 0.79 against 0.92).  3 = always lists, 2 = always the sorted pass.
    bool tail_tune = true;
    int tail_phase = 0;               // 0 decided / nothing to decide, 1 time the lists next, 2 time the sorted pass next, 3 both enqueued: waiting for their events
    bool tail_sorted = false;         // the decision for this table
    hipEvent_t tail_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float tail_us[2] = {0.f, 0.f};    // the two times of the last measurement {lists, sorted pass}
    bool sun_table_stale = false;     // the flags in the records belong to a scene that has moved since (neb_gi_update_transforms): no sun brings them back
    // ---- moving submeshes: neb_gi_update_transforms (gi_refit.hip) ----
    // Host copies of what a transform is applied to (the build bakes h_tris from them again when a geometry is dirty) ...
    struct HostGeom {
        uint32_t firstIndex = 0, vertexBase = 0, n_tris = 0; // into h_indices / h_pos; triangles of the geometry
        uint32_t firstTri = 0;                               // its first triangle in h_tris (geometries follow one another)
        uint32_t firstRef = 0, n_refs = 0;                   // its referenced vertices (each once), into h_ref_verts
        uint32_t n_verts = 0;                                // numVertices of neb_gi_set_scene (neb_gi_update_vertices checks ranges against it)
        bool valid = false;                                  // DevGeom::valid: the normal and tangent pools hold data of this geometry
        float obj_lo[3] = {0, 0, 0}, obj_hi[3] = {0, 0, 0};  // object-space box of the referenced vertices
        float world_lo[3] = {0, 0, 0}, world_hi[3] = {0, 0, 0}; // exact world-space box under the current transform
        float m[16] = {};                                    // surfaceToWorld as last set
        bool dirty = false;                                  // h_tris still holds the bake of an earlier transform
        bool host_stale = false;                             // h_pos no longer holds the truth (neb_gi_update_vertices_device); cleared by a build
    };
    std::vector<HostGeom> h_geoms;
    std::vector<uint32_t> h_indices, h_ref_verts;
    std::vector<float> h_pos; // 3 per vertex, object space
    std::vector<uint32_t> h_seen; // per geometry: the update call that named it last (duplicate check without clearing)
    uint32_t seen_stamp = 0;
    // ... and on the device: the object-space positions, the 4x4 of every geometry, and two stamp arrays -- geom_epoch[g] == epoch:
    // geometry g was moved by the update in progress; node_epoch[i] == epoch: a child box of node i was rewritten by it.
    float* d_pos = nullptr; // (rewritten by neb_gi_update_vertices)
    float* d_xf = nullptr;
    uint32_t* d_geom_epoch = nullptr;
    uint32_t* d_node_epoch = nullptr; // (belongs to the tree: replaced by every build)
    uint32_t epoch = 0;               // updates enqueued so far
    std::vector<uint32_t> level_first; // breadth-first nodes: level l = [level_first[l], level_first[l + 1])
    // The arguments of an update wait in pinned host memory until its first kernel has read them: kStageSlots updates may be
    // enqueued before the host has to wait for the oldest one's kernel.
    static constexpr int kStageSlots = 4;
    struct StageEntry { uint32_t geom, pad[3]; float m[16]; };
    StageEntry* h_stage = nullptr;    // [kStageSlots][n_geoms]
    hipEvent_t stage_ev[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool stage_used[kStageSlots] = {false, false, false, false};
    // ---- deforming submeshes: neb_gi_update_vertices (gi_refit.hip) ----
    // One staged range of vertices: lanes [first_lane, first_lane + count) of deform_scatter_kernel write pool vertices dst ..;
    // the offsets are in floats from the start of the slot's data, kNoStream where the update keeps that attribute.
    struct DeformRange { uint32_t first_lane, count, dst, geom, pos_off, nrm_off, tan_off, pad; };
    static constexpr uint32_t kNoStream = 0xffffffffu;
    // The vertex data of an update waits in pinned host memory like the matrices of h_stage, in the same ring of kStageSlots slots under
    // the same events (slot = epoch % kStageSlots for either kind of update).  Allocated by the first update, grown to the largest seen.
    void* h_vstage = nullptr;         // [kStageSlots][vstage_cap bytes]: {DeformRange x n, padded to 16 B | positions | normals | tangents}
    size_t vstage_cap = 0;
    void* d_vstage = nullptr;         // "gi_deform_stage" = 1: the slot is copied here (one hipMemcpyAsync) and the scatter reads device memory
    size_t d_vstage_cap = 0;
    int deform_stage = 0;             // option "gi_deform_stage"
    // ---- device-sourced deformation, boxes reduced on the device: neb_gi_update_vertices_device (gi_refit.hip) ----
    // One source range of a device-sourced update, beside its DeformRange in the pinned slot: device pointers, strides in bytes.
    struct DeformSource { const uint8_t *pos, *nrm, *tan; uint32_t pos_stride, nrm_stride, tan_stride, pad; };
    // The boxes of a geometry whose h_pos is stale are reduced by geom_box_kernel over its referenced vertices: a device copy of
    // h_ref_verts and of every geometry's {firstRef, n_refs}, uploaded by the first call that needs them.
    uint32_t* d_ref_verts = nullptr;
    uint2* d_ref_spans = nullptr;
    // What such an update reports back, one slot of the ring per call: {call, refusal word, entries, 0} then 12 words per listed
    // geometry -- keys of refit_ordered, the upper bounds complemented so that all twelve are reduced with atomicMin:
    // {obj lo xyz, ~obj hi xyz, world lo xyz, ~world hi xyz}.  The chain ends with one copy d_result -> h_result and result_ev.
    static constexpr uint32_t kResultHead = 4, kResultEntry = 12;
    uint32_t* d_result = nullptr;     // [kStageSlots][kResultHead + kResultEntry * n_geoms]
    uint32_t* h_result = nullptr;     // pinned, same layout
    uint32_t* h_box_list = nullptr;   // pinned [kStageSlots][n_geoms]: the geometries of the slot's entries (geom_box_kernel reads it)
    hipEvent_t result_ev[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
    struct ResultRecord {
        bool used = false;            // enqueued, not harvested yet
        bool device_sourced = false;  // counts in neb_gi_update_status
        uint32_t call = 0;
        std::vector<uint32_t> geoms;  // entry e holds the boxes of geometry geoms[e]
    } result_rec[kStageSlots];
    uint64_t device_updates_accepted = 0, device_updates_refused = 0; // as harvested
    // ---- deforming submeshes under reprojection: option svgf_vertex_motion (gi_refit.hip) ----
    // While the option is on: the position and normal pools as they were when the most recent neb_gbuffer_raycast (or
    // neb_svgf_snapshot_vertices) ran, and one word per geometry that deform_scatter_kernel sets and deform_roll_kernel clears.
    // All three null with the option off: every kernel that takes them stores nothing then.
    float* d_pos_prev = nullptr;
    float* d_nrm_prev = nullptr;
    uint32_t* d_deform_dirty = nullptr;
    // per geometry, the union [x, y) of the vertex ranges (in the geometry's own numbering) passed to an update call since the last roll;
    // x >= y: none.  One span per geometry however many updates arrive.
    std::vector<uint2> roll_span;
    bool roll_pending = false;
    // One span of a roll in the pinned slot: lanes [first_lane, first_lane + count) copy pool vertices dst .. of geometry geom.
    struct RollSpan { uint32_t first_lane, count, dst, geom; };
    // ---- skinned submeshes: neb_gi_set_skin / neb_gi_skin_vertices (gi_refit.hip) ----
    // What neb_gi_set_skin keeps of a geometry, one device allocation of 64 bytes per vertex, every stream tight and 16-byte streams first:
    // {weights float4 | bind tangents float4 | joints uint16 x 4 | bind positions float3 | bind normals float3} x n_verts.
    struct Skin {
        void* d_block = nullptr;
        uint32_t n_joints = 0; // 0: the geometry has no skin
    };
    std::vector<Skin> skins;          // per geometry; empty until the first neb_gi_set_skin
    uint32_t n_skins = 0, skin_joints = 0; // bound geometries, the sum of their numJoints
    // One range of a skin call beside its DeformRange: the geometry's block and where its palette starts among the call's matrices.
    struct SkinSource { const uint8_t* block; uint32_t n_verts, pal_first, n_joints, attrs, pad[2]; };
    // The per-context palette buffer: what a skin call copies to the device in ONE hipMemcpyAsync from its pinned slot --
    // {DeformRange x n | SkinSource x n | 16 floats x the joints of the n geometries}.  Sized by neb_gi_set_skin for a call that names
    // every bound geometry (64 bytes of ranges + 64 bytes per joint: the geometry's share), so a skin call never allocates.
    // The morph calls copy their arguments into the same buffer: its capacity is args_capacity() below, whichever set-up call sizes it.
    void* d_skin_args = nullptr;
    size_t skin_args_cap = 0;
    // ---- morph targets: neb_gi_set_morph_targets / neb_gi_morph_vertices (gi_refit.hip) ----
    // What neb_gi_set_morph_targets keeps of a geometry, one device allocation, every stream tight, the 16-byte stream first:
    // {rest tangents float4 | rest positions float3 | rest normals float3} x n_verts, then target-major float3 streams:
    // position deltas [n_targets][n_verts], normal deltas likewise (has_n), tangent deltas likewise (has_t).
    struct Morph {
        void* d_block = nullptr;
        uint32_t n_targets = 0; // 0: the geometry has no targets
        bool has_n = false, has_t = false;
    };
    std::vector<Morph> morphs;        // per geometry; empty until the first neb_gi_set_morph_targets
    uint32_t n_morphs = 0, morph_targets = 0; // bound geometries, the sum of their numTargets
    // One range of a morph call beside its DeformRange: the geometry's block, its active list among the call's pairs, and -- where the
    // call skins it -- the block of its skin and where its palette starts among the call's matrices (n_joints == 0: not skinned).
    struct MorphSource {
        const uint8_t *block, *skin_block;
        uint32_t n_verts, n_targets, act_first, n_active, pal_first, n_joints, flags, pad;
    };
    static constexpr uint32_t kMorphAttrs = 1u, kMorphNormals = 2u, kMorphTangents = 4u; // MorphSource::flags
    struct MorphPair { uint32_t target; float weight; }; // one entry of an active list
    // A morph call copies {DeformRange x n | MorphSource x n | MorphPair x active, padded to 16 B | 16 floats x the joints of the skinned
    // ones} into d_skin_args in ONE hipMemcpyAsync.  The buffer serves both kinds of call, and both set-up calls size it by this one
    // formula from the four sums, so the order they come in does not matter: a skin call needs 64 bytes per bound skin and 64 per joint,
    // a morph call 80 bytes per geometry, 8 per target, at most 8 of padding, and the joints' share where it skins.
    static size_t args_capacity(uint32_t n_skins, uint32_t skin_joints, uint32_t n_morphs, uint32_t morph_targets)
    {
        return (size_t)64 * n_skins + (size_t)64 * skin_joints + (size_t)96 * n_morphs + (size_t)8 * morph_targets;
    }
    // Streams that have read triangles / nodes / geometry tables since the last update: an update on another stream orders itself
    // behind them (an event recorded on each, waited for on its own stream).  More than kReaderStreams: it waits for the device.
    static constexpr int kReaderStreams = 4;
    hipStream_t reader_streams[kReaderStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t reader_ev[kReaderStreams] = {nullptr, nullptr, nullptr, nullptr};
    int n_reader_streams = 0;
    bool reader_overflow = false;
    uint32_t n_geoms = 0;
    // ---- hidden submeshes: neb_gi_set_visibility (gi_refit.hip) ----
    // One word per geometry on the device (1 = visible) that rebake_kernel and refit_level_kernel read, and its host copy.  A hidden
    // geometry keeps its pools, its matrix and its boxes up to date; its triangle slots hold triangles no ray can hit, its leaves
    // inverted boxes.  neb_gi_set_scene makes everything visible, neb_gi_build_bvh keeps the flags.
    std::vector<uint8_t> h_visible;
    uint32_t* d_visible = nullptr;
    uint32_t n_hidden = 0;        // geometries with h_visible == 0
    bool nothing_visible = false; // no visible geometry has a triangle: the scene box is the zero box, no sun table is built
    // ---- materials and texels in place: neb_gi_update_materials / _set_geometry_materials / _update_textures (gi_material.hip) ----
    // What neb_gi_set_scene decided about the tables, kept for the update calls (the raw images are gone): host copies of the DevMat rows,
    // of DevGeom::material and of the DevTex rows (offset 0xffffffff: no standalone table), and per texture the bundles it sits in -- the
    // uses of texture t are tex_uses[tex_use_first[t] .. tex_use_first[t + 1]).
    struct TexUse { uint32_t material, bundle /* first entry, 32-byte units */, roles /* texpatch::kRole* */; };
    std::vector<DevMat> h_mats;
    std::vector<int32_t> h_geom_mat;
    std::vector<DevTex> h_texs;
    std::vector<TexUse> tex_uses;
    std::vector<uint32_t> tex_use_first;
    std::vector<uint32_t> h_mat_seen; // per material, as h_seen per geometry
    size_t table_bytes = 0, bundle_bytes = 0; // the two parts of texture_table_bytes
    // One staged entry of a factor update (index = material) or of a reassignment (index = geometry, material = the new one).
    struct MatStage { uint32_t index; int32_t material; float albedo[3]; float rough, metal; uint32_t pad; };
    // [n_mats] then [n_geoms] stamps: == epoch where the update in progress wrote the row.  Allocated by the first such call.
    uint32_t* d_mat_epoch = nullptr;
    // Host-sourced texel updates: the pinned slot is copied here in one hipMemcpyAsync and the patch kernels read device memory (every
    // texel is read by four lanes, and by every use of its texture).  Allocated by the first call, grown to the largest seen.
    void* d_tstage = nullptr;
    size_t d_tstage_cap = 0;
    // ---- the caller's rays: neb_gi_cast_rays with NEB_RAYS_SORT (gi_query.hip) ----
    // One grow-only block {keys | indices | their ping-pong partners, n words each | ray_sort_scratch_bytes(n)}: every sorted call of
    // the context uses it, so they run one after the other -- a sorted call records query_ev behind its last kernel, a sorted call on
    // another stream waits for it on the device, and growing waits for it on the host before the block is freed.  Unsorted calls use
    // none of this.  Freed by gi_destroy (neb_gi_set_scene, neb_destroy), kept across neb_gi_build_bvh.
    void* d_query_sort = nullptr;
    size_t query_sort_cap = 0;
    hipEvent_t query_ev = nullptr;
    hipStream_t query_stream = nullptr; // the stream query_ev was recorded on
    bool query_ev_pending = false;
};
// ---- what every update call does with the ring and with its streams (gi_refit.hip) ----
// An update takes slot call % kStageSlots of the pinned rings once that slot's last user has read it (stage_slot_acquire), orders its
// stream behind every reader of what it rewrites (refit_order_behind_readers), commits g->epoch = call, lets the slot go behind the last
// command that reads it (stage_slot_release) and ends with mark_rewrite.  The geometry updates of gi_refit.hip go through this as
// update_begin ... update_finish there, which add the result record and the rewrite of the tree; gi_material.hip calls the parts.
hipError_t vstage_reserve(GiState* g, size_t bytes, size_t want);
hipError_t stage_slot_acquire(GiState* g, uint32_t call, int* slot);
hipError_t stage_slot_release(GiState* g, int slot, hipStream_t stream);
bool device_readable(const neb_ctx* ctx, const void* p, size_t bytes);
int refit_order_behind_readers(neb_ctx* ctx, GiState* g, hipStream_t stream);
hipError_t gi_sun_table_update(GiState* g, const neb_gi_constants& c, hipStream_t stream);
hipError_t gi_sun_table_order(GiState* g, hipStream_t stream);
hipError_t mark_rewrite(GiState* g, hipStream_t stream);
hipError_t gi_quantise_nodes(const Bvh4Node* nodes, uint32_t n, Bvh4NodeQ* out, hipStream_t stream);
void gi_rebake_host(GiState* g);
// The end of neb_gi_build_bvh with hidden geometries: their slots emptied and the tree refitted on `stream` (enqueue only).
hipError_t gi_visibility_after_build(GiState* g, hipStream_t stream);
// the scene box over the visible geometries (over all of them: the box the build sorts by)
void gi_fold_scene_box(const GiState* g, bool visible_only, float lo[3], float hi[3]);
// Applies the result records of finished updates in call order: boxes of the listed geometries, then the scene box.  block = false
// stops at the first record whose event has not passed; block = true waits for every record of a call <= upto.
hipError_t gi_harvest_results(GiState* g, bool block, uint32_t upto = 0xffffffffu);

// Every entry point that reads triangles, nodes or the geometry tables on `stream` starts here: a rewrite enqueued on another stream
// (sun table, neb_gi_update_transforms) comes first, and the stream is remembered for the next update to wait for.
inline hipError_t gi_scene_reader(GiState* g, hipStream_t stream)
{
    bool known = false;
    for (int k = 0; k < g->n_reader_streams; ++k)
        known = known || g->reader_streams[k] == stream;
    if (!known) {
        if (g->n_reader_streams < GiState::kReaderStreams)
            g->reader_streams[g->n_reader_streams++] = stream;
        else
            g->reader_overflow = true;
    }
    return gi_sun_table_order(g, stream);
}

// world = (p, 1) * M, row-vector convention: THE operation order of the bake -- products and sums rounded one by one, left to right.
// rebake_kernel (gi_refit.hip) repeats it with __fmul_rn / __fadd_rn and must give the same bits.  false: not a finite position.
inline bool gi_bake_point(const float* m, const float a[3], float w[3])
{
#pragma clang fp contract(off)
    w[0] = a[0] * m[0] + a[1] * m[4] + a[2] * m[8] + m[12];
    w[1] = a[0] * m[1] + a[1] * m[5] + a[2] * m[9] + m[13];
    w[2] = a[0] * m[2] + a[1] * m[6] + a[2] * m[10] + m[14];
    return fabsf(w[0]) <= 3.0e38f && fabsf(w[1]) <= 3.0e38f && fabsf(w[2]) <= 3.0e38f;
}

void gi_on_resize(GiState* g);
void gi_destroy(GiState* g);

} // namespace neb

// ---- host helpers of the C ABI entry points ----
static inline int gi_fail(neb_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
    else
        snprintf(buf, sizeof(buf), "%s", what);
    ctx->last_error = buf;
    return code;
}

#define GI_HIP(ctx, call)                                   \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess)                               \
            return gi_fail((ctx), NEB_ERR_HIP, #call, e_);  \
    } while (0)

// scoped: run the rest of the entry point on the context's device, restore the caller's device on return
#define GI_GUARD(ctx)                                                        \
    neb::DeviceGuard gi_guard_((ctx)->device);                               \
    if (gi_guard_.err != hipSuccess)                                         \
    return gi_fail((ctx), NEB_ERR_HIP, "hipSetDevice", gi_guard_.err)

template <typename T>
static inline hipError_t upload(neb::GiState* g, const std::vector<T>& h, const T** out)
{
    *out = nullptr;
    if (h.empty())
        return hipSuccess;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, h.size() * sizeof(T));
    if (e != hipSuccess)
        return e;
    g->allocs.push_back(d);
    *out = (const T*)d;
    return hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}
