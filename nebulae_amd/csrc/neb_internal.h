// neb_internal.h -- context layout and kernel launchers behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/nebulae_hip.h"

namespace neb {

struct PlaneInfo {
    uint32_t bytes_per_px;
    uint32_t slots;
};
// the reference-format planes of the enum, and behind them NEB_PLANE_SUBMESH_ID, NEB_PLANE_PREV_POINT and NEB_PLANE_DEMOD (not counted by
// NEB_PLANE_COUNT)
constexpr int kPlaneSlots = NEB_PLANE_COUNT + 3;
extern const PlaneInfo kPlaneInfo[kPlaneSlots];

// Every entry point that launches or copies runs on its context's device whatever device the calling thread had
// current, and leaves the thread's current device as it found it (a host may hold strip contexts on several GPUs).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        if (prev != device)
            err = hipSetDevice(device);
        else
            prev = -1; // nothing to restore
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Per-pass profiler ranges with the reference's PIX event names (NEB_PIX_SCOPED_EVENT, src/nri/PIXRuntime.h:115-117;
// uses at src/DeferredRenderer.cpp:267,338,434,567,599 and src/SVGFDenoiser.cpp:69,136,155): roctx ranges, resolved at
// run time from the ROCm profiler's marker library (no-ops when it is absent); rocprofv3 --marker-trace shows them.
void marker_push(const char* name);
void marker_pop();
struct ScopedRange {
    explicit ScopedRange(const char* name) { marker_push(name); }
    ~ScopedRange() { marker_pop(); }
    ScopedRange(const ScopedRange&) = delete;
    ScopedRange& operator=(const ScopedRange&) = delete;
};

struct SvgfLaunch {
    int device;            // HIP device ordinal of the context (per-device kernel attributes)
    uint32_t W, H;         // full image size (global clamp uses these)
    uint32_t row_begin;    // first resident image row: plane address of (x, y) is (y - row_begin) * W + x
    uint32_t row_end;      // one past the last resident row
    uint32_t row0, row1;   // image rows to process
    int num_cus;           // persistent-grid sizing
    neb_svgf_params p;
};

// Kernel launchers (enqueue only).  All pointers are device pointers to resident row `row_begin`.
hipError_t launch_temporal(const SvgfLaunch& L, float4* rad_cur, const float4* rad_hist, const uint32_t* depth_cur,
                           const uint32_t* depth_hist, const uint2* normal_cur, const uint2* normal_hist,
                           const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance, float4* geometry, hipStream_t s,
                           const uint32_t* demod_albedo = nullptr);
// (demod_albedo, here and on the reprojecting launchers: option svgf_demodulate -- NEB_PLANE_ALBEDO; the pixel's own radiance is divided by its
// divisor on load and rad_hist is NEB_PLANE_DEMOD.  Null: the pass as it is without the option.)

// `geometry`: {decoded shading normal.xyz, depth} per pixel (NEB_PLANE_GEOMETRY), valid for every tap row.
// variant 0 = direct-load kernel, 1 = LDS row-lattice kernel (steps <= 32; wider steps take the direct kernel)
hipError_t launch_atrous(const SvgfLaunch& L, int variant, uint32_t step, const float4* src, float4* dst,
                         const uint16_t* variance, const float4* geometry, hipStream_t s);
// Option svgf_demodulate, the level whose destination is the chain's result: the same filter, the filtered colour unmodulated into `demod_out`
// (NEB_PLANE_DEMOD) and times the output pixel's divisor (svgf_demod.h; `albedo` = NEB_PLANE_ALBEDO) into dst
hipError_t launch_atrous_remodulate(const SvgfLaunch& L, int variant, uint32_t step, const float4* src, float4* dst, const uint16_t* variance,
                                    const float4* geometry, const uint32_t* albedo, float4* demod_out, hipStream_t s);
// true when launch_atrous(L, variant, step, ...) runs the LDS kernel (what the whole-frame fast path below requires of every level)
bool atrous_lds_serves(const SvgfLaunch& L, int variant, uint32_t step);
// Whole-frame denoise, levels after the first: src holds {r, g, b, lum} (written by the level before); dst gets {r, g, b, lum},
// or -- last -- {r, g, b, alpha} with the alpha dst itself holds (radiance[cur] = the frame's input until that store)
hipError_t launch_atrous_lum(const SvgfLaunch& L, uint32_t step, bool last, const float4* src, float4* dst, const uint16_t* variance,
                             const float4* geometry, hipStream_t s);
// Whole-frame denoise, level 0 with the temporal pass as its staging phase: reads the frame's planes, writes moments[cur],
// variance, the geometry plane and the filtered level-0 radiance ({r, g, b, lum}; {r, g, b, alpha} when it is the only level) to dst
hipError_t launch_atrous_fused_temporal(const SvgfLaunch& L, bool only_level, const float4* rad_cur, const float4* rad_hist, const uint32_t* depth_cur,
                                        const uint32_t* depth_hist, const uint2* normal_cur, const uint2* normal_hist, const uint32_t* mom_hist,
                                        uint32_t* mom_cur, uint16_t* variance, float4* geometry, float4* dst, hipStream_t s);
// Option svgf_demodulate: the stand-in history where NEB_PLANE_DEMOD does not hold the last denoised frame -- over the n resident pixels,
// demod[i].rgb = rad_hist[i].rgb / divisor(albedo[i])
hipError_t launch_demod_seed(const float4* rad_hist, const uint32_t* albedo, float4* demod, size_t n, hipStream_t s);
// A camera as neb_gbuffer_raycast's kernel uses it: eye, the view axes (z points from the target to the eye), tan(vfov / 2), aspect and
// the two depth-mapping entries of XMMatrixPerspectiveFovRH.  One host function builds it for the G-buffer producer and for the
// reprojecting temporal pass, so that both see the same float bits.
struct CameraBasis {
    float eye[3], xaxis[3], yaxis[3], zaxis[3];
    float tan_half, aspect, m22, m32;
};
inline CameraBasis camera_basis(const neb_camera& cam, uint32_t W, uint32_t H)
{
    auto norm = [](float* v) {
        const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] /= l;
        v[1] /= l;
        v[2] /= l;
    };
    CameraBasis b;
    float z[3] = {cam.eye[0] - cam.target[0], cam.eye[1] - cam.target[1], cam.eye[2] - cam.target[2]};
    norm(z);
    float x[3] = {cam.up[1] * z[2] - cam.up[2] * z[1], cam.up[2] * z[0] - cam.up[0] * z[2], cam.up[0] * z[1] - cam.up[1] * z[0]};
    norm(x);
    const float y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    for (int k = 0; k < 3; ++k) {
        b.eye[k] = cam.eye[k];
        b.xaxis[k] = x[k];
        b.yaxis[k] = y[k];
        b.zaxis[k] = z[k];
    }
    b.tan_half = tanf(cam.vfov_deg * (3.14159265f / 180.0f) * 0.5f);
    b.aspect = (float)W / (float)H;
    b.m22 = cam.zfar / (cam.znear - cam.zfar); // XMMatrixPerspectiveFovRH
    b.m32 = cam.znear * cam.zfar / (cam.znear - cam.zfar);
    return b;
}

// Reprojecting temporal pass (option svgf_reproject, whole-frame contexts): see neb_svgf_set_camera in nebulae_hip.h.
// cam_hist == nullptr: no camera for the history slot -- the pass takes no history.
hipError_t launch_temporal_reproject(const SvgfLaunch& L, const CameraBasis& cam_cur, const CameraBasis* cam_hist, float4* rad_cur,
                                     const float4* rad_hist, const uint32_t* depth_cur, const uint32_t* depth_hist, const uint2* normal_cur,
                                     const uint2* normal_hist, const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance,
                                     const uint8_t* hlen_hist, uint8_t* hlen_cur, float4* geometry, hipStream_t s,
                                     const uint32_t* demod_albedo = nullptr);

// Option svgf_motion: the motion arm of the same kernel (svgf_temporal_reproject_kernel<ReprojMode::Submesh>) -- id planes of the two slots, and
// the per-geometry delta table launch_reproj_delta wrote in front of it (n_delta = 0: nothing moved between the two snapshots).
struct ReprojMotion {
    const uint32_t* id_cur;
    const uint32_t* id_hist;
    const float4* delta; // n_delta entries of kReprojDeltaFloat4 float4 (svgf_reproject.h)
    uint32_t n_delta;
    // Option svgf_vertex_motion: NEB_PLANE_PREV_POINT, {P_h.xyz, oct16(N_h) | kReprojNoPrevPoint} per pixel.  Non-null picks the third arm
    // of the kernel (ReprojMode::Vertex), which takes P and the geometric normal from it where .w is not the sentinel.
    const float4* prev_point = nullptr;
    // Option svgf_demodulate: NEB_PLANE_ALBEDO (set by the launcher from its demod_albedo; picks the ...Demod mode of the arm)
    const uint32_t* demod_albedo = nullptr;
};
hipError_t launch_temporal_reproject_motion(const SvgfLaunch& L, const CameraBasis& cam_cur, const CameraBasis* cam_hist, float4* rad_cur,
                                            const float4* rad_hist, const uint32_t* depth_cur, const uint32_t* depth_hist, const uint2* normal_cur,
                                            const uint2* normal_hist, const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance,
                                            const uint8_t* hlen_hist, uint8_t* hlen_cur, float4* geometry, const ReprojMotion& motion, hipStream_t s,
                                            const uint32_t* demod_albedo = nullptr);
// one lane per geometry: the two slots' 4x4 tables (n x 16 floats, row-vector convention) -> n delta entries
hipError_t launch_reproj_delta(const float* xf_cur, const float* xf_hist, float4* delta, uint32_t n, hipStream_t s);

// decodes depth / normal rows [row0, row1) (all W columns) into the geometry plane
hipError_t launch_decode_geometry(uint32_t W, uint32_t row_begin, uint32_t row0, uint32_t row1, const uint32_t* depth, const uint2* normal,
                                  float4* geometry, hipStream_t s);
hipError_t launch_decode_geometry2(uint32_t W, uint32_t row_begin, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, const uint32_t* depth,
                                   const uint2* normal, float4* geometry, hipStream_t s);

// raysort.hip: stable LSD radix sort of (key, value) pairs on key bits [0, bits), bits <= 16 (enqueue only)
size_t ray_sort_scratch_bytes(size_t n);
hipError_t ray_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp, uint32_t* vals_out, size_t n, int bits,
                          void* scratch, hipStream_t stream);

// A neb_svgf_temporal call on a whole-frame context is held back until the neb_svgf_atrous call that normally follows it
// (they then run as one fused chain); every other entry point that reads, writes or orders work on the planes calls this
// first, which submits the held-back pass on its own (the stand-alone kernel) -- NEB_OK or the failing status.
int svgf_flush_pending(neb_ctx* ctx);

struct GiState;               // gi.hip / gi_build.hip: scene tables, BVH, counters
void gi_destroy(GiState* g);
void gi_on_resize(GiState* g);
int gi_set_debug_hits(neb_ctx* ctx, int on);
int gi_set_defer_resolve(neb_ctx* ctx, int on);
int gi_set_sort_rays(neb_ctx* ctx, int mask);
int gi_set_max_bvh_depth(neb_ctx* ctx, int depth);
int gi_set_exact_shade(neb_ctx* ctx, int on);
int gi_set_sun_table(neb_ctx* ctx, int on);
int gi_set_sun_hints(neb_ctx* ctx, int n);
int gi_set_sun_hold(neb_ctx* ctx, int n);
int gi_set_deform_stage(neb_ctx* ctx, int mode);
// option svgf_motion (gi.hip): the two per-slot transform tables and the delta table exist while the option is on and a scene is set
int gi_motion_tables_alloc(neb_ctx* ctx); // NEB_OK also without a scene (nothing to allocate); forgets both snapshots
void gi_motion_tables_free(neb_ctx* ctx);
int gi_snapshot_transforms(neb_ctx* ctx, int s, hipStream_t stream); // s = 0 / 1, resolved
// option svgf_vertex_motion (gi_refit.hip): the previous position / normal pools and the per-geometry dirty words exist while the option
// is on and a scene is set
int gi_vertex_motion_alloc(neb_ctx* ctx); // NEB_OK also without a scene (nothing to allocate); the pools start as copies of the live ones
void gi_vertex_motion_free(neb_ctx* ctx);
int gi_roll_vertices(neb_ctx* ctx, hipStream_t stream); // live -> previous for the vertex spans updated since the last roll; enqueue only

} // namespace neb

struct neb_ctx {
    int device = 0;
    int num_cus = 256; // hipDeviceProp_t::multiProcessorCount (persistent-grid sizing)
    uint32_t W = 0, H = 0, row_begin = 0, row_end = 0, levels = 4;
    void* planes[neb::kPlaneSlots][2] = {};
    int cur = 0, hist = 1;
    uint32_t geom_lo = 0, geom_hi = 0; // image rows [geom_lo, geom_hi) of the geometry plane hold this frame's decoded normal / depth
    neb_svgf_params params{};
    int atrous_variant = 1; // 0 = direct-load kernel, 1 = LDS row-lattice kernel
    int fuse = 0;           // option svgf_fuse (opt-in): hold neb_svgf_temporal of a whole frame back so that neb_svgf_atrous can run both as the fused chain
    bool pending_temporal = false; // a neb_svgf_temporal held back for the fused chain
    hipStream_t pending_stream = nullptr;
    int profile = 0;                   // option svgf_profile: neb_svgf_atrous brackets its kernels with events (neb_svgf_level_times)
    std::vector<hipEvent_t> prof_events; // levels + 1 of them once profiling has run
    uint32_t prof_recorded = 0;
    int reproject = 0;                 // option svgf_reproject: the temporal pass reprojects (planes[NEB_PLANE_HISTORY_LENGTH] exist only then)
    neb_camera cams[2] = {};           // neb_svgf_set_camera / neb_gbuffer_raycast: the camera each slot's depth / normal planes were rendered with
    bool has_cam[2] = {false, false};
    int motion = 0;                    // option svgf_motion: the temporal pass follows moved submeshes (planes[NEB_PLANE_SUBMESH_ID] exist only then)
    float* xf_snap[2] = {nullptr, nullptr}; // neb_svgf_snapshot_transforms: the 4x4 table each slot's G-buffer was rendered with (n_geoms x 16)
    bool has_snap[2] = {false, false};
    uint32_t snap_epoch[2] = {0, 0};   // updates enqueued before the snapshot: equal for both slots = nothing moved between them
    float4* motion_delta = nullptr;    // reproj_delta_kernel's output, n_geoms entries
    uint32_t motion_geoms = 0;         // geometries the three tables were sized for
    // option svgf_demodulate: albedo divided out in front of the temporal pass, multiplied back at the last level (planes[NEB_PLANE_DEMOD] exists
    // only then: the demodulated denoised colour = the temporal pass's history).  The plane is valid for a temporal call iff it matches
    // radiance[hist]: written by the last level in the bracket before (or seeded in this one) for the slot that is now hist.
    int demod = 0;
    uint64_t frame_serial = 0;         // neb_begin_frame calls so far
    uint64_t demod_serial = 0;         // the bracket in which the last level wrote the demod plane, or the seed kernel did
    int demod_slot = -1;               // the radiance slot whose image it then held demodulated (-1: none -- uploads, reset_history, resize)
    uint32_t demod_seeds = 0;          // seed launches since option svgf_profile was last set (neb_svgf_level_times reports it)
    int vertex_motion = 0;             // option svgf_vertex_motion: the temporal pass follows deformed submeshes (planes[NEB_PLANE_PREV_POINT] exists only then)
    neb::GiState* gi = nullptr;
    // neb_strip_frame* (strips.hip): a side stream for the halo exchange beside level 0, and the events that order it -- created on first use
    struct StripSync {
        hipStream_t xstream = nullptr;
        hipEvent_t ready = nullptr, done = nullptr; // launch stream -> side stream, side stream -> launch stream
        hipEvent_t pushed = nullptr;                // local transport: this strip's boundary rows are in its neighbours' halos
        hipEvent_t frame_done = nullptr;            // ... this strip's frame has been enqueued to its end (its halo rows may be overwritten after it)
        bool frame_done_recorded = false;
        hipEvent_t inputs = nullptr;                // ... what its stream holds up to its neb_strip_frame_begin of this frame (a push into its rows from another stream waits for it)
        hipStream_t stream = nullptr;               // the stream of that call: a neighbour that begins later enqueues this strip's push into it there
        bool begun = false;                         // between this frame's neb_strip_frame_begin and _finish (neb_begin_frame clears it)
        bool linked[2] = {false, false};            // [0] up, [1] down: both pushes across that edge are enqueued for this frame
    } strip;
    std::string last_error;
};
