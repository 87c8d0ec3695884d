/*
 * nebulae_hip.h -- C ABI of libnebulae_hip.so: the MI355X (gfx950) back end for the
 * ray-traced GI + SVGF hot path of KatanaMajesty/Nebulae.
 *
 * The reference has no plugin/FFI interface; the seam is the set of calls that
 * Renderer/DeferredRenderer make on SVGFDenoiser and on DeferredRenderer's GI
 * methods.  Each entry point below names the reference member it replaces
 * (paths relative to the reference checkout).  D3D12 command lists become HIP
 * streams: every neb_* "submit" call only ENQUEUES work on the given stream and
 * never synchronises, exactly as the reference records into a command list.
 *
 * Conventions: plain pointers and sizes only; every function returns
 * NEB_OK (0) or a negative neb_status, never throws; neb_last_error() gives
 * the message for the last failure on that context (the reference throws
 * HrException / asserts instead, src/nri/stdafx.h:31-98).  A context is not
 * thread-safe: the caller serialises, as the reference's single render thread does;
 * different contexts may be driven from different threads at the same time (tests/test_soak_gpu.py).
 */
#ifndef NEBULAE_HIP_H
#define NEBULAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct neb_ctx neb_ctx;
typedef void* neb_stream; /* hipStream_t (NULL = the null stream) */

typedef enum neb_status {
    NEB_OK = 0,
    NEB_ERR_INVALID_ARG = -1,
    NEB_ERR_HIP = -2,
    NEB_ERR_NO_DEVICE = -3,
    NEB_ERR_STATE = -4,
    NEB_ERR_OUT_OF_RANGE = -5
} neb_status;

/* Device-resident planes.  Formats are the reference's DXGI formats, stored
 * linear, row-major, pitch == width (src/SVGFDenoiser.h:160-168,
 * src/DeferredRenderer.cpp:758-770). */
typedef enum neb_plane {
    NEB_PLANE_RADIANCE = 0,    /* R32G32B32A32_FLOAT 16 B/px, 2 slots (SVGFDenoiser.h:143)       */
    NEB_PLANE_NORMAL = 1,      /* R16G16B16A16_FLOAT  8 B/px, 2 slots; .xy oct GN, .zw oct SN     */
    NEB_PLANE_DEPTH = 2,       /* R24G8               4 B/px, 2 slots; D24_UNORM | stencil << 24  */
    NEB_PLANE_MOMENTS = 3,     /* R16G16_FLOAT        4 B/px, 2 slots; (<Y>, <Y^2>)               */
    NEB_PLANE_VARIANCE = 4,    /* R16_FLOAT           2 B/px, 1 slot                              */
    NEB_PLANE_SCRATCH = 5,     /* R32G32B32A32_FLOAT 16 B/px, 1 slot (reference: m_denoisedOutput) */
    NEB_PLANE_ALBEDO = 6,      /* R11G11B10_FLOAT     4 B/px, 1 slot (G-buffer, GI input)         */
    NEB_PLANE_ROUGH_METAL = 7, /* R16G16_FLOAT        4 B/px, 1 slot                              */
    NEB_PLANE_WORLDPOS = 8,    /* R16G16B16A16_FLOAT  8 B/px, 1 slot                              */
    NEB_PLANE_LDR = 9,         /* R8G8B8A8_UNORM      4 B/px, 1 slot (tonemapped back buffer, row f3) */
    NEB_PLANE_GEOMETRY = 10,   /* R32G32B32A32_FLOAT 16 B/px, 1 slot: {decoded shading normal.xyz, depth in [0,1]} of the current frame.
                                  No reference counterpart: the temporal pass decodes normal[cur] / depth[cur] once per frame and the
                                  a-trous levels read this instead of decoding them five times (read-only for callers). */
    NEB_PLANE_HISTORY_LENGTH = 11, /* R8_UINT 1 B/px, 2 slots: frames of valid history per pixel, saturating at 255.  No reference
                                      counterpart: exists only while option "svgf_reproject" is 1 (see neb_svgf_set_camera);
                                      neb_get_plane / uploads / downloads of it return NEB_ERR_STATE otherwise. */
    NEB_PLANE_COUNT = 12
} neb_plane;
/* R32_UINT 4 B/px, 2 slots: the geometry index (submesh) of each pixel's primary hit, 0xFFFFFFFF where depth holds no surface.  Not one
 * of the reference-format planes, not counted by NEB_PLANE_COUNT: exists only while option "svgf_motion" is 1 (allocated zeroed, freed
 * when the option is turned off, re-created by neb_resize); neb_get_plane / uploads / downloads of it return NEB_ERR_STATE otherwise.
 * neb_gbuffer_raycast writes slot cur; a host with its own raster G-buffer uploads or writes it. */
#define NEB_PLANE_SUBMESH_ID 12
/* R32G32B32A32 16 B/px, ONE slot: per-vertex motion for the reprojecting temporal pass.  .xyz = the world point (fp32)
 * where the surface point this pixel shows was when the PREVIOUS G-buffer was rendered; .w as uint32 = that point's previous geometric
 * normal in the oct16 pair encoding of the normal plane's .xy (low half x, high half y).  .w == 0xFFFFFFFF (no encoded normal gives that
 * word): no per-vertex motion for this pixel, the per-submesh rule of "svgf_motion" applies.  Behind the enum like the id plane: exists
 * only while option "svgf_vertex_motion" is 1 (allocated with every byte 0xFF -- every pixel the sentinel -- freed with the option,
 * re-created so by neb_resize).  neb_gbuffer_raycast
 * writes it; a host with its own raster G-buffer uploads or writes it.  While the option is 0 every plane entry point refuses index 13
 * with NEB_ERR_INVALID_ARG, the answer the index had before the option existed. */
#define NEB_PLANE_PREV_POINT 13
/* R32G32B32A32_FLOAT 16 B/px, ONE slot: the DEMODULATED denoised colour of the last denoised frame (.w unspecified) -- the temporal pass's
 * history while option "svgf_demodulate" is 1, see the block above neb_svgf_set_camera.  Behind the enum like the two planes above:
 * exists only while the option is 1 (allocated zeroed, freed with the option, re-created zeroed by neb_resize).  While the option is 0
 * every plane entry point refuses index 14 with NEB_ERR_INVALID_ARG, the answer an unknown plane index gets. */
#define NEB_PLANE_DEMOD 14

/* Slot selectors for the 2-slot (ping-pong) planes. */
#define NEB_SLOT_CURRENT (-1) /* GetCurrentResourceIndex(), SVGFDenoiser.h:24 */
#define NEB_SLOT_HISTORY (-2) /* GetHistoryResourceIndex(), SVGFDenoiser.h:25 */

typedef struct neb_create_info {
    int32_t device;        /* HIP device ordinal */
    uint32_t width;        /* full image width  (SVGFDenoiser::Init, SVGFDenoiser.h:16) */
    uint32_t height;       /* full image height */
    uint32_t row_begin;    /* first image row resident in this context (0 on one GPU) */
    uint32_t row_end;      /* one past the last resident row (0 = height).  Multi-GPU row strips
                              keep [row_begin,row_end) = owned rows + halo rows; see DESIGN.md */
    uint32_t atrous_levels; /* NumAtrousPasses, SVGFDenoiser.h:199 (reference: 4) */
} neb_create_info;

/* SVGFTemporalConstants + SVGFAtrousConstants tunables (SVGFDenoiser.h:76-92);
 * resolution/step are filled in per dispatch as in SVGFDenoiser.cpp:74-75,158-160. */
typedef struct neb_svgf_params {
    float depthSigma;  /* 0.002  */
    float alpha;       /* 0.9    */
    float varianceEps; /* 1e-4   */
    float phiColor;    /* 4/255  */
    float phiNormal;   /* 128    */
    float phiDepth;    /* 0.002  */
} neb_svgf_params;

/* ---- lifecycle: SVGFDenoiser::Init / Resize (SVGFDenoiser.cpp:14-37), DeferredRenderer::Init ---- */
int neb_create(const neb_create_info* info, neb_ctx** out_ctx);
int neb_resize(neb_ctx* ctx, uint32_t width, uint32_t height); /* re-creates (zeroes) all planes */
int neb_destroy(neb_ctx* ctx);
const char* neb_last_error(const neb_ctx* ctx); /* ctx may be NULL: last creation error */
const char* neb_version(void);

/* ---- profiler ranges: NEB_PIX_SCOPED_EVENT (src/nri/PIXRuntime.h:115-117) becomes a roctx range.  Every submit call below
 * brackets itself with the reference's event name ("SVGF: Temporal Accumulation", "SVGF: A-Trous compute i (step s)", ...);
 * these two let the host add its own enclosing ranges ("SVGF Denoising", DeferredRenderer.cpp:599).  No-ops without a
 * ROCm marker library; rocprofv3 --marker-trace records them. ---- */
int neb_marker_push(const char* name);
int neb_marker_pop(void);

/* ---- per-frame bracket: SVGFDenoiser::BeginFrame/EndFrame (SVGFDenoiser.cpp:39-47) ---- */
int neb_begin_frame(neb_ctx* ctx, uint32_t frame_index); /* cur = f & 1, hist = cur ^ 1 */
int neb_end_frame(neb_ctx* ctx);
int neb_current_index(const neb_ctx* ctx);
int neb_history_index(const neb_ctx* ctx);

/* ---- tunables: GetTemporalConstants()/GetATrousConstants() (SVGFDenoiser.h:83,93) ---- */
int neb_svgf_default_params(neb_svgf_params* out);
int neb_svgf_set_params(neb_ctx* ctx, const neb_svgf_params* p);
int neb_svgf_get_params(const neb_ctx* ctx, neb_svgf_params* out);
/* Implementation knobs with no reference counterpart (A/B arms for profiling):
 *   "atrous_variant": 1 = LDS row-lattice kernel (default; 4 rows per lane for steps <= 4, 2 for steps 8..32; wider steps take the
 *                     direct kernel), 0 = direct-load kernel;
 *   "gi_debug_hits":  1 = neb_gi_trace also records a neb_gi_hit per pixel (needs a scene);
 *   "gi_sort_rays":   mask, bit 0 = radix-sort the shadow rays by origin Morton code before tracing them (until the option is set:
 *                     on for dispatches of 1.5 M pixels and more, off for smaller ones, where the sort costs more than it saves),
 *                     bit 1 = sort the bounce rays by direction octant + origin (default off);
 *   "gi_defer_resolve": 1 = neb_gi_trace leaves the frame's indirect term in its records; neb_gi_resolve adds it;
 *                       2 = the same on TWO sets of records, used alternately: a second neb_gi_trace (the next frame's, on another stream)
 *                       may be issued and run before the first one's neb_gi_resolve has executed; neb_gi_resolve retires the dispatches in
 *                       the order they were traced.  The caller orders the streams: a trace must not start before the resolve that read
 *                       its set (two traces earlier) has finished, a resolve not before its own trace has;
 *   "gi_exact_shade":   1 = hit shading in the C arithmetic of the CPU oracle (IEEE division, sqrt, powf, sinf / cosf) instead of
 *                       the 1-ulp hardware forms an HLSL compiler emits (default).  The two differ by ~1e-7 relative, except where the
 *                       BRDF itself is ill-conditioned (mirror-like roughness: the GGX denominator cancels), where it can be percents;
 *   "gi_sun_table":     1 (default) / 0: answer the sun-visibility query of a hit from the per-triangle table where it is proven
 *                       (neb_gi_sun_table_stats) instead of tracing the shadow ray, and trace the rest -- from compacted ray lists or
 *                       through the sorted pass, whichever two timed dispatches after each table build say is faster
 *                       (neb_gi_shadow_tail_mode); 3 = always the lists, 2 = always the sorted / tiled pass; results are bit-identical
 *                       in all of them.  No table is built for a sun disk wider than 3.4 degrees (sunTanHalfAngle > 0.03);
 *   "gi_sun_hold":      how many consecutive dispatches a NEW sun must be seen on before a table is built for it (a build costs five frames' time):
 *                       0 (default) = two -- or 32 when the table it replaces served fewer than 32 dispatches (a sun that moves in steps of a few
 *                       frames: a build per step would cost more than no table at all); N >= 2 pins the count.  A sun that changes every
 *                       dispatch is never built for; meanwhile every shadow ray is traced.  Results never depend on it;
 *   "gi_sun_hints":     4 (default), 2 or 0: how many of a triangle's occluder hints the shade pass tries (with the traverser's own
 *                       triangle test) before it leaves the shadow ray to the list pass; results are bit-identical in all three;
 *   "gi_max_bvh_depth": 1..21, the deepest BVH4 neb_gi_build_bvh accepts (default 21 = traversal stack / 3);
 *   "gi_deform_stage":  0 (default) / 1: where neb_gi_update_vertices' scatter kernel reads the staged vertices from, see there;
 *   "svgf_fuse":        0 (default) / 1 (opt-in), see neb_svgf_atrous;   "svgf_profile": 0 (default) / 1 / 2, see neb_svgf_level_times;
 *   "svgf_reproject":   0 (default) / 1 (opt-in): the temporal pass reprojects the history through the two frames' cameras, see
 *                       neb_svgf_set_camera.  NEB_ERR_STATE on a row-strip context.  1 allocates the (zeroed) history-length plane,
 *                       0 frees it: a context switched on and off again computes what a context that never had it on computes.
 *                       NEB_ERR_STATE for 0 while "svgf_motion" is 1 (turn that off first);
 *   "svgf_vertex_motion": 0 (default) / 1 (opt-in, needs "svgf_motion" = 1, else NEB_ERR_STATE; "svgf_motion" cannot be turned off while
 *                       it is 1): the temporal pass follows submeshes deformed by neb_gi_update_vertices / _device through
 *                       NEB_PLANE_PREV_POINT, see neb_svgf_snapshot_vertices.  1 allocates the plane and, with a scene, the previous
 *                       vertex pools; 0 frees them.  With the option 0 nothing changes;
 *   "svgf_demodulate":  0 (default) / 1 (opt-in): the albedo is divided out in front of the temporal pass and multiplied back at the last
 *                       a-trous level, so that the filter leaves textures sharp; see the block above neb_svgf_set_camera.  NEB_ERR_STATE on
 *                       a row-strip context.  1 allocates the (zeroed) NEB_PLANE_DEMOD, 0 frees it.  With 0 nothing changes;
 *   "svgf_motion":      0 (default) / 1 (opt-in, needs "svgf_reproject" = 1, else NEB_ERR_STATE): the reprojecting temporal pass follows
 *                       submeshes moved by neb_gi_update_transforms, see neb_svgf_snapshot_transforms.  1 allocates the (zeroed) submesh-id
 *                       plane and, with a scene set, two per-slot transform tables and the delta table; 0 frees them.  With 0 every
 *                       kernel, plane and call behaves as if the option did not exist. */
int neb_set_option(neb_ctx* ctx, const char* key, int value);

/* ---- resource sharing: the ~25 getters of SVGFDenoiser.h:24-70 collapse into one call.
 * Returns a borrowed device pointer to image row `row_begin` of the plane, valid until
 * resize/destroy; pitch in bytes; rows = row_end - row_begin. ---- */
int neb_get_plane(neb_ctx* ctx, int plane, int slot, void** dptr, size_t* pitch_bytes, uint32_t* rows);
/* Host <-> device convenience for harnesses (rows are image rows, must be resident).
 * Asynchronous on `stream`; the host buffer must stay valid until the stream is synchronised. */
int neb_upload_rows(neb_ctx* ctx, int plane, int slot, uint32_t row0, uint32_t nrows, const void* host, neb_stream stream);
int neb_download_rows(neb_ctx* ctx, int plane, int slot, uint32_t row0, uint32_t nrows, void* host, neb_stream stream);
int neb_stream_synchronize(neb_ctx* ctx, neb_stream stream);

/* ---- SVGF entry points (enqueue only) ---- */
/* SVGFDenoiser::ResetHistory (SVGFDenoiser.cpp:49-64): radiance[hist] <- radiance[cur]. */
int neb_svgf_reset_history(neb_ctx* ctx, neb_stream stream);
/* SVGFDenoiser::SubmitTemporalAccumulation (SVGFDenoiser.cpp:66-131) over all resident rows.
 * The G-buffer of the frame (normal[cur], depth[cur]) must be complete before this call, as the G-buffer pass precedes SVGF in the
 * reference: the a-trous levels of the frame read the decoded copy this pass (or, for rows it did not cover, a lazy decode) made. */
int neb_svgf_temporal(neb_ctx* ctx, neb_stream stream);
/* SVGFDenoiser::SubmitATrousComputeWavelet (SVGFDenoiser.cpp:133-203): all levels, all rows.
 * Only valid when the context holds the full image (row_begin == 0, row_end == height).
 *
 * By default both calls are stream-ordered at the call, as the reference records into its command list at the call
 * (SVGFDenoiser.cpp:116,185): after neb_svgf_temporal returns, the pass is enqueued on `stream`.
 *
 * Option "svgf_fuse" = 1 (OPT-IN; the binding of INTEGRATION.md sets it in SVGFDenoiser::Init): the two calls, made in this order
 * on the same stream with no other neb_* call between them -- what DeferredRenderer::SubmitCommandsSVGFDenoising does
 * (src/DeferredRenderer.cpp:610-611) -- run as ONE chain on a whole-frame context whose width and height are multiples of 8:
 * neb_svgf_temporal only NOTES the request (nothing is enqueued yet), and neb_svgf_atrous runs the temporal pass inside the
 * staging phase of level 0 (the accumulated radiance is never written to memory: quirk 5 makes the FILTERED image the next
 * frame's history), carries the luminance between the levels and writes radiance[cur], moments[cur] and variance exactly as the
 * separate passes do -- the same bits.  Any other neb_* call in between (a plane pointer, an upload or download, a row-range
 * form, neb_end_frame, neb_stream_synchronize ...) first submits the noted pass as its own kernel.
 * WHO CAN SEE THE DIFFERENCE, and so must not opt in (or must call neb_end_frame / neb_stream_synchronize first): a host that kept
 * plane pointers from an earlier neb_get_plane and, between the two calls, orders work on them WITHOUT going through the library
 * -- a raw hipStreamSynchronize / hipEventRecord on `stream`, or a kernel of its own reading moments, variance or the accumulated
 * radiance: until neb_svgf_atrous (or any other neb_* call) it finds them un-accumulated, and a launch error of the noted pass is
 * reported by that later call.  After the chain, radiance[hist] and the scratch plane hold intermediate levels (as radiance[hist]
 * does in the reference), here with the luminance in .w.  neb_svgf_denoise below is the same chain as one explicit call. */
int neb_svgf_atrous(neb_ctx* ctx, neb_stream stream);
/* DeferredRenderer::SubmitCommandsSVGFDenoising's pair of calls (src/DeferredRenderer.cpp:610-611: SubmitTemporalAccumulation, then
 * SubmitATrousComputeWavelet) as ONE entry point, whatever "svgf_fuse" says: the fused chain on a whole-frame context whose width
 * and height are multiples of 8, the two separate passes otherwise; the same bits as neb_svgf_temporal + neb_svgf_atrous, everything
 * enqueued on `stream` when the call returns.  Only valid when the context holds the full image. */
int neb_svgf_denoise(neb_ctx* ctx, neb_stream stream);
/* With option "svgf_profile" = 1, neb_svgf_atrous brackets each of its kernels with events on `stream`; this call waits for the
 * last chain submitted and returns the kernels' durations in microseconds (entry 0 = level 0, fused with the temporal pass when
 * the chain ran fused), *n_out = how many.  With "svgf_profile" = 2 only three events are recorded and two durations returned:
 * the first kernel, and all the others together (an event between two launches costs about 2 us of its own). */
/* With option "svgf_demodulate" = 1 one more entry follows the durations: the number of temporal calls that ran the seed kernel (below)
 * since "svgf_profile" was last set -- a count, not a time. */
int neb_svgf_level_times(neb_ctx* ctx, float* out_us, uint32_t capacity, uint32_t* n_out);
/* ---- Albedo demodulation (option "svgf_demodulate" = 1; no reference counterpart: the reference filters direct + indirect light with the
 * textures in it, SURVEY.md section 8a, and the a-trous levels cannot tell texture from noise).  Independent of "svgf_reproject",
 * "svgf_motion" and "svgf_vertex_motion", and composes with each.  With d_c = max(albedo_c, 1/32) per channel, albedo = the pixel's
 * R11G11B10_FLOAT word of NEB_PLANE_ALBEDO decoded (csrc/svgf_demod.h holds the floor and the order of operations):
 *   temporal pass:  the pixel's own radiance[cur].rgb is divided by d (the correctly rounded division) on load; the history -- same pixel
 *                   or the four reprojected taps -- is read from NEB_PLANE_DEMOD instead of radiance[hist]; moments and variance are
 *                   those of the demodulated luminance; the accumulated demodulated colour goes to radiance[cur] in place.
 *   a-trous levels: all but the last are the kernels they are without the option; they filter demodulated colour, so phiColor acts on
 *                   lighting, not on texture.  The level whose destination is the chain's result (neb_svgf_atrous_level_planes) writes
 *                   the filtered colour as it is into NEB_PLANE_DEMOD and the colour times the output pixel's d (one product) into its
 *                   destination: radiance[cur] ends up modulated, as a caller expects it.  Alpha is carried as without the option.
 * Which calls behave differently: as with "svgf_reproject", neb_svgf_temporal enqueues the pass at once even with "svgf_fuse" = 1 and
 * neb_svgf_atrous / neb_svgf_denoise run the separate kernels (bit for bit the same result with "svgf_fuse" 0 and 1).  NEB_ERR_INVALID_ARG
 * for a value other than 0 / 1, NEB_ERR_STATE on a row-strip context and on a context created with atrous_levels = 0 (there is no last
 * level to multiply the albedo back).  With the option 0 nothing changes, and a context switched on and off again computes what one that
 * never had it on computes.
 * VALIDITY of NEB_PLANE_DEMOD.  radiance[hist] holds the modulated image, and a reprojected tap comes from another pixel with another
 * albedo, so the history is KEPT demodulated, not re-derived.  The plane is taken as the history only if (1) the last level of the denoise
 * of the frame that is now hist wrote it -- in the previous neb_begin_frame bracket, all rows -- (2) with the option on, and (3) nothing has
 * written that radiance slot through the ABI since: neb_upload_rows, neb_svgf_reset_history, neb_resize.  Otherwise the temporal call first
 * runs a seed kernel over the resident plane, demod.rgb = radiance[hist].rgb / d(albedo) with the CURRENT albedo plane: the best stand-in
 * there is, exact for a static camera.  That covers the first frame, the option switched on mid-sequence, a frame the host did not denoise
 * and neb_svgf_reset_history.
 * TWO CAVEATS.  A write into radiance[hist] through a raw neb_get_plane pointer cannot be seen: such a host calls neb_svgf_reset_history,
 * or uploads a matching NEB_PLANE_DEMOD itself.  And the albedo plane must not change between a frame's temporal call and its last level:
 * the two read the same word of it to divide and to multiply back. ---- */
/* ---- Temporal reprojection (option "svgf_reproject" = 1; no reference counterpart: the reference's temporal pass reads the history at
 * the same pixel, SURVEY.md quirk 3, so a moving camera either skips SVGF or ghosts).  In this mode every temporal pass -- neb_svgf_temporal,
 * neb_svgf_denoise, neb_svgf_temporal_rows (whole frame only) -- runs the reprojecting kernel.  Per pixel p of the dispatch region
 * [0,Wd) x [0,Hd) (Wd = W/8*8, Hd = H/8*8, as the same-pixel pass):
 *   mapping:  P = the world point of p, rebuilt from depth[cur] and the camera of cur by inverting neb_gbuffer_raycast's projection
 *             (pixel centre (x+0.5)/W, the same axes, linear depth -z_view = m32 / (d + m22)); a pixel with no surface (D24 = 0xFFFFFF)
 *             takes no history.  P is projected with the camera of hist to a continuous pixel position q; its bilinear taps are
 *             floor(q - 0.5) + {0,1}^2.
 *   validity: a tap counts when it lies in [0,Wd) x [0,Hd), depth[hist] holds a surface there, the geometric normals (normal.xy) of p and
 *             of the tap have dot >= 0.9, and the tap's own world point P_t (from depth[hist] and the camera of hist) lies on p's plane:
 *             |dot(P_t - P, N_p)| <= 0.01 x the linear depth of P in the camera of hist (plane distance, not depth difference: grazing
 *             floors keep their history).
 *   blend:    radiance[hist] and moments[hist] are resampled as the bilinear-weighted, renormalised mean over the valid taps, and
 *             n = the largest history_length[hist] among them (n = 0 with no valid tap or a total weight <= 1e-4).  History weight
 *             a = n == 0 ? 0 : min(alpha, 1 - 1/(n+1)) -- a cumulative mean until it reaches alpha; radiance[cur] = lerp(current,
 *             history, a), moments likewise, variance = max(M2 - M1^2, varianceEps), history_length[cur] = min(n + 1, 255).
 *             depthSigma plays no part, nor does quirk 2 (the same-pixel pass keeps 100 % history where depth and normals disagree).
 * Which calls behave differently: neb_svgf_temporal enqueues the pass at once, even with "svgf_fuse" = 1, and neb_svgf_atrous /
 * neb_svgf_denoise run the separate levels (the "svgf_fuse" = 0 kernels: the same bits as with the option 0); neb_svgf_reset_history
 * also zeroes history_length[hist]; neb_svgf_temporal_rows on less than the whole frame and neb_strip_frame* return NEB_ERR_STATE.
 * A temporal pass with no camera recorded for cur returns NEB_ERR_STATE; with none for hist it is no error: the pass takes no history.
 *
 * neb_svgf_set_camera records the camera that slot `slot` (0, 1, NEB_SLOT_CURRENT or NEB_SLOT_HISTORY, resolved at the call) of the depth
 * and normal planes was rendered with.  neb_gbuffer_raycast records its camera for cur by itself; a host with its own raster G-buffer
 * (the reference: InspectCamera eye / target / up, 60 degrees, 0.1, 100 -- src/DeferredRenderer.cpp:133-148) calls this once per frame,
 * after neb_begin_frame, with slot NEB_SLOT_CURRENT.  neb_resize forgets both cameras.  NEB_ERR_INVALID_ARG for a bad slot or camera. */
struct neb_camera;
int neb_svgf_set_camera(neb_ctx* ctx, int slot, const struct neb_camera* cam);
/* ---- Moving submeshes under reprojection (option "svgf_motion" = 1 on top of "svgf_reproject" = 1).  Submeshes move as
 * whole units (neb_gi_update_transforms), so a pixel's motion is: which submesh it shows (NEB_PLANE_SUBMESH_ID) and one small matrix per
 * submesh and frame pair.  The library keeps, per G-buffer slot, a snapshot of the surfaceToWorld table the slot was rendered with; in front
 * of every temporal pass one small kernel turns the two snapshots into a delta entry per geometry (skipped when no update was enqueued
 * between them): flag 0 = the two matrices are equal bit for bit, 1 = moved, 2 = a matrix is singular or not finite; D = M_cur^-1 . M_hist
 * (row-vector convention: a world point of the current frame -> where that surface point was in the history frame), K = the inverse transpose
 * of D's 3x3 (carries a normal the same way).  The rule above then changes in two places, for every temporal pass while the option is 1:
 *   mapping:  g = submesh_id[cur][p].  Entry of g has flag 1: P_h = (P, 1) . D_g, N_h = normalise(N_p . K_g); flag 0, no entry (g >= the
 *             scene's geometry count, a slot without a snapshot, no scene) or no id: P_h = P, N_h = N_p exactly; flag 2: p takes no history.
 *             P_h is projected with the camera of hist as P was; the plane tolerance uses ITS linear depth.
 *   validity: the four tests above with P_h, N_h in place of P, N_p -- and one more: submesh_id[hist][tap] == g.  It applies to every
 *             pixel, moved or not: a wall uncovered by an object that moved away does not inherit the object's radiance, nor the object the wall's.
 * Blend, history length and variance are unchanged.
 *
 * neb_svgf_snapshot_transforms copies the scene's current transform table into slot `slot`'s snapshot (0, 1, NEB_SLOT_CURRENT or
 * NEB_SLOT_HISTORY), device to device, enqueue-only on `stream`, ordered behind an update enqueued on another stream and in front of a later one.
 * neb_gbuffer_raycast does it for cur by itself; a host with its own raster G-buffer calls it once per frame next to neb_svgf_set_camera
 * (and fills the submesh-id plane of cur).  neb_gi_set_scene and neb_resize forget both snapshots; a context without a scene keeps none (NEB_OK:
 * nothing moved).  NEB_ERR_INVALID_ARG for a bad slot, NEB_ERR_STATE while "svgf_motion" is 0. */
int neb_svgf_snapshot_transforms(neb_ctx* ctx, int slot, neb_stream stream);

/* ---- Deforming submeshes under reprojection (option "svgf_vertex_motion" = 1 on top of "svgf_motion" = 1).  A vertex
 * update (neb_gi_update_vertices, neb_gi_update_vertices_device) moves every surface point its own way, so the motion is one previous
 * point per pixel: NEB_PLANE_PREV_POINT.  While the option is 1 and a scene is set the library keeps a previous copy of the position and
 * normal pools -- the pools as they were when the most recent neb_gbuffer_raycast (or neb_svgf_snapshot_vertices) ran -- and a dirty word
 * per geometry, set by an accepted vertex update.  neb_gbuffer_raycast writes {P_h, oct16(N_h)} for every hit pixel of a dirty, valid
 * geometry when the history slot has a transform snapshot: the previous object-space vertices of the hit triangle interpolated at the
 * hit's barycentrics, under the history slot's transform -- so a deformation and a neb_gi_update_transforms between the same two frames
 * are followed at once -- and the sentinel everywhere else; behind the G-buffer kernel, on the same stream, it rolls the updated vertex
 * ranges into the previous pools and clears the dirty words.  The temporal pass takes P and the geometric normal from the plane where
 * .w is not the sentinel, and everything downstream of them is the pass of "svgf_motion".
 * "Previous" is the preceding raycast: a host that raycasts twice into one slot between two temporal passes compares against the first
 * of the two.  One raycast per frame is the contract.
 * neb_svgf_snapshot_vertices runs that roll without a raycast (enqueue-only), for a host that renders its own G-buffer and fills
 * NEB_PLANE_PREV_POINT itself: once per frame, after the frame's vertex updates.  NEB_ERR_STATE while "svgf_vertex_motion" is 0;
 * NEB_OK and nothing enqueued without a scene or with nothing updated.
 * The roll -- here and inside neb_gbuffer_raycast -- hands its vertex spans to the device in one of the four pinned argument slots of the
 * update calls and follows their rule: no device synchronisation and no allocation, but the host waits when the slot's last user, an
 * update or roll about a whole ring (kStageSlots = 4 calls) back, has not yet been read by the device. */
int neb_svgf_snapshot_vertices(neb_ctx* ctx, neb_stream stream);
/* Test / tooling aid: runs the delta kernel on the snapshots of (cur, hist) whether or not anything moved and downloads its table:
 * per geometry 32 floats = {flag as uint32 bits, 0, 0, 0 | D, 4 rows x 3 | K, 3 rows x 3 | zeros}; *n_out = entries written (the scene's
 * geometry count, which `capacity` must reach).  Synchronises `stream`.  host == NULL: the launch alone, enqueue-only (for timing it).
 * NEB_ERR_STATE without the option, a scene and both snapshots. */
int neb_svgf_debug_delta_table(neb_ctx* ctx, float* host, uint32_t capacity, uint32_t* n_out, neb_stream stream);
/* Row-range forms for multi-GPU row strips (no reference counterpart):
 * image rows [row0,row1) must be resident, and for the a-trous level so must every
 * (globally clamped) tap row.  `level` picks step = 1 << level and the source/destination
 * planes of that level's link in the ping-pong chain. */
int neb_svgf_temporal_rows(neb_ctx* ctx, uint32_t row0, uint32_t row1, neb_stream stream);
int neb_svgf_atrous_level_rows(neb_ctx* ctx, uint32_t level, uint32_t row0, uint32_t row1, neb_stream stream);
/* Which plane/slot level `level` reads and writes (for halo exchange between levels). */
int neb_svgf_atrous_level_planes(const neb_ctx* ctx, uint32_t level, int* src_plane, int* src_slot, int* dst_plane, int* dst_slot);

/* ======================= Multi-GPU row strips: halo exchange over RCCL (no reference counterpart) ================
 * One context per GPU holds image rows [row_begin, row_end) = the strip it owns plus halo rows (neb_create_info).  Every stage is
 * per-pixel except the a-trous wavelet, so the only data that crosses GPUs are halo rows of radiance (and variance), swapped with
 * the up / down neighbour by grouped ncclSend / ncclRecv straight out of / into the planes (rows are contiguous: no packing), on the
 * caller's stream.  RCCL is resolved at run time (dlopen of librccl): hosts link nothing extra, and without RCCL these calls return
 * NEB_ERR_STATE while everything single-GPU keeps working.  nebulae_amd/strips.py holds the partition arithmetic (which rows, when). */
typedef struct neb_halo_plane {
    int32_t plane; /* neb_plane */
    int32_t slot;  /* 0, 1, NEB_SLOT_CURRENT or NEB_SLOT_HISTORY */
} neb_halo_plane;
typedef struct neb_halo_swap {
    int32_t peer;                  /* rank in the communicator */
    uint32_t send_row0, send_row1; /* image rows sent to the peer (owned by this strip) */
    uint32_t recv_row0, recv_row1; /* image rows received from it (halo rows of this strip) */
} neb_halo_swap;
/* ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy through the library: one rank makes the 128-byte id, the host carries it to
 * the others however it likes (MPI, a socket, torch.distributed), every rank creates its communicator with it. */
int neb_strips_unique_id(void* id128);
int neb_strips_comm_create(int device, int n_ranks, int rank, const void* id128, void** out_comm);
int neb_strips_comm_destroy(void* comm);
/* ncclGroupStart / ncclGroupEnd.  A host with ONE process (or thread) per GPU never needs them.  A host that drives several GPUs
 * from one thread must bracket the neb_strips_comm_create calls of all its ranks in one group (ncclCommInitRank blocks until every
 * rank has joined: RCCL's rule for one thread with several devices; *out_comm is then valid once the group has ended), and likewise
 * the neb_strips_exchange calls of all its contexts for one exchange (the group each call opens nests inside the caller's). */
int neb_strips_group_begin(void);
int neb_strips_group_end(void);
/* For every listed plane and every swap: send rows [send_row0, send_row1), receive rows [recv_row0, recv_row1), all in ONE RCCL group,
 * enqueued on `stream` (ordered after the kernels that produced the rows, before the ones that read the halo).  Every rank of the
 * communicator must make the matching call.  comm = the ncclComm_t from neb_strips_comm_create (or the host's own). */
int neb_strips_exchange(neb_ctx* ctx, void* comm, const neb_halo_plane* planes, uint32_t n_planes, const neb_halo_swap* swaps, uint32_t n_swaps,
                        neb_stream stream);
const char* neb_strips_last_error(void); /* message of the last failed neb_strips_* call that had no context */

/* ONE call per strip frame (round 5): everything a strip context does between "radiance[cur] holds the direct term" and "radiance[cur]
 * holds this strip's rows of the denoised frame" -- the GI dispatch on its rows, the temporal pass, the halo exchange(s) and the a-trous
 * levels on the row ranges the exchange scheme prescribes -- enqueued by the library in the order and on the streams nebulae_amd/strips.py
 * used to spell out call by call (105 us of host time per 135-row strip frame from Python against 150 us of device time).  The partition
 * arithmetic is the library's (the same as strips.StripPartition: strips of H / n_strips rows; resident rows = strip +- halo, which the
 * context must have been created with: row_begin / row_end of neb_create_info).
 *   scheme NEB_STRIPS_ONCE:      one exchange per frame -- the h = sum_l 2 * 2^l boundary rows of the temporally accumulated radiance and of the
 *                                variance plane, beside the interior rows of level 0 (side stream); level l filters strip +- sum_{m>l} 2 * 2^m rows;
 *   scheme NEB_STRIPS_PER_LEVEL: an exchange of 2 * 2^l rows of the level's source plane in front of every level;
 *   scheme NEB_STRIPS_OVERLAP:   SURVEY 8e's: GI, temporal pass and levels 0 .. L-2 also on the band beyond the strip, one exchange in front
 *                                of the widest level, one of the final image's band rows (next frame's history) after it.
 * Transports: `comm` = an RCCL communicator (neb_strips_comm_create; one process or thread per GPU: every rank makes the matching call),
 * or `peers` = the neighbouring strips' contexts of a host that drives all strips from ONE thread (any devices: rows are pushed with
 * hipMemcpyPeerAsync; scheme ONCE only).  Such a host calls neb_strip_frame_begin for every strip, then neb_strip_frame_finish for every
 * strip, frame after frame; a host with a communicator calls neb_strip_frame (= begin + finish).
 * The contract of `peers` (strip r on stream[r]; the streams may all be one stream or N different ones; the calls only enqueue, no host wait):
 *   - strip r's inputs of the frame (its G-buffer, the direct term in radiance[cur], whatever else touches its planes) are enqueued on
 *     stream[r] before neb_strip_frame_begin(r), and a strip keeps its stream from frame to frame (or the host orders its streams itself);
 *   - ALL begin calls of a frame come before ANY finish call, from one thread, in any order inside a sweep, after each strip's neb_begin_frame.
 *     A finish without its begin, a finish before a neighbour's begin, a second begin and a begin while a neighbour is still in the frame
 *     before are refused with NEB_ERR_STATE before anything is enqueued;
 *   - the rows cross an edge when the LATER of its two strips begins, each way on the sending strip's stream: behind the sender's temporal
 *     pass (stream order), behind everything the receiver's stream holds up to its begin of this frame (the receiver's `inputs` event,
 *     recorded where the two streams differ) and behind the receiver's previous frame (its `frame_done` event: the halo rows were that
 *     frame's ping-pong buffer); the receiver's border rows of level 0 wait for the sender's `pushed` event, its interior rows for nothing.
 * Tested with N contexts on N streams of ONE device; two devices have not run yet.
 * flags: NEB_STRIP_RESET_HISTORY = neb_svgf_reset_history first (the frame policy's reset, src/DeferredRenderer.cpp:601-609).
 * constants == NULL: no GI dispatch (radiance[cur] is complete as it is). */
enum { NEB_STRIPS_ONCE = 0, NEB_STRIPS_PER_LEVEL = 1, NEB_STRIPS_OVERLAP = 2 };
enum { NEB_STRIP_RESET_HISTORY = 1 };
typedef struct neb_strip_plan {
    uint32_t n_strips, strip; /* this context holds strip `strip` of `n_strips` */
    uint32_t scheme;          /* NEB_STRIPS_* */
    uint32_t flags;           /* NEB_STRIP_* */
} neb_strip_plan;
typedef struct neb_strip_peers {
    neb_ctx* up;   /* the context of strip - 1 (NULL for the first strip) */
    neb_ctx* down; /* the context of strip + 1 (NULL for the last) */
} neb_strip_peers;
struct neb_gi_constants; /* (defined below) */
int neb_strip_frame(neb_ctx* ctx, const struct neb_gi_constants* constants, void* comm, const neb_strip_plan* plan, neb_stream stream);
int neb_strip_frame_begin(neb_ctx* ctx, const struct neb_gi_constants* constants, const neb_strip_plan* plan, const neb_strip_peers* peers, neb_stream stream);
int neb_strip_frame_finish(neb_ctx* ctx, void* comm, const neb_strip_plan* plan, const neb_strip_peers* peers, neb_stream stream);
/* The row ranges the plan implies for this strip (what strips.StripPartition computes; for hosts and tests):
 * out = {owned row0, row1, resident row0, row1, GI / temporal row0, row1, halo rows, band rows}; levels = the context's a-trous levels. */
int neb_strip_rows(const neb_ctx* ctx, const neb_strip_plan* plan, uint32_t out[8]);

/* ======================= GI: one-bounce indirect diffuse =========================================
 * Replaces DeferredRenderer::SubmitCommandsGIPathtrace (src/DeferredRenderer.cpp:396-591) driving
 * assets/shaders/pathtracer.hlsl with the NRC calls stubbed (rtxgi/Nrc.hlsli:579-621), and the DXR
 * driver BVH (src/nri/raytracing/RTAccelerationStructureBuilder.cpp:14-130) with a BVH built on the device (binned SAH, 4-wide). */

/* One submesh: StaticMeshGeometryData (src/nri/GIProcessedScene.h:17-31; shader mirror
 * pathtracer.hlsl:73-87).  The bindless (bufferIndex, offset) pairs become host pointers to the
 * first element; strides are in bytes.  Attribute order (src/nri/StaticMesh.h:14-21): position float3,
 * normal float3, texcoord float2, tangent float4.  neb_gi_set_scene copies everything. */
typedef struct neb_geometry_desc {
    float surfaceToWorld[16]; /* row-major, row-vector convention: world = (p,1) * M (SimpleMath Mat4) */
    int32_t materialIndex;    /* PathtracerInvalidBindlessIndex (-1) = none */
    uint32_t indexStride;     /* 2 or 4 */
    uint32_t numIndices;
    uint32_t numVertices;
    const void* indices;
    const void* attributes[4]; /* NULL = missing: hits on this submesh terminate the path (pathtracer.hlsl:313-318) */
    uint32_t attributeStrides[4];
    uint32_t _pad;
} neb_geometry_desc;

/* StaticMeshMaterialData (src/nri/GIProcessedScene.h:33-39; pathtracer.hlsl:99-105) */
typedef struct neb_material_desc {
    int32_t textureIndices[3]; /* albedo, normal, roughnessMetalness; -1 = use the factors */
    float albedo[4];
    float roughnessMetalness[2];
    uint32_t _pad;
} neb_material_desc;

/* R8G8B8A8_UNORM, one mip, no sRGB decode (src/core/GLTFSceneImporter.cpp:156); sampled linear/wrap at mip 0. */
typedef struct neb_texture_desc {
    const void* rgba8;
    uint32_t width, height;
} neb_texture_desc;

/* GlobalConstants (src/DeferredRenderer.h:219-238, pathtracer.hlsl:11-30) minus the NRC-only members. */
typedef struct neb_gi_constants {
    uint32_t frameIndex;
    uint32_t samplesPerPixel;
    uint32_t maxPathVertices; /* nrcMaxPathVertices, <= 8 (MaxPathtracingRecursionDepth, DeferredRenderer.h:118); 2 = one bounce, the
                                 north-star configuration; > 2 follows the shader's bounce loop with the NRC stubs (row f4) */
    float cameraWorldPos[3];
    float skyColor[3];
    float sunLightDirection[3];
    float sunLightRadiance[3];
    float sunTanHalfAngle;    /* tan(radians(diameter / 2)), DeferredRenderer.cpp:418 */
    float throughputThreshold;
} neb_gi_constants;

/* Per-pixel record of the last sample's bounce ray (the reference's debug UAVs, pathtracer.hlsl:41-42). */
typedef struct neb_gi_hit {
    float t;            /* < 0: miss */
    uint32_t geometry;  /* GeometryIndex() */
    uint32_t primitive; /* PrimitiveIndex() */
    uint32_t flags;     /* bit 0: sun shadow ray unoccluded; bits 8..31: traversal iterations of the bounce ray (diagnostics) */
} neb_gi_hit;

typedef struct neb_camera {
    float eye[3], target[3], up[3]; /* Mat4::CreateLookAt (RH), src/core/InspectCamera.h:44-48 */
    float vfov_deg, znear, zfar;    /* CreatePerspectiveFieldOfView(60 deg, aspect, 0.1, 100), DeferredRenderer.cpp:147-148 */
} neb_camera;

/* DeferredRenderer::InitPathtracerScene -> GIProcessedScene::InitScene (src/nri/GIProcessedScene.cpp:16-137):
 * uploads geometry/material tables and textures and bakes world-space triangles. */
int neb_gi_set_scene(neb_ctx* ctx, const neb_geometry_desc* geoms, uint32_t n_geoms, const neb_material_desc* mats,
                     uint32_t n_mats, const neb_texture_desc* texs, uint32_t n_texs);
/* DeferredRenderer::InitRTAccelerationStructures (src/DeferredRenderer.cpp:978-1030): builds the acceleration structure --
 * on the device, as the reference's driver does (RTAccelerationStructureBuilder.cpp:73-130): Morton sort, binned-SAH splits
 * level by level, collapse to 4-wide nodes; the host reads back one counter per pass, never a node.
 * One-time setup: enqueues on `stream` and SYNCHRONISES it before returning.  On failure the scene keeps its previous
 * state (unbuilt, or the previous valid tree); calling it again rebuilds. */
int neb_gi_build_bvh(neb_ctx* ctx, neb_stream stream);
/* RTAccelerationStructureBuilder::CreateTlas with a valid updateTlas (RTAccelerationStructureBuilder.cpp:100-130): new instance
 * transforms for n submeshes, the tree kept.  geometry_indices[k] names a geometry of neb_gi_set_scene, surfaceToWorld + 16 * k is
 * its new matrix (layout and row-vector convention of neb_geometry_desc::surfaceToWorld).  Every transform is applied to the
 * object-space positions of neb_gi_set_scene, never to the previous world positions: a chain of updates does not drift.
 * What is rewritten, on the device and in place: the world-space triangles of the named submeshes (same operation order as the
 * bake of neb_gi_set_scene, same bits), their rows of the geometry tables, the boxes of the 128-byte nodes above them (refitted
 * bottom-up, one launch per level) and the 64-byte nodes (quantised again).  Topology, node numbering, leaf order and depth do
 * not change; results are those of a tree built from the moved scene up to exact ties between coincident hits (only the exact
 * triangle tests decide a hit).  A leaf none of whose triangles moved keeps its box bit for bit; a leaf holding a clipped
 * reference of a moved triangle takes the whole triangle's bounds.  Tree quality degrades with the distance moved: DESIGN.md 3.4a.
 * A matrix equal to the one already set moves nothing; a call that moves nothing enqueues nothing.
 * Streams: enqueue only -- no device synchronisation, no allocation (the host waits only when it is kStageSlots = 4 updates ahead
 * of the device).  The rewrite runs on `stream` behind every dispatch enqueued before the call on whichever stream (an event is
 * recorded on each stream that has read the scene since the last update: those streams must still exist), and every later
 * neb_gi_trace* / neb_pbr_direct / neb_gbuffer_raycast on another stream waits for it: two frames in flight stay correct.
 * Sun table: treated as after a scene change.  Lit bits and occluder hints are not used from the moment of the call; the hold
 * policy ("gi_sun_hold") decides when a table is built again, against the new scene box (none beyond +-218 units).
 * A later neb_gi_build_bvh builds from the updated transforms.  Row-strip contexts accept the call; contexts given the same
 * updates hold the same tree.
 * Refusals, each leaving everything unchanged: NEB_ERR_STATE before a successful neb_gi_build_bvh; NEB_ERR_INVALID_ARG for a null
 * pointer with n > 0, an index >= n_geoms or an index named twice; NEB_ERR_OUT_OF_RANGE when a matrix entry is not finite or the
 * transform takes a corner of the submesh's object-space box (or a vertex) to a position that is not finite.  n == 0: NEB_OK. */
int neb_gi_update_transforms(neb_ctx* ctx, const uint32_t* geometry_indices, const float* surfaceToWorld /* n x 16, as neb_geometry_desc */,
                             uint32_t n, neb_stream stream);
/* Hiding and showing submeshes, the tree kept: the reference's InstanceMask -- RTCommon.h:90 sets 0xFF for every instance,
 * and InstanceMask = 0 in the PERFORM_UPDATE build it already runs (RTAccelerationStructureBuilder.cpp:100-130) is DXR's way to make an
 * instance absent.  geometry_indices[k] names a geometry of neb_gi_set_scene, visible[k] != 0 shows it, 0 hides it.  A hidden submesh
 * exists for no ray of any kind (camera, bounce, shadow): frames are those of a scene whose geometry k has an empty index list, up to
 * exact ties between coincident hits.  It stays a geometry: its slot, its pools, its matrix and its boxes remain, every update call
 * still applies to it (and keeps it hidden), neb_gi_download_vertices still reads it, and showing it bakes its CURRENT pose under its
 * CURRENT matrix.  What is rewritten, on the device and in place: one word per named geometry, the triangle slots of the geometries
 * whose flag changed (a hidden one gets triangles no ray can hit, the id words kept), the boxes of the 128-byte nodes above them (a
 * leaf bounds its visible triangles only; a leaf or node with none is an inverted box no ray enters) and the 64-byte nodes.  Topology,
 * node numbering, leaf order and depth do not change, so showing restores the tree bit for bit.  Entries that name a geometry already in
 * the state asked for are dropped; a call with nothing left enqueues nothing and keeps the sun table.
 * State: neb_gi_set_scene makes everything visible; neb_gi_build_bvh keeps the flags (it builds over ALL triangles, then empties the
 * hidden ones on the same stream before it returns, inside neb_gi_build_ms).  neb_gi_scene_box is the box of the visible geometries,
 * {0,0,0}-{0,0,0} when nothing is visible.
 * Streams: exactly as neb_gi_update_transforms -- enqueue only, no device synchronisation, no allocation, the arguments travel through
 * the same ring of 4 pinned slots, ordered behind every dispatch enqueued before the call on whichever stream and ahead of every later one.
 * Sun table: dropped whenever a flag changes, as after a scene change; "gi_sun_hold" decides when a table is built again, against the box
 * of the visible geometries; none is built while nothing is visible.  Row-strip contexts accept the call; every context of a group makes it.
 * Refusals, each leaving everything unchanged: NEB_ERR_STATE before a successful neb_gi_build_bvh; NEB_ERR_INVALID_ARG for a null
 * pointer with n > 0 or an index named twice; NEB_ERR_OUT_OF_RANGE for an index >= n_geoms.  n == 0: NEB_OK. */
int neb_gi_set_visibility(neb_ctx* ctx, const uint32_t* geometry_indices, const uint8_t* visible /* n, 0 = hidden */, uint32_t n, neb_stream stream);
/* The flags as the host holds them (1 = visible), one byte per geometry: out[0 .. min(capacity, n_geoms)); *n_out = n_geoms (either may
 * be asked for alone: capacity == 0 or n_out == NULL).  NEB_ERR_STATE without a scene.  Never waits. */
int neb_gi_get_visibility(const neb_ctx* ctx, uint8_t* out, uint32_t capacity, uint32_t* n_out);
/* What a submesh looks like, updated in place: the counterpart of the reference uploading its material table and its
 * textures again without touching the TLAS.  None of the four calls below touches triangles, nodes or shading records: the tree and the
 * SUN TABLE are kept.  They need a scene only (before or after neb_gi_build_bvh; a later build keeps what they set, neb_gi_set_scene
 * starts over), results are those of a fresh scene set from the edited tables, bit for bit.
 * Streams: exactly as neb_gi_update_transforms -- enqueue only, no device synchronisation, ordered behind every dispatch enqueued before
 * the call on whichever stream and ahead of every later one; no allocation after the first call of a kind (the host-sourced texel call
 * grows its staging to the largest call seen).  Row-strip contexts accept the calls; every context of a group makes them.
 * Refusals, each leaving everything unchanged: NEB_ERR_STATE without a scene; NEB_ERR_INVALID_ARG for a null pointer with n > 0, an
 * index named twice (materials and geometries; not textures), textureIndices that differ, a bad pitch, a source the device cannot
 * read; NEB_ERR_OUT_OF_RANGE for an index past its table, a factor that is not finite, a rectangle that is empty or leaves its texture.
 * n == 0: NEB_OK.
 *
 * neb_gi_update_materials: new albedo[0..2] and roughnessMetalness[0..1] for the named materials (albedo[3] is ignored, as in
 * neb_gi_set_scene).  textureIndices must equal what the material was set with (indices outside the texture table count as -1, as there):
 * which maps a material binds decides the layout of the tables, which is not rebuilt here.  A material given the factors it already has
 * is dropped; a call with nothing left enqueues nothing. */
int neb_gi_update_materials(neb_ctx* ctx, const uint32_t* material_indices, const neb_material_desc* mats, uint32_t n, neb_stream stream);
/* The named geometries name another material; a negative index means none (the shade pass sees the fields of no material exactly as
 * neb_gi_set_scene writes them).  Entries that change nothing are dropped. */
int neb_gi_set_geometry_materials(neb_ctx* ctx, const uint32_t* geometry_indices, const int32_t* material_indices, uint32_t n, neb_stream stream);
/* New texels: the rectangle [x, x + width) x [y, y + height) of texture `texture` is replaced by rows of RGBA8 at pitchBytes
 * (a multiple of 4, >= 4 * width).  The rectangle lies inside the texture and does not wrap; the texture's size does not change.
 * Several entries of one call may name the same texture: they apply in order.  The standalone footprint table of the texture and every
 * material bundle it sits in are patched (each texel lives in four entries of each).
 * neb_gi_update_textures: rgba8 is HOST memory, copied before the call returns; the rectangles of one call may total 64 MB at most
 * (NEB_ERR_OUT_OF_RANGE beyond: the staging is pinned memory, four slots of the largest call seen).
 * neb_gi_update_textures_device: rgba8 is memory this context's device reads at that address (as the sources of
 * neb_gi_update_vertices_device), 4-byte aligned, read in stream order: `stream` has to be ordered behind whatever writes it, and it
 * must stay untouched until the stream has passed the update.  No size limit. */
typedef struct neb_texture_update {
    uint32_t texture, x, y, width, height, pitchBytes;
    const void* rgba8;
} neb_texture_update;
int neb_gi_update_textures(neb_ctx* ctx, const neb_texture_update* updates, uint32_t n, neb_stream stream);
int neb_gi_update_textures_device(neb_ctx* ctx, const neb_texture_update* updates, uint32_t n, neb_stream stream);
/* Diagnostics: the texture tables as the device holds them -- the standalone footprint tables (16 bytes per texel position, in texture
 * order), then the material bundles (32 bytes per position, in material order) -- copied to host[0 .. *bytes) behind the work of `stream`;
 * waits for the copy.  host == NULL or capacity == 0: the size alone.  NEB_ERR_INVALID_ARG when capacity is below it. */
int neb_gi_debug_texture_tables(neb_ctx* ctx, void* host, size_t capacity, size_t* bytes, neb_stream stream);
/* Deforming submeshes: new object-space vertices for ranges of n submeshes, the tree kept.  NO reference counterpart:
 * the reference builds its BLASes without ALLOW_UPDATE (RTAccelerationStructureBuilder.cpp:79), so a swaying curtain, a skinned figure or
 * a morph target would mean new BLASes there; here it is the refit of neb_gi_update_transforms with another way in.
 * Entry k replaces vertices [firstVertex, firstVertex + numVertices) of geometry `geometry`: positions (float3, object space, required),
 * and optionally normals (float3) and tangents (float4); NULL keeps what the geometry has.  Pointers are HOST pointers with strides in
 * bytes, as in neb_geometry_desc; the call copies what it needs before it returns.  Indices, UVs, materials and vertex counts do not change.
 * What is rewritten, on the device and in place: the position / normal / tangent pools, the world-space triangles of the named submeshes
 * (ALL their triangles, baked under the current transform in the operation order of neb_gi_set_scene: same bits), the normal and tangent
 * words of their 128-byte shading records when an entry carried normals or tangents (every other word keeps its bits), the boxes of the
 * nodes above them and the 64-byte nodes.  Topology, node numbering, leaf order and depth do not change; results are those of a tree built
 * from the deformed scene up to exact ties between coincident hits; a leaf holding a clipped reference of a deformed triangle takes the
 * whole triangle's bounds.  Tree quality degrades with the amplitude: DESIGN.md 3.4b.
 * Streams, sun table, strips: exactly as neb_gi_update_transforms -- enqueue only, no device synchronisation, ordered behind every
 * dispatch enqueued before the call on whichever stream; the host waits only when it is 4 updates (of either kind) ahead of the device;
 * lit bits and hints are not used from the moment of the call and "gi_sun_hold" decides when a table is built against the new scene box.
 * No allocation once the pinned staging has reached the size of the largest update seen (it is allocated by the first call).
 * A later neb_gi_update_transforms applies its matrix to the deformed positions; a later neb_gi_build_bvh builds from them and packs the
 * records from the new normals and tangents.  "svgf_motion": a vertex update leaves the transform snapshots equal, so pixels of a deformed
 * submesh reproject as if static (the submesh-id test still applies) -- unless "svgf_vertex_motion" is 1 as well: the update then marks the
 * geometry, and neb_gbuffer_raycast writes where each of its pixels' points was one frame ago (neb_svgf_snapshot_vertices).
 * Refusals, each leaving everything unchanged: NEB_ERR_STATE before a successful neb_gi_build_bvh; NEB_ERR_INVALID_ARG for updates == NULL
 * with n > 0, NULL positions, a geometry >= n_geoms, a range beyond the geometry's numVertices, two overlapping ranges of one geometry in
 * the call, normals or tangents for a geometry set without all its attribute streams, a stride smaller than the element;
 * NEB_ERR_OUT_OF_RANGE when a position, or its world position under the current matrix, is not finite.  n == 0, or every numVertices == 0:
 * NEB_OK, nothing enqueued.
 * Option "gi_deform_stage" (A/B arm for profiling, results never depend on it): 0 (default) = the scatter kernel reads the pinned staging
 * directly, 1 = the staging is copied to a device buffer first (one hipMemcpyAsync); profiles/deform_times.json has both times. */
typedef struct neb_vertex_update {
    uint32_t geometry;                 /* index into neb_gi_set_scene's geometries */
    uint32_t firstVertex, numVertices; /* range inside that geometry's vertices */
    const void* positions;             /* float3, object space; required */
    uint32_t positionStride;
    const void* normals;               /* float3; NULL = keep */
    uint32_t normalStride;
    const void* tangents;              /* float4; NULL = keep */
    uint32_t tangentStride;
} neb_vertex_update;
int neb_gi_update_vertices(neb_ctx* ctx, const neb_vertex_update* updates, uint32_t n, neb_stream stream);
/* neb_gi_update_vertices for a host that skins, simulates or blends on the GPU: the same entries, the same rewrite, the
 * same ring, ordering and sun-table handling, but positions / normals / tangents are DEVICE pointers the context's GPU can read, strides
 * in bytes.  The call only enqueues and never reads a vertex on the host: the sources are read in stream order on `stream`, so the caller
 * orders `stream` behind whatever produced them and keeps them alive and unmodified until the stream has passed the update.
 * What the host did per vertex runs on the device: deform_check_kernel validates every position (finite, and finite under the geometry's
 * current matrix), the scatter reads the strided sources in place, and geom_box_kernel reduces the object- and world-space boxes of the
 * touched submeshes over their referenced vertices.  {refusal word, boxes} come back in one small copy at the end of the chain; the host
 * applies such records in call order when it next looks (any update call, neb_gi_update_status, neb_gi_scene_box, neb_gi_build_bvh) and,
 * waiting, at the dispatch whose hold policy would build a sun table -- the table is built against the exact box, never an older one.
 * Until then dispatches sort their work by the last known box (the keys only order work).
 * A position that fails the check refuses the WHOLE call on the device: nothing is written, NEB_OK has long been returned, and
 * neb_gi_update_status counts it (the sun table was dropped for nothing: harmless, frames do not depend on it).
 * The host copy of the touched submeshes' positions is stale from here on: later updates of them (host-sourced ranges, transforms --
 * checked by the corners of the object-space box alone) take their boxes from the device as well, and the next neb_gi_build_bvh reads
 * the positions back first.
 * Refusals at the call, each leaving everything unchanged: those of neb_gi_update_vertices except NEB_ERR_OUT_OF_RANGE, and
 * NEB_ERR_INVALID_ARG for a pointer or stride that is not a multiple of 4 and for a pointer hipPointerGetAttributes does not report as
 * memory of this context's device (or managed / mapped pinned memory), or whose range leaves its allocation. */
int neb_gi_update_vertices_device(neb_ctx* ctx, const neb_vertex_update* updates, uint32_t n, neb_stream stream);
/* Skinned submeshes: the producer neb_gi_update_vertices_device otherwise leaves to the host.  NO reference counterpart
 * (the reference has no compute skinning).  neb_gi_set_skin binds, per entry, four joint indices and four weights to EVERY vertex of a
 * geometry (all its numVertices; glTF JOINTS_0 as uint16 x 4 and WEIGHTS_0 as float x 4, HOST pointers, strides in bytes).  It is a set-up
 * call: it may allocate and wait.  It copies joints and weights to the device, repacked tight, and captures the BIND POSE: a
 * device-to-device copy, in stream order on `stream` and behind any rewrite enqueued on another stream, of the geometry's spans of the
 * live position, normal and tangent pools as they are at the call -- so binding after a neb_gi_update_vertices binds the deformed pose.
 * It also reserves the geometry's share (numJoints x 64 bytes, plus 64 bytes for its range) of the context's one device palette buffer:
 * neb_gi_skin_vertices never allocates.  Binding again replaces the previous skin and bind pose; joints == NULL removes the geometry's
 * skin and gives its memory back.  neb_gi_set_scene and neb_destroy forget and free every skin; neb_gi_build_bvh keeps them.
 * Weights are used as given (not renormalised).
 * Refusals, each leaving everything unchanged: NEB_ERR_STATE without a scene; NEB_ERR_INVALID_ARG for skins == NULL with n > 0, a geometry
 * >= n_geoms or named twice, numJoints of 0 or above 65535, NULL weights with joints, a stride below the element size (8 / 16), a joint
 * index >= numJoints (an influence of weight zero counts: the kernel reads its matrix); NEB_ERR_OUT_OF_RANGE for a weight that is not
 * finite.  n == 0: NEB_OK. */
typedef struct neb_skin_desc {
    uint32_t geometry;      /* index into neb_gi_set_scene's geometries */
    uint32_t numJoints;     /* size of the palette later handed to neb_gi_skin_vertices; 1 .. 65535 */
    const void* joints;     /* HOST, uint16 x 4 per vertex (glTF JOINTS_0); NULL = remove this geometry's skin */
    uint32_t jointStride;   /* bytes, >= 8 */
    const void* weights;    /* HOST, float x 4 per vertex (glTF WEIGHTS_0), used as given (not renormalised) */
    uint32_t weightStride;  /* bytes, >= 16 */
} neb_skin_desc;
int neb_gi_set_skin(neb_ctx* ctx, const neb_skin_desc* skins, uint32_t n, neb_stream stream);
/* The per-frame call: one palette of joint matrices per named geometry, the library does the rest.  Enqueue only; it never allocates after
 * the first call has sized the pinned ring.  The palettes travel through the four-slot pinned ring of the other update calls and reach the
 * device palette buffer in ONE hipMemcpyAsync: the kernels gather four matrices per vertex from device memory, never across the host link.
 * The chain on `stream`, in the ordering bracket of neb_gi_update_vertices_device: skin_check_kernel (one lane per vertex: the skinned
 * position and its world point under the geometry's current matrix must be finite, |x| <= 3.0e38, or the WHOLE call is refused on the
 * device: nothing is written, NEB_OK has long been returned, neb_gi_update_status counts it), skin_scatter_kernel (position, normal and
 * tangent from the BIND POSE, never from the live pools -- a chain of calls does not drift -- into the pools; a geometry set without its
 * attribute streams gets positions only), then the kernels of a vertex update unchanged: re-bake, record rewrite (always: normals always
 * change), boxes, refit levels, requantise, result record.
 * Arithmetic, one written-down order, every product and every sum rounded by itself (no fused multiply-add): with the four influences
 * i = 0..3 in the order stored, for rows 0-3 and columns 0-2 of the matrices,  S[q] = ((w0 J0[q] + w1 J1[q]) + w2 J2[q]) + w3 J3[q];
 * position = (p, 1) * S in the operation order of the bake; normal n'[c] = (n.x S[0][c] + n.y S[1][c]) + n.z S[2][c] (the upper 3x3,
 * NOT renormalised: the shading normalises each vertex normal at the hit); tangent .xyz as the normal, .w copied.
 * Host state, sun table, strips, svgf_vertex_motion: exactly a device-sourced update of the whole geometry -- the host copy of its positions
 * is stale from the enqueue on, its boxes come back in the result record, neb_gi_update_status counts the call once (accepted or refused),
 * the sun table is dropped and rebuilt by the hold policy against the harvested box, the denoiser follows the figure.
 * A later neb_gi_update_vertices / _device on a skinned geometry overwrites the pools but NOT the bind pose: the next skin call starts
 * from the bind pose again.  neb_gi_update_transforms composes (the skin lives in object space).
 * Refusals at the call, each leaving everything unchanged: NEB_ERR_STATE before a successful neb_gi_build_bvh or for a geometry without
 * a skin; NEB_ERR_INVALID_ARG for a null pointer with n > 0, a geometry >= n_geoms or named twice; NEB_ERR_OUT_OF_RANGE for a matrix
 * entry in columns 0-2 that is not finite.  n == 0: NEB_OK, nothing enqueued. */
typedef struct neb_skin_update {
    uint32_t geometry;
    const float* jointMatrices; /* HOST, numJoints x 16: layout and row-vector convention of surfaceToWorld, in the geometry's OBJECT
                                   space (glTF: inverseBind * jointGlobal * inverse(meshGlobal) in this convention); column 3 is ignored */
} neb_skin_update;
int neb_gi_skin_vertices(neb_ctx* ctx, const neb_skin_update* updates, uint32_t n, neb_stream stream);
/* Morph targets: the other half of glTF mesh animation, blended by the library, alone or under a skin.  NO reference
 * counterpart.  neb_gi_set_morph_targets binds, per entry, numTargets targets to EVERY vertex of a geometry: per target one float3 stream
 * of position deltas (glTF target POSITION; required), and optionally of normal and of tangent deltas (glTF: vec3, .w is not morphed) --
 * arrays of numTargets HOST pointers, strides in bytes.  It is a set-up call: it may allocate and wait.  It uploads the deltas repacked
 * tight and target-major, and captures the REST POSE: a device-to-device copy, in stream order on `stream` and behind any rewrite
 * enqueued on another stream, of the geometry's spans of the live position, normal and tangent pools as they are at the call -- so
 * binding after a neb_gi_update_vertices binds the deformed pose.  It also reserves the geometry's share of the context's one device
 * argument buffer (the palette buffer of the skin calls: 96 bytes, 8 per target, and its joints' share if it is skinned, whichever of the
 * two set-up calls comes first): neb_gi_morph_vertices never allocates.  Binding again replaces targets and rest pose; numTargets == 0
 * removes them and gives the memory back.  neb_gi_set_scene and neb_destroy free everything; neb_gi_build_bvh keeps the targets.
 * Refusals, each leaving everything unchanged (the previous targets stay in force): NEB_ERR_STATE without a scene; NEB_ERR_INVALID_ARG
 * for descs == NULL with n > 0, a geometry >= n_geoms or named twice, numTargets above 65535, NULL positionDeltas or a NULL entry of a
 * given array, a stride below 12, normal or tangent deltas for a geometry set without its attribute streams; NEB_ERR_OUT_OF_RANGE for a
 * delta that is not finite.  n == 0: NEB_OK. */
typedef struct neb_morph_desc {
    uint32_t geometry;                   /* index into neb_gi_set_scene's geometries */
    uint32_t numTargets;                 /* 1 .. 65535; 0 = remove this geometry's targets and rest pose */
    const void* const* positionDeltas;   /* HOST: numTargets pointers, each float3 per vertex (glTF target POSITION); required */
    uint32_t positionStride;             /* bytes, >= 12 */
    const void* const* normalDeltas;     /* HOST: numTargets pointers, float3 per vertex; NULL = the targets carry none */
    uint32_t normalStride;
    const void* const* tangentDeltas;    /* HOST: numTargets pointers, float3 per vertex (glTF: vec3, .w is not morphed); NULL = none */
    uint32_t tangentStride;
} neb_morph_desc;
int neb_gi_set_morph_targets(neb_ctx* ctx, const neb_morph_desc* descs, uint32_t n, neb_stream stream);
/* The per-frame call: one weight per target and named geometry and, for a skinned geometry, optionally its palette.  Enqueue only; it
 * never allocates once the pinned ring is sized.  The host compacts each geometry's weights to its ACTIVE LIST -- the pairs {target,
 * weight} with weight != 0 (+0 and -0 both drop out), in target order -- so the cost follows the active targets, not numTargets.  Ranges,
 * active lists and palettes travel through the pinned ring of the other update calls and reach device memory in ONE hipMemcpyAsync.
 * The chain on `stream`, in the ordering bracket of neb_gi_skin_vertices: morph_check_kernel (one lane per vertex: the final position,
 * skinned where a palette is given, and its world point under the geometry's current matrix must be finite, |x| <= 3.0e38, or the WHOLE
 * call is refused on the device: nothing is written, NEB_OK has long been returned, neb_gi_update_status counts it),
 * morph_scatter_kernel, then the kernels of a vertex update unchanged: re-bake, record rewrite (always), boxes, refit levels,
 * requantise, result record.
 * Arithmetic, one written-down order, every product and every sum rounded by itself (no fused multiply-add):
 *     m = rest position;  for each active {k, w} in target order:  m[c] = m[c] + w * dP_k[c]
 *     n, t.xyz likewise with dN_k, dT_k where the targets carry them (otherwise the rest value, its bits kept);  t.w copied
 * A target of weight zero contributes nothing, not even the sum: a -0.0 of the rest pose stays -0.0.  Nothing is renormalised (the
 * shading normalises each vertex normal at the hit).  jointMatrices == NULL: the pools get m, n, t.  With a palette, m, n, t take the
 * place of the bind pose in neb_gi_skin_vertices' order (glTF: morph, then skin): joints and weights come from the geometry's skin, the
 * skin's own bind pose is neither read nor changed, and nothing passes through an intermediate vertex buffer.  The blend always starts
 * from the REST pose, never from the live pools: a chain of calls does not drift, and all-zero weights restore the rest pose bit for bit.
 * neb_gi_skin_vertices on a geometry that also has targets behaves as without them (it reads its bind pose).
 * Host state, sun table, strips, svgf_vertex_motion: exactly a device-sourced update of the whole geometry, as neb_gi_skin_vertices.
 * Refusals at the call, each leaving everything unchanged: NEB_ERR_STATE before a successful neb_gi_build_bvh, for a geometry without
 * targets, for jointMatrices != NULL on a geometry without a skin; NEB_ERR_INVALID_ARG for a null pointer with n > 0, a geometry >=
 * n_geoms or named twice; NEB_ERR_OUT_OF_RANGE for a weight, or a matrix entry in columns 0-2, that is not finite.  n == 0: NEB_OK. */
typedef struct neb_morph_update {
    uint32_t geometry;
    const float* weights;        /* HOST, numTargets floats */
    const float* jointMatrices;  /* HOST, numJoints x 16 as in neb_skin_update, or NULL = do not skin */
} neb_morph_update;
int neb_gi_morph_vertices(neb_ctx* ctx, const neb_morph_update* updates, uint32_t n, neb_stream stream);
/* Copies the current contents of a geometry's spans of the device pools to host arrays: what a host whose own copy has gone stale (a
 * device-sourced update, a skin call) reads back.  Ordered behind rewrites enqueued on other streams, and it waits for the copies.  Any
 * geometry, skinned or not; a geometry set without its attribute streams reads zeros for normals and tangents.
 * Refusals: NEB_ERR_STATE without a scene; NEB_ERR_INVALID_ARG for a geometry >= n_geoms, a range beyond the geometry's numVertices, or
 * NULL positions with numVertices > 0.  numVertices == 0: NEB_OK. */
int neb_gi_download_vertices(neb_ctx* ctx, uint32_t geometry, uint32_t firstVertex, uint32_t numVertices, float* positions /* n x 3 */,
                             float* normals /* n x 3 or NULL */, float* tangents /* n x 4 or NULL */, neb_stream stream);
/* out = {device-sourced updates accepted, refused on the device} since neb_gi_set_scene.  Waits for every outstanding result record and
 * applies it first, so the counts include every neb_gi_update_vertices_device enqueued before the call. */
int neb_gi_update_status(neb_ctx* ctx, uint64_t out[2]);
/* The exact world-space box of the scene (the union of the submeshes' boxes over their referenced vertices), as the sun table's
 * certificate uses it.  Waits for outstanding result records like neb_gi_update_status; without device-reduced updates it returns
 * the box the host folded. */
int neb_gi_scene_box(neb_ctx* ctx, float lo[3], float hi[3]);
int neb_gi_scene_info(const neb_ctx* ctx, uint32_t* n_triangles, uint32_t* n_nodes);
/* Device bytes of the scene: {texture footprint tables + material bundles, triangles + shading records, BVH nodes: the
 * builder's 128-byte nodes + the 64-byte quantised nodes the rays walk}. */
int neb_gi_scene_bytes(const neb_ctx* ctx, uint64_t out[3]);
/* Inner-node levels of the BVH4 of the last successful build.  neb_gi_build_bvh returns NEB_ERR_OUT_OF_RANGE (and keeps the
 * previous tree, if any) when the depth exceeds what the traversal stack covers: 21, or "gi_max_bvh_depth". */
int neb_gi_bvh_depth(const neb_ctx* ctx, uint32_t* depth);
/* Passes (levels of the binary SAH tree) the last successful build took: diagnostics. */
int neb_gi_build_passes(const neb_ctx* ctx, uint32_t* passes);
/* Wall time in milliseconds of the last successful neb_gi_build_bvh (the build ends with a stream synchronisation). */
int neb_gi_build_ms(const neb_ctx* ctx, float* ms);
/* DeferredRenderer::SubmitCommandsGIPathtrace: radiance[cur].rgb += mean over spp of the path radiance
 * (stands in for NRC Resolve, DeferredRenderer.cpp:586).  Reads the ALBEDO / ROUGH_METAL / WORLDPOS planes and
 * normal[cur].  _rows: image rows [row0,row1) only (multi-GPU strips). */
int neb_gi_trace(neb_ctx* ctx, const neb_gi_constants* constants, neb_stream stream);
int neb_gi_trace_rows(neb_ctx* ctx, const neb_gi_constants* constants, uint32_t row0, uint32_t row1, neb_stream stream);
/* The same dispatch in two calls, for a host that keeps two frames in flight (the reference's swapchain keeps three, src/nri/Swapchain.h:15):
 * _begin enqueues ray generation + the closest-hit walk -- they read the G-buffer and write only GI records --, _finish the shading and shadow
 * passes of the dispatch begun longest ago, which add into the radiance[cur] of the frame current AT THE _finish CALL.  Two sets of GI records:
 * the _begin of frame f+1 may be enqueued (on another stream) while the _finish of frame f is still executing -- the short, latency-bound
 * shadow pass of frame f then runs beside the closest-hit walk of frame f+1 instead of alone on the chip.  `after_shade_event`: NULL, or a
 * hipEvent_t that _finish records between its two passes (what the next _begin's stream may wait for).  The caller orders the streams: a
 * _finish must not start before its own _begin has completed, a _begin not before the _finish that read its set (two dispatches earlier).
 * One sample and one bounce per pixel only (samplesPerPixel == 1, maxPathVertices <= 2); not together with "gi_defer_resolve". */
int neb_gi_trace_begin(neb_ctx* ctx, const neb_gi_constants* constants, uint32_t row0, uint32_t row1, neb_stream stream);
int neb_gi_trace_finish(neb_ctx* ctx, neb_stream stream, void* after_shade_event);
/* The reference's separate resolve step (nrc Resolve(commandList, GetRadianceOutput()), DeferredRenderer.cpp:586):
 * radiance[cur].rgb += the indirect term of the last neb_gi_trace that ran with "gi_defer_resolve" = 1.  Lets the GI
 * stages of frame f+1 overlap the SVGF passes of frame f on another stream (they share no plane until this call). */
int neb_gi_resolve(neb_ctx* ctx, neb_stream stream);
/* Rays traced (bounce + shadow) by all GI dispatches since the last reset.  Synchronises `stream`. */
int neb_gi_ray_count(neb_ctx* ctx, uint64_t* rays, int reset, neb_stream stream);
/* Diagnostics: counters as of the last neb_gi_ray_count call: {rays, bounce node visits, bounce triangle tests,
 * shadow node visits, shadow triangle tests}; the shadow entries are only collected while "gi_debug_hits" is 1. */
int neb_gi_traversal_stats(neb_ctx* ctx, uint64_t out[5]);
/* The sun-visibility table (no reference counterpart: the reference's shadow rays go to the driver's TraceRay,
 * assets/shaders/pathtracer.hlsl:567-569).  Every shadow ray of the path points at the sun disk; for each (triangle, side) the
 * library decides once per sun position -- exactly, from the scene's geometry -- whether ANY such ray leaving it can meet ANY
 * triangle; where none can, the hit's sun-visibility query is answered without a traversal, with the traversal's own answer.
 * out = {triangle sides proven lit on the +normal side, on the -normal side (last build), shadow rays answered by the table as of
 * the last neb_gi_ray_count call (they are part of its count: a ray = a visibility query), table builds so far}. */
int neb_gi_sun_table_stats(neb_ctx* ctx, uint64_t out[4], neb_stream stream);
/* Device time of the last build of the table (its two launches, between events on the stream it was enqueued on), in milliseconds.  Waits for that build.
 * NEB_ERR_STATE when no table has been built. */
int neb_gi_sun_table_build_ms(neb_ctx* ctx, float* ms);
/* Which pass takes the shadow rays the sun table leaves ("gi_sun_table" = 1): *mode = 0 the compacted lists, 1 the sorted pass, -1 not decided yet
 * for the current table (the first two dispatches after a build are the timed ones); us (may be NULL) = the two times of the last measurement
 * {lists, sorted pass}, shade + shadow launches between events, in microseconds.  Does not synchronise. */
int neb_gi_shadow_tail_mode(neb_ctx* ctx, int* mode, float us[2]);
/* Diagnostics (collected while "gi_debug_hits" is 1, as of the last neb_gi_ray_count call): where the closest-hit pass's waves spend
 * their loop iterations -- {waves, loop iterations, iterations that ran a node phase, lanes live in those, iterations that ran a leaf
 * phase, lanes live in those}; a wave executes every phase some lane needs, so lanes / (64 x iterations) is the lane utilisation. */
int neb_gi_wave_stats(neb_ctx* ctx, uint64_t out[6]);
/* Diagnostics (same collection): where in the breadth-first node array the closest-hit pass's node visits fall -- {visits of nodes with
 * an index below 64, below 256, below 1024, below 4096, node phases that ended with more than 12 entries on the ray's stack}; the
 * total is neb_gi_traversal_stats' bounce node visits.  (What a copy of the top of the tree in LDS would serve.) */
int neb_gi_node_index_stats(neb_ctx* ctx, uint64_t out[5]);
/* Tuning: the order in which the closest-hit pass takes its 8x8 tiles -- workgroup b walks tile order[b] (a permutation of 0 .. n - 1, n = the tiles of the
 * dispatches it applies to; any other dispatch keeps the default, XCD-aware order); NULL / 0 restores the default.  Results do not depend on it.  Synchronises. */
int neb_gi_debug_set_tile_order(neb_ctx* ctx, const uint32_t* order, uint32_t n);
/* Diagnostics of the sun-table build (collected when the environment variable NEB_SUN_WALK_STATS is set at build time of the table): for the lit pass
 * (out[0 .. 5]) and the hint pass (out[6 .. 11]) {node visits of all walks, the longest walk, candidate triangles tested, sum of the waves' run times and
 * the longest wave in 10-ns ticks, waves}.  Synchronises. */
int neb_gi_debug_sun_walk_stats(neb_ctx* ctx, uint64_t out[12]);
/* Diagnostics / tests: the sun table as the device holds it.  Copied to host[0 .. *bytes) behind the work of `stream` -- and behind the last
 * rewrite of the table on whichever stream, as a dispatch on `stream` would be -- in this order: the 128-byte shading records of the n_slots
 * triangle slots in leaf order (word 27 = the geometry | lit bits << 30, word 28 = the primitive, words 29-31 = four 23-bit occluder hints,
 * each a slot index or 0x7fffff, and in bit 95 the side they were chosen for), then the 48 bytes per slot the traverser tests
 * {v0.xyz, e1.x | e1.yz, e2.xy | e2.z, geometry, primitive, -}, then one neb_shade_records_info.  table_valid = 1: the lit bits and hints are
 * those of (sunLightDirection, sunTanHalfAngle) and the last dispatch used them; 0: no table, or one of another sun or of a scene that has
 * been updated since (the dispatches ignore it; the fields keep what they held).  lit_plus / lit_minus / hinted: the counters of the last
 * build (0 without a valid table).  Launches nothing; waits for the copy.  host == NULL or capacity == 0: the size alone.
 * NEB_ERR_STATE before a successful neb_gi_build_bvh, NEB_ERR_INVALID_ARG when capacity is below the size. */
typedef struct neb_shade_records_info {
    uint32_t n_slots, table_valid;
    float sunLightDirection[3], sunTanHalfAngle;
    uint32_t builds, reserved;
    uint64_t lit_plus, lit_minus, hinted;
} neb_shade_records_info;
int neb_gi_debug_shade_records(neb_ctx* ctx, void* host, size_t capacity, size_t* bytes, neb_stream stream);
/* Debug: when option "gi_debug_hits" is 1, every trace also records neb_gi_hit per resident pixel. */
int neb_gi_download_hits(neb_ctx* ctx, neb_gi_hit* host, neb_stream stream);
/* Diagnostics / tests: runs the library's ray-reordering sort (raysort.hip: stable LSD radix sort on key bits
 * [0, bits), bits <= 16) on n host (key, value) pairs and returns the values in sorted order.  Synchronises. */
int neb_debug_sort_pairs(neb_ctx* ctx, const uint32_t* keys, const uint32_t* values, uint32_t n, int bits, uint32_t* sorted_values);
/* "next" row f1: DeferredRenderer::SubmitCommandsPBRLighting (src/DeferredRenderer.cpp:326-394) driving
 * assets/shaders/deferred_pbr.hlsl:39-115: Cook-Torrance sun light x one any-hit shadow ray per pixel; OVERWRITES
 * radiance[cur] (alpha = 1).  Uses cameraWorldPos, sunLight*, sunTanHalfAngle and frameIndex of the constants. */
int neb_pbr_direct(neb_ctx* ctx, const neb_gi_constants* constants, neb_stream stream);
/* "next" row f3: DeferredRenderer::SubmitCommandsHDRTonemapping (src/DeferredRenderer.cpp:616-660),
 * assets/shaders/tonemapping.hlsl:3-53: ACES fit of radiance[cur] into the R8G8B8A8_UNORM LDR plane (alpha = luma). */
int neb_tonemap(neb_ctx* ctx, neb_stream stream);
/* "next" row f2: primary-visibility G-buffer producer with the encodings of
 * assets/shaders/deferred_gbuffers.hlsl:71-103 (writes ALBEDO, ROUGH_METAL, WORLDPOS, normal[cur], depth[cur]). */
int neb_gbuffer_raycast(neb_ctx* ctx, const neb_camera* camera, neb_stream stream);

/* Ray queries: the caller's own rays against the scene the context holds and keeps animated -- picking, line of sight,
 * probe and lightmap baking, AO, audio occlusion, sweeps -- without a second acceleration structure.  NO reference counterpart as a call
 * (it is what DXR inline queries, Embree and HIPRT offer as intersect / occluded).
 * `rays` and `out` are DEVICE pointers the context's GPU can read and write (as the sources of neb_gi_update_vertices_device: device
 * memory of this device with the whole range inside its allocation, managed memory, or mapped pinned memory): n rays in, and out =
 * neb_ray_hit[n], or uint32_t[n] with NEB_RAYS_ANY_HIT.  rays is 16-byte aligned, out 32-byte aligned for hit records (a record is
 * one 32-byte sector, written at its ray's index whatever order the rays are walked in) and 4-byte aligned for any-hit words.
 * The call only enqueues on `stream`: it runs behind every update call enqueued before it on any stream, and an update enqueued after
 * it waits for it.  The caller orders `stream` behind whatever wrote the rays and keeps both buffers alive until the stream has passed.
 * Per ray: the closest hit with tmin < t < tmax by the triangle test and the barycentrics of the frame's own walks -- u weighs the
 * triangle's second vertex, v its third (for a triangle the builder split, those of the whole triangle) -- t in units of the
 * direction's length (directions need not be normalised; tmax = +inf is allowed), geometry / primitive as neb_gi_hit names them.
 * Hidden submeshes are absent; every update call before it is reflected.  A miss: t = +inf, u = v = 0, geometry = primitive =
 * 0xFFFFFFFF.  reserved is written as 0.  A ray that cannot be walked reports a miss and costs nothing: a zero direction, an origin
 * or direction that is not finite (or so large that its squared length is not), tmin that is not >= 0 (NaN included), tmax that is
 * not > tmin.  With NEB_RAYS_ANY_HIT the walk ends at the first hit in the interval and the answer is one word, 1 = occluded.
 * NEB_RAYS_SORT walks the rays in the order of a 16-bit key (direction octant, then the origin's cell in the scene box), for rays
 * that arrive in no coherent order; the answers are the same bits.  The sort uses one block of device memory per context that only
 * grows: A SORTED CALL LARGER THAN ANY SORTED CALL BEFORE IT ALLOCATES AND WAITS (for the sorted call before it, on the host); NO
 * OTHER CALL DOES -- sorted calls on different streams run one after the other (the later one waits on the device), unsorted calls
 * use no scratch memory at all.  neb_gi_set_scene and neb_destroy free the block, neb_gi_build_bvh keeps it.
 * Leaves neb_gi_ray_count, the traversal statistics, the sun table and every plane untouched.  Strip contexts accept it: every
 * strip holds the whole scene.
 * Refusals, each enqueuing nothing: NEB_ERR_STATE without a built tree; NEB_ERR_INVALID_ARG for unknown flag bits, a null,
 * misaligned or unreadable pointer (or a range that leaves its allocation) and for out overlapping rays; NEB_ERR_OUT_OF_RANGE for
 * n above 2^28.  n == 0 succeeds and looks at neither pointer. */
typedef struct neb_ray {
    float origin[3], tmin, direction[3], tmax; /* 32 bytes, the layout of D3D12's RayDesc */
} neb_ray;
typedef struct neb_ray_hit {
    float t, u, v;
    uint32_t geometry, primitive, reserved[3]; /* 32 bytes */
} neb_ray_hit;
#define NEB_RAYS_ANY_HIT 1u /* first hit ends the walk; the output is one uint32_t per ray, 1 = occluded */
#define NEB_RAYS_SORT 2u    /* reorder the rays for coherence before the walk; the answers do not change */
int neb_gi_cast_rays(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags, void* out, neb_stream stream);

/* Shaded ray queries: the rays of neb_gi_cast_rays, and at each closest hit the surface the frame's shade pass would
 * reconstruct there (NEB_SHADE_SURFACE) or what the frame's path adds at a vertex reached along the ray with throughput 1
 * (NEB_SHADE_RADIANCE) -- the closest-hit shader's inputs of DXR, Embree and HIPRT, from the shading records, headers, footprint
 * tables and material bundles the device keeps, which no host copy follows across the update calls.  NO reference counterpart as a call.
 * `rays` and `out` are DEVICE pointers the context's GPU can read and write (as neb_gi_cast_rays takes them): n rays in, and out =
 * neb_ray_surface[n] or neb_ray_radiance[n].  rays is 16-byte aligned, out 32-byte aligned (a surface record is three 32-byte
 * sectors, a radiance record one, written at its ray's index whatever order the rays are walked in); the two do not overlap.
 * The call only enqueues on `stream`: it runs behind every update call enqueued before it on any stream, and an update enqueued after
 * it waits for it.  The caller orders `stream` behind whatever wrote the rays and keeps both buffers alive until the stream has passed.
 * Per ray: the closest hit with tmin < t < tmax; t, u, v, geometry and primitive are THE BITS neb_gi_cast_rays RETURNS FOR THE SAME
 * RAY.  Hidden submeshes are absent; every update call before it is reflected, materials and texels included.  The arithmetic policy
 * is the shade pass's ("gi_exact_shade").  flags (NEB_HIT_*): FOUND; ATTRIBUTES, the geometry has all its attribute streams, so
 * geometricNormal and texcoord are valid; MATERIAL, it has a material too, so shadingNormal, albedo, roughness and metalness are
 * valid; BACKFACE, dot(geometricNormal, direction) > 0 (defined only with ATTRIBUTES); NOT_WALKED; SUN_VISIBLE (radiance records).
 * A field whose flag is clear is written as 0 -- except material = -1, and shadingNormal = geometricNormal for a geometry with
 * attributes and no material.  A miss: t = +inf, geometry = primitive = 0xFFFFFFFF, material = -1, everything else 0.  A ray that
 * cannot be walked (the six kinds of neb_gi_cast_rays) never enters the tree: the miss record with NEB_HIT_NOT_WALKED set.
 * NEB_SHADE_SURFACE: position = origin + direction * t, each product and sum rounded by itself (the frame's hit point);
 * geometricNormal: world space, unit, as the vertex normals say, NOT flipped towards the ray; shadingNormal: the normal map applied;
 * texcoord: the interpolated uv the maps are sampled at; albedo, roughness, metalness: maps (bilinear, wrap) or factors, as the frame.
 * `constants` is ignored and may be NULL.
 * NEB_SHADE_RADIANCE: a miss gives skyColor (the constants' bits); a ray that was not walked gives 0, so that it can be told from a
 * miss; a hit without attributes or material gives 0 (the frame's path ends there too); a hit with NEB_HIT_MATERIAL casts ONE sun-disk
 * shadow ray, built as the frame builds it (pathtracer.hlsl:546-557): the two disk draws come from rng = JenkinsHash(i ^
 * JenkinsHash(frameIndex)), i = the ray's index in `rays` (vary frameIndex to average over the disk); origin = position -+ 1e-2
 * geometricNormal, on the side the ray leaves to; tmin 0.001, tmax 10000.  Unoccluded: rgb = EvaluateDirectBRDF(surface, V =
 * normalize(-direction), L = normalize(-sunLightDirection)) * sunLightRadiance -- the BRDF at the disk's CENTRE, no N.L factor, as
 * the frame -- and NEB_HIT_SUN_VISIBLE is set; occluded: 0.  Of the constants only frameIndex, skyColor, sunLightDirection,
 * sunLightRadiance and sunTanHalfAngle are read; they are taken as neb_gi_trace takes them, which refuses no value of them.  So a
 * degenerate sun acts as it acts on the frame: a zero (or non-finite) sunLightDirection gives a NaN sun frame, the shadow ray is one
 * the walk refuses -- hence "unoccluded" -- and every hit with a material reports NaN radiance with NEB_HIT_SUN_VISIBLE set.  Every
 * shadow ray is walked: the sun table is neither read nor touched.
 * NEB_RAYS_SORT: as neb_gi_cast_rays -- the same key, the same block of device memory and its rule (A SORTED CALL LARGER THAN ANY
 * SORTED CALL BEFORE IT, OF EITHER ENTRY POINT, ALLOCATES AND WAITS; NO OTHER CALL DOES); the answers are the same bits.
 * Leaves neb_gi_ray_count, the traversal statistics, the sun table with its hold counters and every plane untouched.  Strip contexts
 * accept it.
 * Refusals, each enqueuing nothing: NEB_ERR_STATE without a built tree; NEB_ERR_INVALID_ARG for an unknown `what`, unknown flag
 * bits or NEB_RAYS_ANY_HIT, NEB_SHADE_RADIANCE without constants, a null, misaligned or unreadable pointer (or a range that leaves its
 * allocation) and for out overlapping rays; NEB_ERR_OUT_OF_RANGE for n above 2^28.  n == 0 succeeds and looks at no pointer. */
typedef struct neb_ray_surface {
    float position[3], t;
    float geometricNormal[3];
    uint32_t geometry;
    float shadingNormal[3];
    uint32_t primitive;
    float albedo[3], roughness;
    float metalness, texcoord[2];
    int32_t material; /* -1: none */
    float u, v;       /* barycentrics, as neb_ray_hit */
    uint32_t flags, reserved; /* 96 bytes */
} neb_ray_surface;
typedef struct neb_ray_radiance {
    float r, g, b, t;
    uint32_t geometry, primitive, flags, reserved; /* 32 bytes */
} neb_ray_radiance;
#define NEB_SHADE_SURFACE 0u
#define NEB_SHADE_RADIANCE 1u
#define NEB_HIT_FOUND 1u
#define NEB_HIT_ATTRIBUTES 2u
#define NEB_HIT_MATERIAL 4u
#define NEB_HIT_BACKFACE 8u
#define NEB_HIT_NOT_WALKED 16u
#define NEB_HIT_SUN_VISIBLE 32u
int neb_gi_shade_rays(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t what, uint32_t flags /* 0 or NEB_RAYS_SORT */,
                      const neb_gi_constants* constants /* RADIANCE: required; SURFACE: ignored, may be NULL */, void* out, neb_stream stream);

/* Path queries: the rays of neb_gi_cast_rays, each followed as the frame follows a pixel's path -- the bounce loop of
 * pathtracer.hlsl:495-621 with up to maxPathVertices - 1 segments, its RNG stream, its by-value EvaluateIndirectBRDF draws and its
 * throughput rule -- for probes and lightmap bakers that need indirect light.  NO reference counterpart as a call.
 * `rays`, `out` and `vertices` are DEVICE pointers (as neb_gi_shade_rays takes them): n rays in, out = neb_ray_path[n], and vertices
 * = NULL or neb_path_vertex[n * (maxPathVertices - 1)].  rays is 16-byte aligned, out and vertices 32-byte aligned; no two of the
 * three overlap.  Stream ordering behind and ahead of the update calls, n == 0, the 2^28 limit, NEB_RAYS_SORT (the same key, the same
 * block of device memory and its rule: A SORTED CALL LARGER THAN ANY SORTED CALL BEFORE IT, OF ANY OF THE THREE ENTRY POINTS, ALLOCATES
 * AND WAITS; NO OTHER CALL DOES) and the arithmetic policy are those of neb_gi_shade_rays.  Only the first segment is walked in sorted
 * order; the answers are the same bits.
 * Per ray i: throughput = 1, rng = JenkinsHash(i ^ JenkinsHash(frameIndex)), i the index in `rays`; segment 1 is the caller's ray.  A ray
 * that cannot be walked (the six kinds of neb_gi_cast_rays) gives the miss record with NEB_HIT_NOT_WALKED, radiance 0, segments 0.
 * For k = 1 .. maxPathVertices - 1 the closest hit is walked.  A miss adds skyColor * throughput, sets NEB_PATH_ESCAPED and ends the
 * path.  A hit without attributes or material ends the path and adds nothing.  A hit with NEB_HIT_MATERIAL takes two disk draws from
 * rng and casts the sun-disk shadow ray of NEB_SHADE_RADIANCE (every shadow ray is walked); unoccluded, it adds EvaluateDirectBRDF *
 * sunLightRadiance * throughput and sets NEB_HIT_SUN_VISIBLE.  If k + 1 < maxPathVertices the next segment is sampled: e0, e1 from a
 * COPY of rng, direction = the cosine-weighted hemisphere sample about normalize(shadingNormal), origin = position + 1e-2
 * geometricNormal, tmin 0.001, tmax 10000; pdiff = 1 - specular probability(saturate(V.N), F0, albedo); throughput *= albedo * (1 -
 * metalness); then, if Rand(rng) < pdiff, throughput /= pdiff (NEB_PATH_DIVIDED).  A later segment the walk refuses (a direction that
 * is not finite) is a miss, as on the frame, and its vertex carries NEB_HIT_NOT_WALKED.
 * Vertex 1 ASSIGNS the sum and later vertices add to it: with maxPathVertices = 2 the record is NEB_SHADE_RADIANCE's bit for bit (r, g,
 * b, t, geometry, primitive, flags & 0x3F), the NaN of a degenerate sun included.  t, geometry, primitive and the NEB_HIT_* flags of
 * the record are those of the first segment.
 * With vertices != NULL, record i * (maxPathVertices - 1) + (k - 1) describes segment k of ray i: the segment's ray (k = 1: the
 * caller's bits), t / geometry / primitive / u / v as neb_gi_cast_rays answers that ray (t = +inf, ids 0xFFFFFFFF: it missed),
 * throughput and rng on ENTERING the vertex, what the vertex added to the sum (throughput included), its flags, and pdiff (0 where no
 * next segment is sampled).  A record past the path's end is 96 zero bytes; every record is written.  `out` is the same bits with and
 * without `vertices`.
 * Of the constants only frameIndex, maxPathVertices, skyColor, sunLightDirection, sunLightRadiance and sunTanHalfAngle are read
 * (samplesPerPixel is not: average calls with different frameIndex).  Leaves neb_gi_ray_count, the traversal statistics, the sun
 * table with its hold counters and every plane untouched.  Strip contexts accept it.
 * Refusals, each enqueuing nothing: NEB_ERR_STATE without a built tree; NEB_ERR_INVALID_ARG for unknown flag bits or
 * NEB_RAYS_ANY_HIT, null constants, maxPathVertices outside 2..8, a null (rays, out), misaligned or unreadable pointer (or a range that
 * leaves its allocation) and for overlapping ranges; NEB_ERR_OUT_OF_RANGE for n above 2^28.  n == 0 succeeds and looks at no pointer. */
typedef struct neb_ray_path { /* 32 bytes, the layout of neb_ray_radiance */
    float r, g, b, t;             /* path radiance; t of the FIRST hit (+inf: none) */
    uint32_t geometry, primitive; /* of the first hit */
    uint32_t flags;               /* NEB_HIT_* of vertex 1 (SUN_VISIBLE included) | NEB_PATH_ESCAPED */
    uint32_t segments;            /* closest-hit walks this path made: 0 (not walked) .. maxPathVertices - 1 */
} neb_ray_path;
typedef struct neb_path_vertex { /* 96 bytes, three 32-byte sectors */
    float origin[3], tmin; /* the segment's ray; k = 1: the caller's bits */
    float direction[3], t; /* t = +inf: this segment missed */
    float throughput[3];
    uint32_t rng; /* both on ENTERING the vertex, before its disk draws */
    float added[3];
    uint32_t flags; /* what this vertex added to the sum (throughput included); NEB_HIT_* of this vertex | NEB_PATH_DIVIDED */
    uint32_t geometry, primitive;
    float u, v;
    float tmax, pdiff; /* pdiff: 1 - specular probability used for the next bounce (0 where none is sampled) */
    uint32_t reserved[2];
} neb_path_vertex;
#define NEB_PATH_ESCAPED 64u  /* some segment missed: the sky (times throughput) is in the sum */
#define NEB_PATH_DIVIDED 128u /* the throughput leaving this vertex was divided by pdiff (Rand < pdiff) */
int neb_gi_trace_paths(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags /* 0 or NEB_RAYS_SORT */, const neb_gi_constants* constants,
                       void* out /* neb_ray_path[n] */, void* vertices /* NULL, or neb_path_vertex[n * (maxPathVertices - 1)] */, neb_stream stream);

/* Probe baking: S path samples per probe generated, followed and reduced on the device, one 128-byte record per probe
 * -- second-order spherical harmonics of the incoming radiance (NEB_BAKE_SH: an irradiance probe) or the irradiance of a surface point
 * (NEB_BAKE_IRRADIANCE: a lightmap texel).  NO reference counterpart as a call.
 * `probes` and `out` (neb_gi_probe_rays: `rays`) are DEVICE pointers, as neb_gi_trace_paths takes them: probes and rays 16-byte
 * aligned, out 32-byte aligned, the two ranges of a call not overlapping.  samples = S is a multiple of 64 in 64..4096 and n * S <= 2^28.
 * Sample s of probe p is ray index i = p * S + s.  neb_gi_probe_rays writes these n * S rays; neb_gi_bake_probes follows, for every i,
 * EXACTLY the path neb_gi_trace_paths follows for ray i of a call over those rays with the same constants (the same stream rng =
 * JenkinsHash(i ^ JenkinsHash(frameIndex)), the same arithmetic policy, maxPathVertices 2..8), the first segment over the probe's
 * (tmin, tmax), and reduces the path radiances L_i.  So neb_gi_bake_probes(...) == reduce(neb_gi_trace_paths(neb_gi_probe_rays(...)))
 * bit for bit, at 0 bytes of scratch memory against 64 bytes per sample.
 * DIRECTIONS, one IEEE operation per step under both policies (no contraction, the roundings as written), from a stream of their own:
 *   rng_d = JenkinsHash(~i ^ JenkinsHash(frameIndex + 0x9E3779B9));  r0 = Rand(rng_d);  r1 = Rand(rng_d);
 *   u0 = (float(s) + r0) / float(S)       (a sum, then an IEEE division: one stratum of [0, 1] per sample);   u1 = r1
 *   NEB_BAKE_SH (the whole sphere, uniform; `normal` is ignored):
 *     z = 1 - 2 * u0;  rho = sqrt(max(0, 1 - z * z))  (IEEE square root);  (sin, cos) = det_sincosf(6.2831853f * u1)
 *     d = (rho * cos, rho * sin, z) / sqrt((x * x + y * y) + z * z)        (IEEE square root, three IEEE divisions)
 *   NEB_BAKE_IRRADIANCE (cosine-distributed about the normal):
 *     N = normal / sqrt((nx * nx + ny * ny) + nz * nz);  d = the bounce sample of the frame about N with (u0, u1) in its exact form
 *     (brdf.hlsli:166-185 with IEEE sqrt and division and det_sincosf: cosine_hemisphere_aligned<false> of the library)
 * det_sincosf is the fixed sequence the frame uses for its bounce directions (the same text in the library and in oracle/trace_ref.cpp).
 * PROJECTION, per sample, every product and difference rounded by itself (no fused multiply-add anywhere):
 *   Y00 = 0.282095f;  Y1-1 = 0.488603f * y;  Y10 = 0.488603f * z;  Y11 = 0.488603f * x;  Y2-2 = 1.092548f * (x * y);
 *   Y2-1 = 1.092548f * (y * z);  Y20 = 0.315392f * ((3 * z) * z - 1);  Y21 = 1.092548f * (x * z);  Y22 = 0.546274f * (x * x - y * y)
 *   word[3 * lm + c] = L.c * Y_lm  (NEB_BAKE_SH, 27 words);  word[c] = L.c  (NEB_BAKE_IRRADIANCE, 3 words)
 * REDUCTION, round-major: for r = 0 .. S / 64 - 1 the 64 samples s = 64 r + l, l = 0 .. 63, are reduced per word by a butterfly over
 * the masks 32, 16, 8, 4, 2, 1 in this order -- v[l] = v[l] + v[l ^ m] for every l at once -- and the round's sum (v[0]) is added to
 * the running total, which starts at +0, in round order; the total is multiplied ONCE by float(4 pi / S) (SH) or float(3.14159265f /
 * S) (irradiance: E = pi * mean(L)), the factor computed in double and rounded once.  hits, backfaces and segments are exact integer sums.
 * A probe is NOT BAKED -- its record all zero but flags = NEB_PROBE_NOT_BAKED, samples = 0, no walk made; neb_gi_probe_rays writes S
 * rays of zeroes for it, which the queries report as NEB_HIT_NOT_WALKED -- if the position's squared length (x x + y y) + z z is not
 * finite in float (a component that is not finite, or above about 1.8e19: the origins neb_gi_cast_rays does not walk from), tmin is not
 * >= 0 or tmax is not > tmin (a NaN says no), or, under NEB_BAKE_IRRADIANCE, the normal's squared length is not positive and finite in
 * float (a normal below about 1e-19 in every component is a zero normal).  Both squared lengths are formed with every product and sum
 * rounded by itself.
 * A baked probe's record does not depend on which other probes are in the call, except through i.
 * Everything else is neb_gi_trace_paths': the call only enqueues on `stream`, behind every update call enqueued before it on any stream
 * (an update enqueued after it waits for it); it allocates nothing; hidden submeshes are absent; every shadow ray is walked; of the
 * constants only frameIndex, maxPathVertices, skyColor and the three sun fields are read; neb_gi_ray_count, the traversal statistics,
 * the sun table and every plane are left untouched.  To refine a bake, fold the records of calls with different frameIndex
 * into one buffer with neb_gi_accumulate_probes (below).
 * neb_gi_probe_rays needs a context but no scene.
 * Refusals, each enqueuing nothing: NEB_ERR_STATE without a built tree (bake); NEB_ERR_INVALID_ARG for an unknown `what`, samples
 * not a multiple of 64 in 64..4096, flags other than 0 (NEB_RAYS_SORT with a message of its own: a wave's rays share their origin),
 * null constants, maxPathVertices outside 2..8, a null, misaligned or unreadable pointer (or a range that leaves its allocation) and
 * for overlapping ranges; NEB_ERR_OUT_OF_RANGE for n * samples above 2^28.  n == 0 (with valid `what` and samples) succeeds and looks
 * at no pointer. */
typedef struct neb_probe { /* 32 bytes, the layout of neb_ray */
    float position[3], tmin; /* the first segment's interval: tmin > 0 keeps samples off the surface a texel lies on */
    float normal[3], tmax;   /* normal: NEB_BAKE_IRRADIANCE only, need not be normalised */
} neb_probe;
typedef struct neb_probe_record { /* 128 bytes, four 32-byte sectors */
    float sh[9][3];     /* NEB_BAKE_SH: coefficient (l,m) x rgb in the order above; NEB_BAKE_IRRADIANCE: sh[0] = E, the other 24 words 0 */
    uint32_t samples;   /* S, or 0 for a probe that was not baked */
    uint32_t hits;      /* samples whose first segment found a hit (NEB_HIT_FOUND) */
    uint32_t backfaces; /* ... of those, first hits flagged NEB_HIT_BACKFACE (a probe inside geometry shows here) */
    uint32_t segments;  /* sum of neb_ray_path.segments over the samples */
    uint32_t flags;     /* NEB_PROBE_NOT_BAKED */
} neb_probe_record;
#define NEB_BAKE_SH 0u
#define NEB_BAKE_IRRADIANCE 1u
#define NEB_PROBE_NOT_BAKED 1u
int neb_gi_probe_rays(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t frame_index,
                      neb_ray* rays /* n * samples */, neb_stream stream);
int neb_gi_bake_probes(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags /* 0 */,
                       const neb_gi_constants* constants, neb_probe_record* out /* n */, neb_stream stream);

/* Probe volumes: the probes of a regular grid, a running mean of bakes kept on the device, and the irradiance a grid of
 * NEB_BAKE_SH records gives at points -- bake -> accumulate -> gather with no record leaving the device.  NO reference counterpart.
 * All three calls need a context but NO SCENE and no frame, as neb_gi_probe_rays does.  Each only enqueues on `stream`, allocates nothing
 * and touches no plane, counter or sun table.  `probes`, `acc`, `add`, `records`, `points` and `out` are DEVICE pointers: probes and
 * points 16-byte aligned, records (acc, add) and gather records (out) 32-byte aligned, the ranges of a call not overlapping.
 * GRID.  Probe (x, y, z) has index x + nx * (y + ny * z) and sits at origin + float(x) * spacing per axis: ONE PRODUCT AND ONE SUM, EACH
 * ROUNDED BY ITSELF (no fused multiply-add).  neb_gi_probe_grid writes exactly these bits, the normal (0, 0, 1) and the interval (tmin,
 * tmax) it is given -- which it does not judge: neb_gi_bake_probes does --, and neb_gi_gather_probes forms a probe's position by the
 * same two operations, so that a point copied from a probe coincides with it.  Its output feeds neb_gi_bake_probes unchanged.
 * ACCUMULATION, per probe, with sa = acc.samples and sb = add.samples:
 *   sb == 0 (not baked, or an empty record): acc keeps all its bits (nothing is stored);
 *   sa == 0: acc becomes add, all 32 words -- a zeroed buffer is a valid start;
 *   sa + sb does not fit 32 bits: acc keeps its words and gains NEB_PROBE_SATURATED;
 *   otherwise  sh word = acc * wa + add * wb  (two products and a sum, each rounded by itself) with wa = float(double(sa) / double(sa +
 *   sb)), wb = float(double(sb) / double(sa + sb)), each rounded once; samples = sa + sb; hits, backfaces and segments are sums that
 *   stop at 2^32 - 1; flags = (acc.flags | add.flags) & ~NEB_PROBE_NOT_BAKED.
 * It serves NEB_BAKE_SH and NEB_BAKE_IRRADIANCE records alike.
 * GATHER, per point, DDGI's blend without its distance moments (neb_gi_gather_probes_visible, below, adds them), one IEEE operation per step:
 *   usable: (px px + py py) + pz pz finite and the normal's squared length, formed the same way, positive and finite -- the tests
 *     neb_gi_bake_probes makes under NEB_BAKE_IRRADIANCE; tmin and tmax are not read.  Otherwise the record is zero but for
 *     NEB_GATHER_NOT_GATHERED and no record of the grid is loaded.
 *   N = normal / sqrt(nn)  (IEEE square root, three IEEE divisions)
 *   per axis: t = (p - origin) / spacing (IEEE division);  tc = min(max(t, 0), float(dims - 1));  NEB_GATHER_CLAMPED if tc != t on any
 *     axis;  base = min(uint(floor(tc)), max(dims - 2, 0));  f = tc - float(base).  An axis with dims == 1 has base = 0, f = 0 and only
 *     its low corner: high corners along it are not loaded and their bit stays clear.  cell = bx + nx * (by + ny * bz).
 *   corner c = cx + 2 cy + 4 cz, in this order:
 *     w_tri = ((cx ? fx : 1 - fx) * (cy ? fy : 1 - fy)) * (cz ? fz : 1 - fz)
 *     q = origin + float(base + c) * spacing  (the grid's two operations);  v = q - p;  vv = (vx vx + vy vy) + vz vz
 *     d = ((vx Nx + vy Ny) + vz Nz) / sqrt(vv)  (IEEE), or 0 where vv == 0: the probe coincides with the point
 *     h = (d + 1) * 0.5;  w_n = h * h + 0.2
 *     valid = 0 if the record has samples == 0, or NEB_PROBE_NOT_BAKED, or float(backfaces) > backface_limit * float(samples)
 *     w = valid ? w_tri * w_n : 0.  A corner with w == 0 contributes nothing: its bit is clear and its sh words are not used, so a NaN
 *     among them cannot reach the result; the sh words of an invalid corner are not even loaded.
 *   W = the sum of w over c in order from +0;  W == 0: NEB_GATHER_NO_PROBE, E = 0, weight = 0, corners = 0.  Otherwise r = 1 / W (IEEE)
 *   and word k of the blend is the sum, over the contributing corners in order from +0, of (w * r) * sh[k] -- every product rounded.
 *   Y_lm(N) by the projection's formulas above; k_lm = A_l * Y_lm with A = (3.14159265f, 2.0943951f, 0.78539816f) = (pi, 2 pi / 3, pi / 4)
 *   E.c = max(0, sum over lm = 0 .. 8 in order from +0 of blend[3 lm + c] * k_lm)
 * A point's answer does not depend on which other points are in the call or where it stands in it: the kernel fetches a cell's records
 * once per wave where a wave's points share their cell and per lane where they do not, and both routes perform the operations above.
 * Refusals, each enqueuing nothing: NEB_ERR_INVALID_ARG for a null grid, a dims of 0, more than 2^24 probes, an origin that is not
 * finite, a spacing that is not finite and > 0, a backface_limit outside 0..1, a null, misaligned or unreadable pointer (or a range that
 * leaves its allocation) and for overlapping ranges.  n == 0 (with a valid grid, where there is one) succeeds and looks at no pointer. */
typedef struct neb_probe_grid { /* host struct, passed by pointer, 40 bytes */
    float origin[3], spacing[3]; /* probe (x, y, z) sits at origin + (x, y, z) * spacing; spacing finite and > 0 */
    uint32_t dims[3];            /* >= 1 each; dims[0] * dims[1] * dims[2] <= 2^24 */
    float backface_limit;        /* a probe whose backfaces > backface_limit * samples is ignored by the gather; 0..1, 0.25 is DDGI's */
} neb_probe_grid;
typedef struct neb_probe_gather { /* 32 bytes per point */
    float irradiance[3];          /* E at the point for its normal, >= 0 */
    float weight;                 /* sum of the corner weights */
    uint32_t corners;             /* bit (cx + 2 cy + 4 cz) set: that corner of the cell contributed */
    uint32_t cell;                /* linear index of the cell's base probe */
    uint32_t flags;               /* NEB_GATHER_* */
    uint32_t reserved;            /* 0 */
} neb_probe_gather;
#define NEB_PROBE_SATURATED 2u     /* flags of neb_probe_record: an accumulation was refused because samples would pass 2^32 - 1 */
#define NEB_GATHER_NO_PROBE 1u     /* every corner was ignored: E = 0, weight = 0 */
#define NEB_GATHER_CLAMPED 2u      /* the point lies outside the grid's box and was clamped to it */
#define NEB_GATHER_NOT_GATHERED 4u /* position or normal unusable: record zero but this flag */
int neb_gi_probe_grid(neb_ctx* ctx, const neb_probe_grid* grid, float tmin, float tmax, neb_probe* probes /* nx * ny * nz */, neb_stream stream);
int neb_gi_accumulate_probes(neb_ctx* ctx, neb_probe_record* acc, const neb_probe_record* add, uint32_t n, neb_stream stream);
int neb_gi_gather_probes(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records /* nx * ny * nz, NEB_BAKE_SH */,
                         const neb_probe* points /* n: position and normal read, tmin / tmax ignored */, uint32_t n,
                         neb_probe_gather* out /* n */, neb_stream stream);

/* Probe-lit frames: the frame's G-buffer as the gather's points, and the gather's irradiance added to radiance[cur] as
 * the frame's indirect diffuse term -- the stand-in for neb_gi_trace in a frame.  NO reference counterpart.
 * Rows are those of neb_gi_trace_rows: image rows [row0, row1) inside the context's rows (a row-strip context holds [row_begin, row_end));
 * neb_gi_probe_indirect is the _rows call over all the context's rows.  Neither call needs a scene: the planes may come from
 * neb_gbuffer_raycast or from neb_upload_rows.  Both only enqueue on `stream` and allocate nothing; neither touches a counter, a GI
 * record, a hit record or the sun table.  neb_gbuffer_points writes no plane; neb_gi_probe_indirect writes radiance[cur] and no other.
 * POINT of pixel i (x + W * (y - row_begin) in the planes), the point neb_gi_trace's ray generation shades, one IEEE operation per step:
 *   sky = (depth[cur][i] >> 24) == 0 (the stencil byte):  position = (0, 0, 0), normal = (0, 0, 0)
 *   else position = the first three fp16 words of NEB_PLANE_WORLDPOS, each converted to float32 (exact);
 *        (ex, ey) = the .zw fp16 words of NEB_PLANE_NORMAL[cur] converted likewise;  v = (ex, ey, (1 - |ex|) - |ey|);
 *        if v.z < 0:  v.xy = ((1 - |v.y|) * (v.x > 0 ? 1 : -1), (1 - |v.x|) * (v.y > 0 ? 1 : -1))  (both from the old v.xy)
 *        normal = v / sqrt((v.x v.x + v.y v.y) + v.z v.z)  (IEEE square root, three IEEE divisions)
 *   tmin = 0.01f, tmax = +infinity.
 * neb_gbuffer_points writes these 32 bytes per pixel, pixel (x, y) at index (y - row0) * W + x: a valid `points` of neb_gi_gather_probes
 * -- whose usability rule answers NEB_GATHER_NOT_GATHERED for a sky pixel, or a pixel whose fp16 words hold an infinity or a NaN, with
 * no special case -- and a valid `probes` of neb_gi_bake_probes(..., NEB_BAKE_IRRADIANCE).
 * INDIRECT TERM, per pixel of the rows.  g = what neb_gi_gather_probes(grid, records, the pixel's POINT) returns: the same operations, the
 * same bits.  g.flags with NEB_GATHER_NOT_GATHERED or NEB_GATHER_NO_PROBE: the pixel's 16 bytes of radiance are not stored to.
 * Otherwise, with albedo = the R11G11B10 word of NEB_PLANE_ALBEDO decoded, metalness = the high fp16 word of NEB_PLANE_ROUGH_METAL:
 *   k.c = albedo.c * (1 - metalness)                                     (the throughput ray generation starts from)
 *   with NEB_INDIRECT_FRAME_WEIGHT:  k.c = k.c * e, where e is the expectation of the factor ray generation's draw applies to that
 *     throughput -- it divides by pd where Rand < pd, so e = pd (1 / pd) + (1 - pd) = 2 - pd for pd > 0, else 1 --;
 *     pd = 1 - Brdf_GetSpecularProbability(saturate(dot(normalize(V), normal)), F0, albedo), V = constants->cameraWorldPos - position,
 *     F0 = lerp(0.04, albedo, metalness), every step as neb_gi_trace's ray generation performs it (float32, no fused multiply-add)
 *   add.c = (k.c * g.irradiance.c) * (1 / 3.14159265f);   radiance.c = radiance.c + add.c       -- each product and the sum rounded
 *   by itself; alpha keeps its bits.
 * Without the flag the term is Lambert's albedo (1 - metalness) E / pi; with it a probe-lit frame converges toward what the traced frame
 * converges toward.  Of the constants only cameraWorldPos is read, and only with the flag (else `constants` may be NULL).
 * A pixel's answer does not depend on the rows of the call or on its neighbours: a wave takes an 8 x 8 pixel tile and the gather's
 * wave-uniform or per-lane route, which perform the same operations.
 * Refusals, each enqueuing nothing: NEB_ERR_INVALID_ARG for the grid as neb_gi_gather_probes refuses it, unknown flag bits,
 * NEB_INDIRECT_FRAME_WEIGHT with null constants, a null, misaligned (records: 32 bytes, points: 16) or unreadable pointer (or a range
 * that leaves its allocation), `records` overlapping the radiance plane, `points` overlapping a plane the call reads;
 * NEB_ERR_OUT_OF_RANGE for rows outside the context's rows or row1 <= row0. */
#define NEB_INDIRECT_FRAME_WEIGHT 1u
int neb_gbuffer_points(neb_ctx* ctx, uint32_t row0, uint32_t row1, neb_probe* points /* (row1 - row0) * W */, neb_stream stream);
int neb_gi_probe_indirect(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records /* nx * ny * nz, NEB_BAKE_SH */,
                          const neb_gi_constants* constants /* read only with NEB_INDIRECT_FRAME_WEIGHT, else may be NULL */, uint32_t flags,
                          neb_stream stream);
int neb_gi_probe_indirect_rows(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_gi_constants* constants,
                               uint32_t flags, uint32_t row0, uint32_t row1, neb_stream stream);

/* Probe visibility: DDGI's distance maps -- per probe an 8 x 8 octahedral map of filtered distance moments, in a buffer
 * PARALLEL to the records (neb_probe_record and every call above are unchanged) -- and the gather with a Chebyshev visibility factor per
 * corner, so that a probe behind a wall thinner than a cell does not light the point.  NO reference counterpart.
 * `out`, `acc`, `add` and `visibility` are DEVICE pointers, 32-byte aligned; the other pointers as in the calls above.  One IEEE
 * operation per step, every product and sum rounded by itself, IEEE sqrt and division, no fused multiply-add.
 * TEXEL k = i + 8 j has the direction n_k:  (ex, ey) = (((i + 0.5) / 8) * 2 - 1, ((j + 0.5) / 8) * 2 - 1)  (exact);  v = (ex, ey, (1 - |ex|) -
 *   |ey|);  if v.z < 0:  v.xy = ((1 - |ey|) * sgn(ex), (1 - |ex|) * sgn(ey)) with sgn(0) = +1;  n_k = v / sqrt((vx vx + vy vy) + vz vz).
 * BAKE.  The directions are those of neb_gi_probe_rays(probes, n, samples, NEB_BAKE_SH, frame_index): the same ray index i = p * S + s,
 * stratification and stream, so that neb_gi_probe_rays yields the very rays followed.  Each is walked ONCE by the closest-hit walk of
 * neb_gi_cast_rays over the probe's (tmin, tmax): no shading, no sun, no bounce, the same bits under both arithmetic policies.
 *   per sample s:  dist = hit ? min(t, max_distance) : max_distance
 *   per texel k, over s = 0 .. S - 1 IN SAMPLE ORDER, the three sums starting from +0:
 *     c = (nx dx + ny dy) + nz dz;  c < 0.25: the sample counts nothing for this texel (keeps the filter free of denormals);  otherwise
 *     g = c^32 by five squarings;  A += g;  M1 += g * dist;  M2 += g * (dist * dist)
 *   A > 0:  weight = A, moments = (M1 / A, M2 / A);  otherwise weight = 0, moments = (max_distance, max_distance * max_distance).
 * A probe neb_gi_bake_probes would not bake under NEB_BAKE_SH (position not finite in its squared length, tmin not >= 0 or tmax not >
 * tmin) gets every texel (max_distance, max_distance^2, weight 0) at no walk.  A probe's record does not depend on the other probes of
 * the call except through i.  samples, ordering behind updates, hidden submeshes, allocation (none) and what is left untouched (every
 * plane, neb_gi_ray_count, the statistics, the sun table) are neb_gi_bake_probes'; so are the refusals, with NEB_ERR_INVALID_ARG also
 * for a max_distance that is not finite and > 0.
 * ACCUMULATION, per texel, wa = acc.weight, wb = add.weight:  wb == 0: acc keeps its bits;  wa == 0: acc becomes add;  otherwise W = wa +
 *   wb, moment = acc * (wa / W) + add * (wb / W) for both moments, weight = W.  A zeroed buffer is a valid start.  Needs no scene.
 * VISIBLE GATHER: neb_gi_gather_probes (above) with one more factor per corner, computed only for corners whose record is valid:
 *     pb = p + normal_bias * N;  u = pb - q  (q by the grid's two operations);  rr = (ux ux + uy uy) + uz uz;  r = sqrt(rr)
 *     rr == 0: vis = 1.  Otherwise  s = (|ux| + |uy|) + |uz|;  ox = ux / s;  oy = uy / s;
 *     if uz < 0:  (ox, oy) = ((1 - |oy|) * sgn(ox), (1 - |ox|) * sgn(oy))  (both from the old values, sgn(0) = +1)
 *     tx = ox * 4 + 3.5;  ix = floor(tx)  (-1 .. 7);  fx = tx - float(ix);  likewise ty, iy, fy
 *     taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1), each wrapped, x first and then y: an index outside 0..7 on an axis is
 *     clamped on that axis and the index b on the other axis becomes 7 - b  (so (-1, -1) lands on (7, 7): the octahedral map's own edges)
 *     m = ((1 - fx) t00 + fx t10) (1 - fy) + ((1 - fx) t01 + fx t11) fy   for both moments, every product and sum rounded
 *     var = max(m2 - m1 * m1, 2^-10 * m2);  cheb = r > m1 ? var / (var + (r - m1) * (r - m1)) : 1;  vis = max(0.05, (cheb * cheb) * cheb)
 *     w = valid ? (w_tri * w_n) * vis : 0
 *   W: a corner with vis == 1 (w unchanged) is added to W by the very operation of neb_gi_gather_probes, whose library build adds the
 *   product w_tri * w_n to W in one fused step (W may differ from the sum of the rounded w by an ulp; w itself is rounded); a corner
 *   with vis < 1 is added as the rounded w.  Only so do the two calls agree to the bit where nothing is hidden.
 *   Everything else is the plain gather's: the sum order, r = 1 / W, the convolution, the flags, the validity rule.  With maps whose
 *   every texel is (D, D^2), D above every r that occurs, the call returns the bits of neb_gi_gather_probes; a point's answer does not
 *   depend on the other points of the call.
 * neb_gi_probe_indirect_visible(_rows) is neb_gi_probe_indirect(_rows) over the visible gather: the same pixels' points, the same
 * weighting, the same flags.
 * Refusals of the two gathers: those of neb_gi_gather_probes / neb_gi_probe_indirect, and NEB_ERR_INVALID_ARG for a normal_bias that is
 * not finite and >= 0 and for a visibility pointer that is null, misaligned (32 bytes), unreadable, leaves its allocation (one record per
 * probe of the grid) or overlaps what the call writes. */
typedef struct neb_probe_visibility { /* 768 bytes per probe, 32-byte aligned */
    float moments[64][2]; /* texel k = i + 8 j: filtered mean distance, mean squared distance */
    float weight[64];     /* the texel's sum of filter weights: what a running mean needs; 0 = the texel was never filled */
} neb_probe_visibility;
int neb_gi_bake_visibility(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t frame_index, float max_distance,
                           neb_probe_visibility* out /* n */, neb_stream stream);
int neb_gi_accumulate_visibility(neb_ctx* ctx, neb_probe_visibility* acc, const neb_probe_visibility* add, uint32_t n, neb_stream stream);
int neb_gi_gather_probes_visible(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records,
                                 const neb_probe_visibility* visibility /* nx * ny * nz */, float normal_bias, const neb_probe* points, uint32_t n,
                                 neb_probe_gather* out /* n */, neb_stream stream);
int neb_gi_probe_indirect_visible(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records, const neb_probe_visibility* visibility,
                                  float normal_bias, const neb_gi_constants* constants, uint32_t flags, neb_stream stream);
int neb_gi_probe_indirect_visible_rows(neb_ctx* ctx, const neb_probe_grid* grid, const neb_probe_record* records,
                                       const neb_probe_visibility* visibility, float normal_bias, const neb_gi_constants* constants, uint32_t flags,
                                       uint32_t row0, uint32_t row1, neb_stream stream);

/* Probe feedback: a path query or a bake whose paths END IN A PROBE GRID.  At the path's last possible vertex, where no
 * further segment is sampled, the grid's irradiance stands for everything the path did not walk, so that bake -> accumulate -> bake(tail
 * = the accumulated grid) adds one bounce per update to every probe with a bake as short as two path vertices.  NO reference counterpart.
 * tail == NULL: the call IS neb_gi_trace_paths / neb_gi_bake_probes -- the same kernels, the same bits, the same refusals.
 * THE TAIL.  Everything up to the path's last possible vertex is neb_gi_trace_paths' contract bit for bit: the walk, the RNG stream, the
 * flags, the throughput, every earlier `added`.  With last = maxPathVertices - 1, the tail applies at segment k == last and only where
 * that vertex carries NEB_HIT_MATERIAL, after the vertex's direct term, one IEEE operation per step:
 *   1. sd = (SN.x * d.x + SN.y * d.y) + SN.z * d.z, every product and sum rounded; Ng = SN if sd <= 0, else -SN.  SN is the shading normal
 *      as NEB_SHADE_SURFACE reports it for this hit, d the segment's own direction.  The POINT is {position = origin + direction * t as
 *      the path forms it (NEB_SHADE_SURFACE's position), normal = Ng}.
 *   2. g = what neb_gi_gather_probes(grid, records, POINT) returns; with `visibility`, what neb_gi_gather_probes_visible(grid, records,
 *      visibility, normal_bias, POINT) returns: the same operations, the same bits, whichever route the wave's points take.
 *   3. g.flags with NEB_GATHER_NOT_GATHERED or NEB_GATHER_NO_PROBE: nothing is added, no flag is set, the record is the plain call's.
 *   4. k.c = throughput.c * (albedo.c * (1 - metalness)), the throughput on ENTERING the vertex: the two products the next bounce
 *      would have formed.
 *   5. with NEB_TAIL_FRAME_WEIGHT: pd = the pdiff the next bounce would have used (the same expression, under the context's arithmetic
 *      policy, as at an inner vertex); it is written to the vertex record's pdiff, which otherwise stays 0;
 *      k.c = k.c * (pd > 0 ? 2 - pd : 1), each operation rounded (NEB_INDIRECT_FRAME_WEIGHT's reasoning).
 *   6. tail.c = (k.c * g.irradiance.c) * (1 / 3.14159265f), every product rounded by itself under both policies.
 *   7. the vertex's added.c = added.c + tail.c, one rounded sum; the vertex record and the path record gain NEB_PATH_TAIL.
 *   8. out.rgb stays the float32 running sum of the `added` words, vertex 1 assigning.
 * A vertex that ends a path earlier -- a miss, a hit without material, a segment the walk refuses -- gets no tail.  A terminal hit
 * flagged NEB_HIT_BACKFACE does: Ng faces the ray, thin two-sided geometry is legitimate.
 * neb_gi_bake_probes_tail(...) == reduce(neb_gi_trace_paths_tail(neb_gi_probe_rays(...))) bit for bit: projection, reduction order,
 * scale and counters are neb_gi_bake_probes'; hits, backfaces and segments are unchanged by a tail.
 * `records` and `visibility` are DEVICE pointers read in stream order, like any device pointer of these calls: bake -> neb_gi_accumulate_
 * probes -> bake on one stream is well-defined.  Everything else is the plain calls': they allocate nothing (a sorted call as
 * neb_gi_trace_paths), run behind updates, leave planes, counters and the sun table untouched; hidden submeshes are absent; strip
 * contexts accept them.
 * Refusals, each enqueuing nothing: all of the plain call's, checked first and under the plain call's name; then, with a non-NULL
 * tail, NEB_ERR_INVALID_ARG for the grid as neb_gi_gather_probes refuses it, unknown tail->flags, `records` null, misaligned (32 bytes),
 * unreadable or leaving its allocation (one record per probe of the grid), `visibility` likewise when non-NULL, with `visibility` a
 * normal_bias that is not finite and >= 0, and `records` or `visibility` overlapping out, vertices, rays or probes (the in-place hazard
 * of a feedback loop: bake into a second buffer, then accumulate).  n == 0 succeeds and looks at nothing of the tail. */
#define NEB_TAIL_FRAME_WEIGHT 1u
#define NEB_PATH_TAIL 256u /* vertex flags: this vertex's `added` contains a grid tail; path flags: the path took one */
typedef struct neb_probe_tail { /* host struct, passed by pointer */
    neb_probe_grid grid;
    const neb_probe_record* records;        /* nx * ny * nz NEB_BAKE_SH records, device, 32-byte aligned */
    const neb_probe_visibility* visibility; /* NULL: the plain gather; else the visible gather */
    float normal_bias;                      /* read only with visibility */
    uint32_t flags;                         /* 0 or NEB_TAIL_FRAME_WEIGHT */
} neb_probe_tail;
int neb_gi_trace_paths_tail(neb_ctx* ctx, const neb_ray* rays, uint32_t n, uint32_t flags /* 0 or NEB_RAYS_SORT */, const neb_gi_constants* constants,
                            const neb_probe_tail* tail /* NULL: neb_gi_trace_paths */, void* out /* neb_ray_path[n] */,
                            void* vertices /* NULL, or neb_path_vertex[n * (maxPathVertices - 1)] */, neb_stream stream);
int neb_gi_bake_probes_tail(neb_ctx* ctx, const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags /* 0 */,
                            const neb_gi_constants* constants, const neb_probe_tail* tail /* NULL: neb_gi_bake_probes */, neb_probe_record* out /* n */,
                            neb_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* NEBULAE_HIP_H */
