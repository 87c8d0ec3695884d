// nebulae_hip.hpp -- C++ host-side mirror of the reference classes over the C ABI (nebulae_hip.h).
//
// Same member names and argument meaning as Neb::SVGFDenoiser (src/SVGFDenoiser.h:11-93) and the GI
// methods of Neb::DeferredRenderer (src/DeferredRenderer.h:50-81); ID3D12GraphicsCommandList4* becomes a
// HIP stream.  Error behaviour follows the reference: failures throw (the reference throws HrException
// through ThrowIfFailed/ThrowIfFalse, src/nri/stdafx.h:44-98); here the exception carries neb_last_error().
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "nebulae_hip.h"

namespace Neb
{

    struct NebException : std::runtime_error
    {
        int Status;
        NebException(int status, const std::string& what) : std::runtime_error(what), Status(status) {}
    };

    inline void ThrowIfFailed(neb_ctx* ctx, int status, const char* what)
    {
        if (status != NEB_OK)
            throw NebException(status, std::string(what) + ": " + neb_last_error(ctx));
    }

    class SVGFDenoiser
    {
    public:
        SVGFDenoiser() = default;
        SVGFDenoiser(const SVGFDenoiser&) = delete;
        SVGFDenoiser& operator=(const SVGFDenoiser&) = delete;
        ~SVGFDenoiser() { neb_destroy(m_ctx); }

        bool IsInitialized() const { return m_ctx != nullptr; }

        // SVGFDenoiser::Init (src/SVGFDenoiser.cpp:14-26).  rowBegin/rowEnd select a multi-GPU row strip.
        bool Init(uint32_t width, uint32_t height, uint32_t numAtrousPasses = NumAtrousPasses, int device = 0,
                  uint32_t rowBegin = 0, uint32_t rowEnd = 0)
        {
            if (IsInitialized())
                throw NebException(NEB_ERR_STATE, "SVGFDenoiser::Init: already initialised");
            neb_create_info info{device, width, height, rowBegin, rowEnd, numAtrousPasses};
            ThrowIfFailed(nullptr, neb_create(&info, &m_ctx), "neb_create");
            // This class orders all its work on the planes through neb_* calls, so it opts into the held-back temporal pass:
            // SubmitTemporalAccumulation + SubmitATrousComputeWavelet back to back run as one fused chain (nebulae_hip.h).
            // A host that also touches cached plane pointers with raw HIP calls between the two: SetOption("svgf_fuse", 0).
            ThrowIfFailed(m_ctx, neb_set_option(m_ctx, "svgf_fuse", 1), "neb_set_option");
            return true;
        }
        // The reference returns false on success (src/SVGFDenoiser.cpp:36) and its caller throws on it; fixed here.
        bool Resize(uint32_t width, uint32_t height)
        {
            ThrowIfFailed(m_ctx, neb_resize(m_ctx, width, height), "neb_resize");
            return true;
        }

        void BeginFrame(uint32_t frameIndex) { ThrowIfFailed(m_ctx, neb_begin_frame(m_ctx, frameIndex), "neb_begin_frame"); }
        void EndFrame() { ThrowIfFailed(m_ctx, neb_end_frame(m_ctx), "neb_end_frame"); }
        uint32_t GetCurrentResourceIndex() const { return (uint32_t)neb_current_index(m_ctx); }
        uint32_t GetHistoryResourceIndex() const { return (uint32_t)neb_history_index(m_ctx); }

        // One accessor instead of the ~25 descriptor getters: device pointer of a plane (borrowed).
        void* GetPlane(neb_plane plane, int slot = NEB_SLOT_CURRENT, size_t* pitchBytes = nullptr, uint32_t* rows = nullptr)
        {
            void* p = nullptr;
            ThrowIfFailed(m_ctx, neb_get_plane(m_ctx, plane, slot, &p, pitchBytes, rows), "neb_get_plane");
            return p;
        }
        void* GetCurrentRadianceTexture() { return GetPlane(NEB_PLANE_RADIANCE, NEB_SLOT_CURRENT); }
        void* GetHistoryRadianceTexture() { return GetPlane(NEB_PLANE_RADIANCE, NEB_SLOT_HISTORY); }

        void ResetHistory(neb_stream commandList) { ThrowIfFailed(m_ctx, neb_svgf_reset_history(m_ctx, commandList), "neb_svgf_reset_history"); }
        void SubmitTemporalAccumulation(neb_stream commandList) { ThrowIfFailed(m_ctx, neb_svgf_temporal(m_ctx, commandList), "neb_svgf_temporal"); }
        // (called right after SubmitTemporalAccumulation on the same command list -- DeferredRenderer::SubmitCommandsSVGFDenoising's
        // order -- the two run as one fused chain: see neb_svgf_atrous in nebulae_hip.h)
        void SubmitATrousComputeWavelet(neb_stream commandList) { ThrowIfFailed(m_ctx, neb_svgf_atrous(m_ctx, commandList), "neb_svgf_atrous"); }
        // Both passes as one explicit call (DeferredRenderer::SubmitCommandsSVGFDenoising, src/DeferredRenderer.cpp:610-611)
        void SubmitDenoising(neb_stream commandList) { ThrowIfFailed(m_ctx, neb_svgf_denoise(m_ctx, commandList), "neb_svgf_denoise"); }
        // Implementation knobs without a reference counterpart ("svgf_fuse", "svgf_profile", "atrous_variant", the "gi_*" options)
        void SetOption(const char* key, int value) { ThrowIfFailed(m_ctx, neb_set_option(m_ctx, key, value), "neb_set_option"); }
        // Option "svgf_reproject" = 1: the camera the slot's depth / normal planes were rendered with (NEB_SLOT_CURRENT once per frame,
        // after BeginFrame, for a host with its own raster G-buffer -- see neb_svgf_set_camera and INTEGRATION.md)
        void SetCamera(int slot, const neb_camera& camera)
        {
            ThrowIfFailed(m_ctx, neb_svgf_set_camera(m_ctx, slot, &camera), "neb_svgf_set_camera");
        }
        // Option "svgf_motion" = 1: the snapshot of the scene's transforms the slot's G-buffer was rendered with (NEB_SLOT_CURRENT once per
        // frame next to SetCamera, for a host with its own raster G-buffer -- see neb_svgf_snapshot_transforms), and the submesh-id plane
        // such a host fills (NEB_PLANE_SUBMESH_ID lies behind the neb_plane enum, hence an accessor of its own)
        void SnapshotTransforms(int slot, neb_stream commandList)
        {
            ThrowIfFailed(m_ctx, neb_svgf_snapshot_transforms(m_ctx, slot, commandList), "neb_svgf_snapshot_transforms");
        }
        void* GetSubmeshIdPlane(int slot = NEB_SLOT_CURRENT, size_t* pitchBytes = nullptr, uint32_t* rows = nullptr)
        {
            void* p = nullptr;
            ThrowIfFailed(m_ctx, neb_get_plane(m_ctx, NEB_PLANE_SUBMESH_ID, slot, &p, pitchBytes, rows), "neb_get_plane");
            return p;
        }
        // Option "svgf_vertex_motion" = 1 (SetOption, after "svgf_motion"): once per frame after the frame's vertex updates, for a host with
        // its own raster G-buffer -- the updated vertices become the "previous" ones of the next frame (neb_svgf_snapshot_vertices) -- and
        // the one-slot previous-point plane such a host fills (NEB_PLANE_PREV_POINT, behind the neb_plane enum as well)
        void SnapshotVertices(neb_stream commandList) { ThrowIfFailed(m_ctx, neb_svgf_snapshot_vertices(m_ctx, commandList), "neb_svgf_snapshot_vertices"); }
        void* GetPrevPointPlane(size_t* pitchBytes = nullptr, uint32_t* rows = nullptr)
        {
            void* p = nullptr;
            ThrowIfFailed(m_ctx, neb_get_plane(m_ctx, NEB_PLANE_PREV_POINT, 0, &p, pitchBytes, rows), "neb_get_plane");
            return p;
        }
        // Option "svgf_demodulate": the albedo is divided out in front of the temporal pass and multiplied back at the last a-trous level (see
        // the block above neb_svgf_set_camera), and the one-slot plane that holds the demodulated history while it is on (NEB_PLANE_DEMOD,
        // behind the neb_plane enum as well)
        void SetAlbedoDemodulation(bool on) { ThrowIfFailed(m_ctx, neb_set_option(m_ctx, "svgf_demodulate", on ? 1 : 0), "neb_set_option"); }
        void* GetDemodPlane(size_t* pitchBytes = nullptr, uint32_t* rows = nullptr)
        {
            void* p = nullptr;
            ThrowIfFailed(m_ctx, neb_get_plane(m_ctx, NEB_PLANE_DEMOD, 0, &p, pitchBytes, rows), "neb_get_plane");
            return p;
        }
        // Durations (us) of the kernels of the last SubmitATrousComputeWavelet chain, after SetOption("svgf_profile", 1); returns how many
        uint32_t LevelTimes(float* outMicroseconds, uint32_t capacity)
        {
            uint32_t n = 0;
            ThrowIfFailed(m_ctx, neb_svgf_level_times(m_ctx, outMicroseconds, capacity, &n), "neb_svgf_level_times");
            return n;
        }

        // GetTemporalConstants()/GetATrousConstants(): one POD with the six tunables (SVGFDenoiser.h:76-92).
        neb_svgf_params GetConstants() const
        {
            neb_svgf_params p;
            ThrowIfFailed(m_ctx, neb_svgf_get_params(m_ctx, &p), "neb_svgf_get_params");
            return p;
        }
        void SetConstants(const neb_svgf_params& p) { ThrowIfFailed(m_ctx, neb_svgf_set_params(m_ctx, &p), "neb_svgf_set_params"); }

        neb_ctx* Context() const { return m_ctx; }
        static constexpr uint32_t NumAtrousPasses = 4; // src/SVGFDenoiser.h:199

    private:
        neb_ctx* m_ctx = nullptr;
    };

    // The GI methods of DeferredRenderer that sit on the hot path (src/DeferredRenderer.h:79, .cpp:396-591,978-1030).
    class GIPathtracer
    {
    public:
        explicit GIPathtracer(SVGFDenoiser& svgf) : m_svgf(svgf) {}
        void InitPathtracerScene(const neb_geometry_desc* geoms, uint32_t nGeoms, const neb_material_desc* mats, uint32_t nMats,
                                 const neb_texture_desc* texs, uint32_t nTexs)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_set_scene(m_svgf.Context(), geoms, nGeoms, mats, nMats, texs, nTexs), "neb_gi_set_scene");
        }
        void InitRTAccelerationStructures(neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_build_bvh(m_svgf.Context(), commandList), "neb_gi_build_bvh");
        }
        // RTAccelerationStructureBuilder::CreateTlas(commandList, instances, updateTlas) with a valid updateTlas: new transforms, the tree kept
        void UpdateInstanceTransforms(const uint32_t* geometryIndices, const float* surfaceToWorld, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_transforms(m_svgf.Context(), geometryIndices, surfaceToWorld, n, commandList), "neb_gi_update_transforms");
        }
        // InstanceMask = 0 / 0xFF in that same update (RTCommon.h:90): submeshes hidden from every ray or shown again, the tree kept
        void SetVisibility(const uint32_t* geometryIndices, const uint8_t* visible, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_set_visibility(m_svgf.Context(), geometryIndices, visible, n, commandList), "neb_gi_set_visibility");
        }
        // one byte per geometry, 1 = visible; *nOut = the geometry count
        void GetVisibility(uint8_t* out, uint32_t capacity, uint32_t* nOut) const
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_get_visibility(m_svgf.Context(), out, capacity, nOut), "neb_gi_get_visibility");
        }
        // The material table and the textures uploaded again, the TLAS untouched (GIProcessedScene.cpp:16-137): new factors for materials, ...
        void UpdateMaterials(const uint32_t* materialIndices, const neb_material_desc* mats, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_materials(m_svgf.Context(), materialIndices, mats, n, commandList), "neb_gi_update_materials");
        }
        // ... another material for geometries (negative: none), ...
        void SetGeometryMaterials(const uint32_t* geometryIndices, const int32_t* materialIndices, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_set_geometry_materials(m_svgf.Context(), geometryIndices, materialIndices, n, commandList),
                          "neb_gi_set_geometry_materials");
        }
        // ... new texels for rectangles of textures, from host memory or (Device) from memory the device reads in stream order; the tree and the sun table are kept
        void UpdateTextures(const neb_texture_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_textures(m_svgf.Context(), updates, n, commandList), "neb_gi_update_textures");
        }
        void UpdateTexturesDevice(const neb_texture_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_textures_device(m_svgf.Context(), updates, n, commandList), "neb_gi_update_textures_device");
        }
        // diagnostics: the standalone footprint tables, then the material bundles, as the device holds them (host == nullptr: the size alone)
        void TextureTables(void* host, size_t capacity, size_t* bytes, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_debug_texture_tables(m_svgf.Context(), host, capacity, bytes, commandList), "neb_gi_debug_texture_tables");
        }
        // diagnostics: the shading records (lit bits, hints) in leaf order, the triangles behind them, then one neb_shade_records_info
        void ShadeRecords(void* host, size_t capacity, size_t* bytes, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_debug_shade_records(m_svgf.Context(), host, capacity, bytes, commandList), "neb_gi_debug_shade_records");
        }
        // No reference counterpart (its BLASes are built without ALLOW_UPDATE, RTAccelerationStructureBuilder.cpp:79): new object-space
        // vertices for ranges of submeshes -- a swaying drape, a skinned figure --, the tree refitted in place
        void UpdateVertices(const neb_vertex_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_vertices(m_svgf.Context(), updates, n, commandList), "neb_gi_update_vertices");
        }
        // ... the same with DEVICE pointers in the entries (a skinning or cloth kernel's output): read in stream order on commandList, never on the
        // host; the caller orders commandList behind the producer and keeps the sources until the stream has passed the update
        void UpdateVerticesDevice(const neb_vertex_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_update_vertices_device(m_svgf.Context(), updates, n, commandList), "neb_gi_update_vertices_device");
        }
        // Skinned submeshes: bind joints + weights to every vertex of a geometry (the bind pose is the pools as they are, in stream order) ...
        void SetSkin(const neb_skin_desc* skins, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_set_skin(m_svgf.Context(), skins, n, commandList), "neb_gi_set_skin");
        }
        // ... then one palette of joint matrices per geometry and frame: blended on the device from the bind pose, the tree refitted in place
        void SkinVertices(const neb_skin_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_skin_vertices(m_svgf.Context(), updates, n, commandList), "neb_gi_skin_vertices");
        }
        // Morph targets: bind per-target delta streams to every vertex of a geometry (the rest pose is the pools as they are, in stream order) ...
        void SetMorphTargets(const neb_morph_desc* descs, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_set_morph_targets(m_svgf.Context(), descs, n, commandList), "neb_gi_set_morph_targets");
        }
        // ... then one weight per target and frame, and the palette of a skinned geometry: blended (and skinned) on the device from the rest pose
        void MorphVertices(const neb_morph_update* updates, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_morph_vertices(m_svgf.Context(), updates, n, commandList), "neb_gi_morph_vertices");
        }
        // the pools' current contents of a geometry's vertices (normals / tangents may be null); waits for the copies
        void DownloadVertices(uint32_t geometry, uint32_t firstVertex, uint32_t numVertices, float* positions, float* normals, float* tangents,
                              neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_download_vertices(m_svgf.Context(), geometry, firstVertex, numVertices, positions, normals, tangents, commandList),
                          "neb_gi_download_vertices");
        }
        // {device-sourced updates accepted, refused on the device}; waits for the updates enqueued so far
        void UpdateStatus(uint64_t out[2]) { ThrowIfFailed(m_svgf.Context(), neb_gi_update_status(m_svgf.Context(), out), "neb_gi_update_status"); }
        // the exact world-space box of the scene; waits like UpdateStatus
        void SceneBox(float lo[3], float hi[3]) { ThrowIfFailed(m_svgf.Context(), neb_gi_scene_box(m_svgf.Context(), lo, hi), "neb_gi_scene_box"); }
        void SubmitCommandsGIPathtrace(const neb_gi_constants& globalConstants, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_trace(m_svgf.Context(), &globalConstants, commandList), "neb_gi_trace");
        }

        // The same dispatch in two command lists, for a renderer that keeps frames in flight (src/nri/Swapchain.h:15): the first half (ray
        // generation + closest-hit walk) touches only the G-buffer and GI records and may be recorded for frame f + 1 on another stream while
        // the second half of frame f (shade + shadow passes, adds into the radiance target) and its SVGF passes still execute.
        void SubmitCommandsGIPathtraceBegin(const neb_gi_constants& globalConstants, uint32_t row0, uint32_t row1, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_trace_begin(m_svgf.Context(), &globalConstants, row0, row1, commandList), "neb_gi_trace_begin");
        }
        void SubmitCommandsGIPathtraceFinish(neb_stream commandList, void* afterShadeEvent = nullptr)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_trace_finish(m_svgf.Context(), commandList, afterShadeEvent), "neb_gi_trace_finish");
        }

        // Ray queries (no reference counterpart as a call: DXR's inline RayQuery is the nearest thing): n rays from a device buffer against the
        // scene as the update calls have left it; hits = neb_ray_hit[n] on the device, or uint32_t[n] with NEB_RAYS_ANY_HIT in flags.
        // NEB_RAYS_SORT reorders the rays for coherence first.  Only enqueues -- a sorted call larger than any before it allocates and waits.
        void CastRays(const neb_ray* rays, uint32_t n, uint32_t flags, void* hits, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_cast_rays(m_svgf.Context(), rays, n, flags, hits, commandList), "neb_gi_cast_rays");
        }
        // The same rays, shaded at their closest hits (the inputs of a closest-hit shader): what = NEB_SHADE_SURFACE writes neb_ray_surface[n]
        // (constants may be null), NEB_SHADE_RADIANCE neb_ray_radiance[n]: sky on a miss, the sun's direct light through one disk-sampled shadow
        // ray on a hit (frameIndex seeds the draws).  flags: 0 or NEB_RAYS_SORT.  Only enqueues, as CastRays.
        void ShadeRays(const neb_ray* rays, uint32_t n, uint32_t what, uint32_t flags, const neb_gi_constants* constants, void* out, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_shade_rays(m_svgf.Context(), rays, n, what, flags, constants, out, commandList), "neb_gi_shade_rays");
        }
        // The same rays followed as the frame follows a path, up to constants->maxPathVertices - 1 segments (2..8): paths = neb_ray_path[n],
        // the radiance summed along each; vertices = null, or neb_path_vertex[n * (maxPathVertices - 1)], one record per segment.  With
        // maxPathVertices = 2 the record is NEB_SHADE_RADIANCE's.  flags: 0 or NEB_RAYS_SORT.  Only enqueues, as CastRays.
        void TracePaths(const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants, void* paths, void* vertices, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_trace_paths(m_svgf.Context(), rays, n, flags, constants, paths, vertices, commandList), "neb_gi_trace_paths");
        }

        // Probe baking: ProbeRays writes the n * samples rays of n probes (sample s of probe p is ray p * samples + s; what = NEB_BAKE_SH: the
        // sphere, NEB_BAKE_IRRADIANCE: cosine-distributed about the normal) and needs no scene; BakeProbes follows the same rays as TracePaths
        // would and reduces them on the device to neb_probe_record[n] -- second-order SH of the incoming radiance, or the irradiance -- with no
        // buffer for rays or paths.  samples: a multiple of 64 in 64..4096; flags: 0.  Only enqueues, as CastRays.
        void ProbeRays(const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t frameIndex, neb_ray* rays, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_probe_rays(m_svgf.Context(), probes, n, samples, what, frameIndex, rays, commandList), "neb_gi_probe_rays");
        }
        void BakeProbes(const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags, const neb_gi_constants* constants,
                        neb_probe_record* out, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_bake_probes(m_svgf.Context(), probes, n, samples, what, flags, constants, out, commandList), "neb_gi_bake_probes");
        }

        // Probe volumes: ProbeGrid writes the probes of a regular grid (what BakeProbes takes), AccumulateProbes folds one bake's records into
        // a sample-weighted running mean (a zeroed `acc` is a valid start), GatherProbes blends the eight NEB_BAKE_SH records around each point
        // into the irradiance for the point's normal (neb_probe_gather[n]).  None needs a scene.  Only enqueue, as CastRays.
        void ProbeGrid(const neb_probe_grid& grid, float tmin, float tmax, neb_probe* probes, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_probe_grid(m_svgf.Context(), &grid, tmin, tmax, probes, commandList), "neb_gi_probe_grid");
        }
        void AccumulateProbes(neb_probe_record* acc, const neb_probe_record* add, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_accumulate_probes(m_svgf.Context(), acc, add, n, commandList), "neb_gi_accumulate_probes");
        }
        void GatherProbes(const neb_probe_grid& grid, const neb_probe_record* records, const neb_probe* points, uint32_t n, neb_probe_gather* out,
                          neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_gather_probes(m_svgf.Context(), &grid, records, points, n, out, commandList), "neb_gi_gather_probes");
        }

        // Probe-lit frames: GBufferPoints writes the points ray generation shades at the pixels of rows [row0, row1) (what GatherProbes and
        // BakeProbes take); ProbeIndirect adds the grid's irradiance at every pixel, weighted as the frame's diffuse term, to radiance[cur]
        // -- the stand-in for the path-traced indirect term.  flags: 0 or NEB_INDIRECT_FRAME_WEIGHT (constants then needed).  rows: the
        // context's own where row1 == 0.  Neither needs a scene.  Only enqueue, as CastRays.
        void GBufferPoints(uint32_t row0, uint32_t row1, neb_probe* points, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gbuffer_points(m_svgf.Context(), row0, row1, points, commandList), "neb_gbuffer_points");
        }
        void ProbeIndirect(const neb_probe_grid& grid, const neb_probe_record* records, const neb_gi_constants* constants, uint32_t flags,
                           neb_stream commandList, uint32_t row0 = 0, uint32_t row1 = 0)
        {
            const int rc = row1 == 0 ? neb_gi_probe_indirect(m_svgf.Context(), &grid, records, constants, flags, commandList)
                                     : neb_gi_probe_indirect_rows(m_svgf.Context(), &grid, records, constants, flags, row0, row1, commandList);
            ThrowIfFailed(m_svgf.Context(), rc, "neb_gi_probe_indirect");
        }

        // Probe visibility: BakeVisibility walks the rays of ProbeRays(..., NEB_BAKE_SH, frameIndex) once and filters their distances (cut at
        // maxDistance) into neb_probe_visibility[n], an 8 x 8 octahedral map of distance moments per probe, in a buffer parallel to the
        // records; AccumulateVisibility folds one such bake into a running mean (a zeroed `acc` is a valid start; needs no scene);
        // GatherProbesVisible and ProbeIndirectVisible are GatherProbes and ProbeIndirect with a Chebyshev visibility factor per corner, looked
        // up toward the point moved by normalBias along its normal.  Only enqueue, as CastRays.
        void BakeVisibility(const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t frameIndex, float maxDistance, neb_probe_visibility* out,
                            neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_bake_visibility(m_svgf.Context(), probes, n, samples, frameIndex, maxDistance, out, commandList),
                          "neb_gi_bake_visibility");
        }
        void AccumulateVisibility(neb_probe_visibility* acc, const neb_probe_visibility* add, uint32_t n, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_accumulate_visibility(m_svgf.Context(), acc, add, n, commandList), "neb_gi_accumulate_visibility");
        }
        void GatherProbesVisible(const neb_probe_grid& grid, const neb_probe_record* records, const neb_probe_visibility* visibility, float normalBias,
                                 const neb_probe* points, uint32_t n, neb_probe_gather* out, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_gather_probes_visible(m_svgf.Context(), &grid, records, visibility, normalBias, points, n, out, commandList),
                          "neb_gi_gather_probes_visible");
        }
        void ProbeIndirectVisible(const neb_probe_grid& grid, const neb_probe_record* records, const neb_probe_visibility* visibility, float normalBias,
                                  const neb_gi_constants* constants, uint32_t flags, neb_stream commandList, uint32_t row0 = 0, uint32_t row1 = 0)
        {
            const int rc = row1 == 0 ? neb_gi_probe_indirect_visible(m_svgf.Context(), &grid, records, visibility, normalBias, constants, flags, commandList)
                                     : neb_gi_probe_indirect_visible_rows(m_svgf.Context(), &grid, records, visibility, normalBias, constants, flags, row0,
                                                                          row1, commandList);
            ThrowIfFailed(m_svgf.Context(), rc, "neb_gi_probe_indirect_visible");
        }

        // Probe feedback: TracePaths / BakeProbes whose paths end in a probe grid -- at a path's last possible vertex the grid's irradiance
        // (tail.records, gathered plain, or through tail.visibility with tail.normal_bias) stands for the bounces the path did not walk, so
        // that BakeProbes -> AccumulateProbes -> BakeProbesTail(the accumulated records) gains one bounce per update.  tail.flags: 0 or
        // NEB_TAIL_FRAME_WEIGHT.  The grid's buffers must not be the ones the call writes.  Only enqueue, as CastRays.
        void TracePathsTail(const neb_ray* rays, uint32_t n, uint32_t flags, const neb_gi_constants* constants, const neb_probe_tail& tail, void* paths,
                            void* vertices, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_trace_paths_tail(m_svgf.Context(), rays, n, flags, constants, &tail, paths, vertices, commandList),
                          "neb_gi_trace_paths_tail");
        }
        void BakeProbesTail(const neb_probe* probes, uint32_t n, uint32_t samples, uint32_t what, uint32_t flags, const neb_gi_constants* constants,
                            const neb_probe_tail& tail, neb_probe_record* out, neb_stream commandList)
        {
            ThrowIfFailed(m_svgf.Context(), neb_gi_bake_probes_tail(m_svgf.Context(), probes, n, samples, what, flags, constants, &tail, out, commandList),
                          "neb_gi_bake_probes_tail");
        }

        // the acceleration structure is built on the device; these report what came out of it
        uint32_t BvhDepth() const
        {
            uint32_t d = 0;
            ThrowIfFailed(m_svgf.Context(), neb_gi_bvh_depth(m_svgf.Context(), &d), "neb_gi_bvh_depth");
            return d;
        }

        // The sun-visibility table (no reference counterpart: the reference's shadow rays go to TraceRay, assets/shaders/pathtracer.hlsl:567-569) is built
        // and kept up to date by SubmitCommandsGIPathtrace itself; these report what it does.
        struct SunTableStats
        {
            uint64_t sidesLitPlus = 0, sidesLitMinus = 0, raysAnswered = 0, builds = 0;
            float lastBuildMs = 0.0f;      // 0 when no table has been built
            int shadowTailMode = -1;       // 0: the rays the table leaves go through the compacted lists, 1: through the sorted pass, -1: not measured yet for this table
        };
        SunTableStats GetSunTableStats(neb_stream commandList) const
        {
            SunTableStats s;
            uint64_t v[4] = {0, 0, 0, 0};
            ThrowIfFailed(m_svgf.Context(), neb_gi_sun_table_stats(m_svgf.Context(), v, commandList), "neb_gi_sun_table_stats");
            s.sidesLitPlus = v[0], s.sidesLitMinus = v[1], s.raysAnswered = v[2], s.builds = v[3];
            if (s.builds)
                ThrowIfFailed(m_svgf.Context(), neb_gi_sun_table_build_ms(m_svgf.Context(), &s.lastBuildMs), "neb_gi_sun_table_build_ms");
            ThrowIfFailed(m_svgf.Context(), neb_gi_shadow_tail_mode(m_svgf.Context(), &s.shadowTailMode, nullptr), "neb_gi_shadow_tail_mode");
            return s;
        }

    private:
        SVGFDenoiser& m_svgf;
    };

    // Halo exchange between the row strips of a multi-GPU frame (no reference counterpart: Nebulae is single-GPU).
    // One communicator per strip group; Exchange() enqueues one RCCL group of sends / receives on the caller's stream.
    // Threading: with one process or thread per GPU nothing else is needed.  ONE thread that drives several GPUs must put
    // the Init() calls of all its ranks, and the Exchange() calls of all its strips for one exchange, between
    // GroupBegin() and GroupEnd() (RCCL's rule for one thread with several devices; otherwise Init blocks for ever).
    class StripExchange
    {
    public:
        static void GroupBegin() { Check(neb_strips_group_begin(), "neb_strips_group_begin"); }
        static void GroupEnd() { Check(neb_strips_group_end(), "neb_strips_group_end"); }
        StripExchange() = default;
        StripExchange(const StripExchange&) = delete;
        StripExchange& operator=(const StripExchange&) = delete;
        ~StripExchange() { neb_strips_comm_destroy(m_comm); }
        static void MakeUniqueId(void* id128) { Check(neb_strips_unique_id(id128), "neb_strips_unique_id"); }
        void Init(int device, int numRanks, int rank, const void* id128)
        {
            Check(neb_strips_comm_create(device, numRanks, rank, id128, &m_comm), "neb_strips_comm_create");
        }
        void Exchange(SVGFDenoiser& strip, const neb_halo_plane* planes, uint32_t nPlanes, const neb_halo_swap* swaps, uint32_t nSwaps, neb_stream commandList)
        {
            ThrowIfFailed(strip.Context(), neb_strips_exchange(strip.Context(), m_comm, planes, nPlanes, swaps, nSwaps, commandList), "neb_strips_exchange");
        }
        // One call per strip frame (round 5): the GI dispatch on the strip's rows (constants == nullptr: none), the temporal pass, the halo
        // exchange(s) of the plan's scheme over this communicator and the a-trous levels on the row ranges the scheme prescribes.
        void SubmitStripFrame(SVGFDenoiser& strip, const neb_gi_constants* constants, const neb_strip_plan& plan, neb_stream commandList)
        {
            ThrowIfFailed(strip.Context(), neb_strip_frame(strip.Context(), constants, m_comm, &plan, commandList), "neb_strip_frame");
        }
        // The same for a host that drives all strips from ONE thread and needs no communicator (the neighbouring strips' contexts instead):
        // Begin for every strip, then Finish for every strip.
        static void SubmitStripFrameBegin(SVGFDenoiser& strip, const neb_gi_constants* constants, const neb_strip_plan& plan, SVGFDenoiser* up, SVGFDenoiser* down,
                                          neb_stream commandList)
        {
            const neb_strip_peers peers{up ? up->Context() : nullptr, down ? down->Context() : nullptr};
            ThrowIfFailed(strip.Context(), neb_strip_frame_begin(strip.Context(), constants, &plan, &peers, commandList), "neb_strip_frame_begin");
        }
        static void SubmitStripFrameFinish(SVGFDenoiser& strip, const neb_strip_plan& plan, SVGFDenoiser* up, SVGFDenoiser* down, neb_stream commandList)
        {
            const neb_strip_peers peers{up ? up->Context() : nullptr, down ? down->Context() : nullptr};
            ThrowIfFailed(strip.Context(), neb_strip_frame_finish(strip.Context(), nullptr, &plan, &peers, commandList), "neb_strip_frame_finish");
        }

    private:
        static void Check(int status, const char* what)
        {
            if (status != NEB_OK)
                throw NebException(status, std::string(what) + ": " + neb_strips_last_error());
        }
        void* m_comm = nullptr;
    };

} // namespace Neb
