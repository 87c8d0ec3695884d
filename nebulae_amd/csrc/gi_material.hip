// gi_material.hip -- what a submesh looks like, updated in place: material factors, the material a geometry names, texels of a map
// (neb_gi_update_materials, neb_gi_set_geometry_materials, neb_gi_update_textures[_device]).
//
// Reference: the material table and the textures of GIProcessedScene (src/nri/GIProcessedScene.cpp:16-137) are plain uploads that the
// reference repeats without touching its TLAS.  Here the counterpart of "upload the material table again" is two small kernels over
// the DevMat / DevGeom rows and the per-geometry ShadeHeader lines that copy them, and the counterpart of "upload the texture again" is
// a patch of the bilinear-footprint tables and material bundles the images were turned into (texture_patch.h): the device keeps no image.
// None of it touches triangles, nodes or shading records, so the tree and the sun table stay as they are.
#include <algorithm>

#include "gi_internal.h"
#include "texture_patch.h"

namespace neb {

// lane k: entry k of the update -> the factors of material `index` (geoms == nullptr) or the material of geometry `index`, and its stamp
__global__ void material_apply_kernel(const GiState::MatStage* __restrict__ stage, uint32_t n, uint32_t n_rows, uint32_t epoch, DevMat* __restrict__ mats,
                                      DevGeom* __restrict__ geoms, uint32_t* __restrict__ row_epoch)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const GiState::MatStage s = stage[k];
    if (s.index >= n_rows)
        return;
    if (geoms) {
        geoms[s.index].material = s.material;
    } else {
        DevMat& m = mats[s.index];
        m.albedo[0] = s.albedo[0], m.albedo[1] = s.albedo[1], m.albedo[2] = s.albedo[2];
        m.rough = s.rough, m.metal = s.metal;
    }
    row_epoch[s.index] = epoch;
}

// lane gi: the material half of the geometry's ShadeHeader (words q2.z .. q5.y) copied again from the two tables when the update in
// progress stamped the geometry or the material it names; m[9] and valid are not touched.  Copies only: the header holds what
// neb_gi_set_scene would have written for the same tables, bit for bit.
__global__ void shade_header_refresh_kernel(uint32_t n_geoms, uint32_t n_mats, uint32_t epoch, const DevGeom* __restrict__ geoms,
                                            const DevMat* __restrict__ mats, const uint32_t* __restrict__ mat_epoch,
                                            const uint32_t* __restrict__ geom_epoch, ShadeHeader* __restrict__ heads)
{
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n_geoms)
        return;
    const int32_t mi = geoms[gi].material;
    const bool has = mi >= 0 && (uint32_t)mi < n_mats;
    if (geom_epoch[gi] != epoch && !(has && mat_epoch[mi] == epoch))
        return;
    ShadeHeader& hd = heads[gi];
    hd.material = mi;
    if (has) {
        const DevMat mt = mats[mi];
        hd.bundle = mt.bundle, hd.bundle_w = mt.bundle_w, hd.bundle_h = mt.bundle_h;
        hd.tex[0] = mt.tex[0], hd.tex[1] = mt.tex[1], hd.tex[2] = mt.tex[2];
        hd.albedo[0] = mt.albedo[0], hd.albedo[1] = mt.albedo[1], hd.albedo[2] = mt.albedo[2];
        hd.rough = mt.rough, hd.metal = mt.metal;
    } else { // the fields of no material: zeros, tex = -1
        hd.bundle = hd.bundle_w = hd.bundle_h = 0u;
        hd.tex[0] = hd.tex[1] = hd.tex[2] = -1;
        hd.albedo[0] = hd.albedo[1] = hd.albedo[2] = 0.f;
        hd.rough = hd.metal = 0.f;
    }
}

// One lane per affected entry of ONE table (texture_patch.h): lanes run along x, so the source reads of a wavefront are one row piece
// and its stores contiguous 16-byte (standalone) or 32-byte (bundle) pieces.  A lane loads its entry whole, replaces the slots whose
// texel lies in the rectangle -- through the role mask for a bundle -- and stores it whole.  Every entry belongs to exactly one lane of
// a launch, and the launches of one call follow one another on the stream: no atomics, nothing to race with.  `table` starts at the
// texture's first entry (uint4 units: one per entry standalone, two per entry for a bundle).
template <bool BUNDLE>
__global__ __launch_bounds__(256) void texture_patch_kernel(texpatch::Patch p, const uint8_t* __restrict__ src, uint32_t pitch_bytes, uint32_t roles,
                                                            uint4* __restrict__ table)
{
    const uint32_t cols = texpatch::patch_cols(p), rows = texpatch::patch_rows(p);
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned long long)cols * rows) // (cols * rows <= w * h < 2^32)
        return;
    const uint32_t j = (uint32_t)idx / cols, i = (uint32_t)idx - j * cols;
    uint32_t ex, ey;
    texpatch::patch_entry(p, i, j, ex, ey);
    const size_t at = (size_t)ey * p.w + ex;
    if (BUNDLE) {
        const uint4 a = table[2 * at], b = table[2 * at + 1];
        uint32_t e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (texpatch::patch_bundle_entry(p, ex, ey, src, pitch_bytes, roles, e)) {
            table[2 * at] = make_uint4(e[0], e[1], e[2], e[3]);
            table[2 * at + 1] = make_uint4(e[4], e[5], e[6], e[7]);
        }
    } else {
        const uint4 a = table[at];
        uint32_t e[4] = {a.x, a.y, a.z, a.w};
        if (texpatch::patch_table_entry(p, ex, ey, src, pitch_bytes, e))
            table[at] = make_uint4(e[0], e[1], e[2], e[3]);
    }
}

// the launches of one rectangle: the texture's standalone table if it has one, then every bundle it sits in
static hipError_t enqueue_texture_patch(GiState* g, uint32_t tex, const texpatch::Patch& p, const uint8_t* src, uint32_t pitch_bytes, hipStream_t stream)
{
    const unsigned long long lanes = (unsigned long long)texpatch::patch_cols(p) * texpatch::patch_rows(p);
    const dim3 grid((unsigned)((lanes + 255u) / 256u)), block(256);
    uint4* tables = reinterpret_cast<uint4*>(const_cast<uint32_t*>(g->view.texels));
    uint4* bundles = const_cast<uint4*>(g->view.bundles);
    if (g->h_texs[tex].offset != 0xffffffffu)
        hipLaunchKernelGGL(texture_patch_kernel<false>, grid, block, 0, stream, p, src, pitch_bytes, 0u, tables + g->h_texs[tex].offset);
    for (uint32_t u = g->tex_use_first[tex]; u < g->tex_use_first[tex + 1]; ++u)
        hipLaunchKernelGGL(texture_patch_kernel<true>, grid, block, 0, stream, p, src, pitch_bytes, g->tex_uses[u].roles,
                           bundles + 2 * (size_t)g->tex_uses[u].bundle);
    return hipGetLastError();
}

// the stamps of the factor and reassignment calls: [n_mats] for the materials, then [n_geoms] for the geometries
static hipError_t material_stamps(GiState* g)
{
    if (g->d_mat_epoch)
        return hipSuccess;
    void* p = nullptr;
    const size_t bytes = ((size_t)g->h_mats.size() + g->n_geoms) * sizeof(uint32_t);
    if (hipError_t e = hipMalloc(&p, bytes); e != hipSuccess)
        return e;
    g->allocs.push_back(p);
    g->d_mat_epoch = (uint32_t*)p;
    return hipMemset(p, 0, bytes);
}

// The slot of update `call` for ns MatStage entries: in the h_stage ring where they fit (a reassignment always does), else in the
// h_vstage ring -- both rings share slots and events.
static hipError_t material_stage_slot(GiState* g, uint32_t call, uint32_t ns, int* slot, GiState::MatStage** st)
{
    const size_t bytes = (size_t)ns * sizeof(GiState::MatStage);
    const bool fits = g->h_stage && bytes <= (size_t)g->n_geoms * sizeof(GiState::StageEntry);
    if (!fits)
        if (hipError_t e = vstage_reserve(g, bytes, g->h_mats.size() * sizeof(GiState::MatStage)); e != hipSuccess)
            return e;
    if (hipError_t e = stage_slot_acquire(g, call, slot); e != hipSuccess)
        return e;
    *st = fits ? (GiState::MatStage*)(g->h_stage + (size_t)*slot * g->n_geoms) : (GiState::MatStage*)((uint8_t*)g->h_vstage + (size_t)*slot * g->vstage_cap);
    return hipSuccess;
}

// apply the staged entries, refresh the headers, release the slot, mark the rewrite
static int material_enqueue(neb_ctx* ctx, GiState* g, int slot, uint32_t call, const GiState::MatStage* st, uint32_t ns, bool reassign, hipStream_t stream)
{
    const uint32_t n_mats = (uint32_t)g->h_mats.size();
    uint32_t* mat_epoch = g->d_mat_epoch;
    uint32_t* geom_epoch = g->d_mat_epoch + n_mats;
    hipLaunchKernelGGL(material_apply_kernel, dim3((ns + 63) / 64), dim3(64), 0, stream, st, ns, reassign ? g->n_geoms : n_mats, call,
                       const_cast<DevMat*>(g->view.mats), reassign ? const_cast<DevGeom*>(g->view.geoms) : (DevGeom*)nullptr,
                       reassign ? geom_epoch : mat_epoch);
    GI_HIP(ctx, hipGetLastError());
    GI_HIP(ctx, stage_slot_release(g, slot, stream));
    if (g->n_geoms) {
        hipLaunchKernelGGL(shade_header_refresh_kernel, dim3((g->n_geoms + 63) / 64), dim3(64), 0, stream, g->n_geoms, n_mats, call, g->view.geoms, g->view.mats,
                           (const uint32_t*)mat_epoch, (const uint32_t*)geom_epoch, const_cast<ShadeHeader*>(g->shade_heads));
        GI_HIP(ctx, hipGetLastError());
    }
    GI_HIP(ctx, mark_rewrite(g, stream));
    return NEB_OK;
}

} // namespace neb

using namespace neb;

// what both texel calls check of their entries before anything changes; *total = the bytes of all rectangles, rows tight
static int texture_updates_check(neb_ctx* ctx, const GiState* g, const neb_texture_update* updates, uint32_t n, const char* who, size_t* total)
{
    char msg[160];
    *total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_texture_update& u = updates[k];
        const char* bad = nullptr;
        int code = NEB_ERR_INVALID_ARG;
        if (!u.rgba8)
            bad = "null source";
        else if (u.texture >= g->h_texs.size())
            bad = "texture index out of range", code = NEB_ERR_OUT_OF_RANGE;
        else if (!u.width || !u.height || u.x >= g->h_texs[u.texture].w || u.y >= g->h_texs[u.texture].h || u.width > g->h_texs[u.texture].w - u.x ||
                 u.height > g->h_texs[u.texture].h - u.y)
            bad = "a rectangle is empty or leaves its texture", code = NEB_ERR_OUT_OF_RANGE;
        else if ((u.pitchBytes & 3u) || (size_t)u.pitchBytes < 4u * (size_t)u.width)
            bad = "pitchBytes must be a multiple of 4 and at least 4 * width";
        if (bad) {
            snprintf(msg, sizeof(msg), "%s: %s", who, bad);
            return gi_fail(ctx, code, msg);
        }
        *total += (((size_t)4u * u.width * u.height) + 15u) & ~(size_t)15u;
    }
    return NEB_OK;
}

extern "C" {

int neb_gi_update_materials(neb_ctx* ctx, const uint32_t* material_indices, const neb_material_desc* mats, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_materials: no scene (neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!material_indices || !mats)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_materials: null pointer");
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t n_mats = (uint32_t)g->h_mats.size(), n_texs = (uint32_t)g->h_texs.size();
    const uint32_t stamp = ++g->seen_stamp; // (one per call, accepted or not: h_mat_seen needs no clearing)
    uint32_t n_changed = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t mi = material_indices[k];
        if (mi >= n_mats)
            return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_materials: material index out of range");
        if (g->h_mat_seen[mi] == stamp)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_materials: a material is named twice");
        g->h_mat_seen[mi] = stamp;
        const neb_material_desc& s = mats[k];
        const DevMat& d = g->h_mats[mi];
        for (int q = 0; q < 3; ++q) { // (as neb_gi_set_scene reads them: an index outside the texture table is "no map")
            const int32_t t = (s.textureIndices[q] >= 0 && (uint32_t)s.textureIndices[q] < n_texs) ? s.textureIndices[q] : -1;
            if (t != d.tex[q])
                return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_materials: textureIndices differ from the material's (the maps a material binds are fixed by neb_gi_set_scene)");
        }
        const float f[5] = {s.albedo[0], s.albedo[1], s.albedo[2], s.roughnessMetalness[0], s.roughnessMetalness[1]};
        for (int q = 0; q < 5; ++q)
            if (!(fabsf(f[q]) <= 3.4028235e38f))
                return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_materials: a factor is not a finite number");
        const float have[5] = {d.albedo[0], d.albedo[1], d.albedo[2], d.rough, d.metal};
        n_changed += memcmp(f, have, sizeof(f)) != 0 ? 1u : 0u;
    }
    if (n_changed == 0)
        return NEB_OK; // every material has the factors asked for: nothing is enqueued
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    GI_HIP(ctx, material_stamps(g));
    const uint32_t call = g->epoch + 1u;
    int slot = 0;
    GiState::MatStage* st = nullptr;
    GI_HIP(ctx, material_stage_slot(g, call, n_changed, &slot, &st));
    if (int rc = refit_order_behind_readers(ctx, g, stream); rc != NEB_OK)
        return rc;
    // ---- commit the host side ----
    g->epoch = call;
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        DevMat& d = g->h_mats[material_indices[k]];
        const neb_material_desc& s = mats[k];
        const float f[5] = {s.albedo[0], s.albedo[1], s.albedo[2], s.roughnessMetalness[0], s.roughnessMetalness[1]};
        const float have[5] = {d.albedo[0], d.albedo[1], d.albedo[2], d.rough, d.metal};
        if (!memcmp(f, have, sizeof(f)))
            continue;
        d.albedo[0] = f[0], d.albedo[1] = f[1], d.albedo[2] = f[2], d.rough = f[3], d.metal = f[4];
        st[ns++] = GiState::MatStage{material_indices[k], 0, {f[0], f[1], f[2]}, f[3], f[4], 0u};
    }
    return material_enqueue(ctx, g, slot, call, st, ns, false, stream);
}

int neb_gi_set_geometry_materials(neb_ctx* ctx, const uint32_t* geometry_indices, const int32_t* material_indices, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_set_geometry_materials: no scene (neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!geometry_indices || !material_indices)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_geometry_materials: null pointer");
    // ---- everything that can refuse the call comes before anything changes ----
    const uint32_t n_mats = (uint32_t)g->h_mats.size();
    const uint32_t stamp = ++g->seen_stamp;
    uint32_t n_changed = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gi = geometry_indices[k];
        if (gi >= g->n_geoms)
            return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_set_geometry_materials: geometry index out of range");
        if (g->h_seen[gi] == stamp)
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_set_geometry_materials: a geometry is named twice");
        g->h_seen[gi] = stamp;
        if (material_indices[k] >= 0 && (uint32_t)material_indices[k] >= n_mats)
            return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_set_geometry_materials: material index out of range");
        n_changed += (material_indices[k] < 0 ? -1 : material_indices[k]) != g->h_geom_mat[gi] ? 1u : 0u;
    }
    if (n_changed == 0)
        return NEB_OK; // every geometry names the material asked for: nothing is enqueued
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    GI_HIP(ctx, material_stamps(g));
    const uint32_t call = g->epoch + 1u;
    int slot = 0;
    GiState::MatStage* st = nullptr;
    GI_HIP(ctx, material_stage_slot(g, call, n_changed, &slot, &st));
    if (int rc = refit_order_behind_readers(ctx, g, stream); rc != NEB_OK)
        return rc;
    // ---- commit the host side ----
    g->epoch = call;
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const int32_t mi = material_indices[k] < 0 ? -1 : material_indices[k];
        if (mi == g->h_geom_mat[geometry_indices[k]])
            continue;
        g->h_geom_mat[geometry_indices[k]] = mi;
        st[ns++] = GiState::MatStage{geometry_indices[k], mi, {0.f, 0.f, 0.f}, 0.f, 0.f, 0u};
    }
    return material_enqueue(ctx, g, slot, call, st, ns, true, stream);
}

int neb_gi_update_textures(neb_ctx* ctx, const neb_texture_update* updates, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_textures: no scene (neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_textures: null pointer");
    size_t total = 0;
    if (int rc = texture_updates_check(ctx, g, updates, n, "neb_gi_update_textures", &total); rc != NEB_OK)
        return rc;
    if (total > ((size_t)64 << 20)) // (the ring holds kStageSlots slots of the largest call seen, in pinned memory)
        return gi_fail(ctx, NEB_ERR_OUT_OF_RANGE, "neb_gi_update_textures: the rectangles of one call total more than 64 MB (split the call, or use neb_gi_update_textures_device)");
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    // ---- the staging slot: pinned host memory, the rectangles one after another, rows tight; and its device copy ----
    GI_HIP(ctx, vstage_reserve(g, total, total));
    if (total > g->d_tstage_cap) {
        void* fresh = nullptr;
        const size_t cap = (total + 4095u) & ~(size_t)4095u;
        GI_HIP(ctx, hipMalloc(&fresh, cap));
        if (g->d_tstage)
            (void)hipFree(g->d_tstage); // (waits for the device: the update that read it is done)
        g->d_tstage = fresh;
        g->d_tstage_cap = cap;
    }
    const uint32_t call = g->epoch + 1u;
    int slot = 0;
    GI_HIP(ctx, stage_slot_acquire(g, call, &slot));
    if (int rc = refit_order_behind_readers(ctx, g, stream); rc != NEB_OK)
        return rc;
    g->epoch = call;
    uint8_t* base = (uint8_t*)g->h_vstage + (size_t)slot * g->vstage_cap;
    size_t off = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_texture_update& u = updates[k];
        for (uint32_t row = 0; row < u.height; ++row)
            memcpy(base + off + (size_t)row * 4u * u.width, (const uint8_t*)u.rgba8 + (size_t)row * u.pitchBytes, (size_t)4u * u.width);
        off += (((size_t)4u * u.width * u.height) + 15u) & ~(size_t)15u;
    }
    // ---- enqueue ----
    GI_HIP(ctx, hipMemcpyAsync(g->d_tstage, base, total, hipMemcpyHostToDevice, stream));
    GI_HIP(ctx, stage_slot_release(g, slot, stream));
    off = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const neb_texture_update& u = updates[k];
        const texpatch::Patch p{g->h_texs[u.texture].w, g->h_texs[u.texture].h, u.x, u.y, u.width, u.height};
        GI_HIP(ctx, enqueue_texture_patch(g, u.texture, p, (const uint8_t*)g->d_tstage + off, 4u * u.width, stream));
        off += (((size_t)4u * u.width * u.height) + 15u) & ~(size_t)15u;
    }
    GI_HIP(ctx, mark_rewrite(g, stream));
    return NEB_OK;
}

int neb_gi_update_textures_device(neb_ctx* ctx, const neb_texture_update* updates, uint32_t n, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_update_textures_device: no scene (neb_gi_set_scene first)");
    if (n == 0)
        return NEB_OK;
    if (!updates)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_textures_device: null pointer");
    size_t total = 0;
    if (int rc = texture_updates_check(ctx, g, updates, n, "neb_gi_update_textures_device", &total); rc != NEB_OK)
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    for (uint32_t k = 0; k < n; ++k) { // (the patch kernels read whole texels: 4-byte loads at the source's own address)
        const neb_texture_update& u = updates[k];
        if (((uintptr_t)u.rgba8 & 3u) || !device_readable(ctx, u.rgba8, (size_t)(u.height - 1u) * u.pitchBytes + (size_t)4u * u.width))
            return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_update_textures_device: a source is not 4-byte aligned memory this device can read over the whole rectangle");
    }
    if (int rc = refit_order_behind_readers(ctx, g, stream); rc != NEB_OK)
        return rc;
    // ---- enqueue: the arguments travel with the launches, the sources are read where they lie, in stream order ----
    for (uint32_t k = 0; k < n; ++k) {
        const neb_texture_update& u = updates[k];
        const texpatch::Patch p{g->h_texs[u.texture].w, g->h_texs[u.texture].h, u.x, u.y, u.width, u.height};
        GI_HIP(ctx, enqueue_texture_patch(g, u.texture, p, (const uint8_t*)u.rgba8, u.pitchBytes, stream));
    }
    GI_HIP(ctx, mark_rewrite(g, stream));
    return NEB_OK;
}

int neb_gi_debug_texture_tables(neb_ctx* ctx, void* host, size_t capacity, size_t* bytes, neb_stream stream_)
{
    if (!ctx)
        return NEB_ERR_INVALID_ARG;
    GiState* g = ctx->gi;
    if (!g)
        return gi_fail(ctx, NEB_ERR_STATE, "neb_gi_debug_texture_tables: no scene (neb_gi_set_scene first)");
    const size_t need = g->table_bytes + g->bundle_bytes;
    if (bytes)
        *bytes = need;
    if (!host || capacity == 0)
        return NEB_OK; // (the size alone)
    if (capacity < need)
        return gi_fail(ctx, NEB_ERR_INVALID_ARG, "neb_gi_debug_texture_tables: capacity below the tables' size");
    hipStream_t stream = (hipStream_t)stream_;
    GI_GUARD(ctx);
    GI_HIP(ctx, gi_scene_reader(g, stream));
    if (g->table_bytes)
        GI_HIP(ctx, hipMemcpyAsync(host, g->view.texels, g->table_bytes, hipMemcpyDeviceToHost, stream));
    if (g->bundle_bytes)
        GI_HIP(ctx, hipMemcpyAsync((uint8_t*)host + g->table_bytes, g->view.bundles, g->bundle_bytes, hipMemcpyDeviceToHost, stream));
    GI_HIP(ctx, hipStreamSynchronize(stream));
    return NEB_OK;
}

} // extern "C"
