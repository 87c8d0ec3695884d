// visibility_host_san.hip -- the host half of neb_gi_set_visibility / neb_gi_get_visibility (validation, state, the scene-box fold) as a
// stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer.  It needs no GPU and loads into no interpreter: the state the
// calls look at is made by hand, every call below ends before its first launch (a refusal, "nothing left", or -- without a device --
// the failing hipSetDevice of the guard, which must leave the state as it was).  Build container only, never on the GPU box:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -fno-slp-vectorize -w -fsanitize=address,undefined -fno-gpu-sanitize
//         -fno-omit-frame-pointer tools/visibility_host_san.hip nebulae_amd/csrc/{api,svgf,gi,gi_build,gi_refit,gi_sun_table,raysort,strips}.hip
//         -ldl -o build_variants/visibility_host_san && build_variants/visibility_host_san
#include <cstdio>
#include <cstdlib>

#include "../nebulae_amd/csrc/gi_internal.h"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main()
{
    using neb::GiState;
    constexpr uint32_t N = 4;
    neb_ctx* ctx = new neb_ctx();
    GiState* g = new GiState();
    g->n_geoms = N;
    g->h_geoms.resize(N);
    g->h_seen.assign(N, 0u);
    g->h_visible.assign(N, 1);
    for (uint32_t gi = 0; gi < N; ++gi) { // unit boxes side by side along x; geometry 3 has no triangle
        GiState::HostGeom& hg = g->h_geoms[gi];
        hg.n_tris = gi == 3 ? 0u : 2u;
        for (int q = 0; q < 3; ++q)
            hg.world_lo[q] = q == 0 ? (float)gi : -1.0f, hg.world_hi[q] = q == 0 ? (float)gi + 1.0f : 1.0f;
    }
    ctx->gi = g;
    uint32_t idx[6] = {0, 1, 2, 3, 0, 7};
    uint8_t vis[6] = {1, 1, 1, 1, 1, 1}, out[8];
    uint32_t n = 99;
    // before a build
    CHECK(neb_gi_set_visibility(ctx, idx, vis, 1, nullptr) == NEB_ERR_STATE);
    g->built = true;
    // refusals, in the documented order of precedence
    CHECK(neb_gi_set_visibility(nullptr, idx, vis, 1, nullptr) == NEB_ERR_INVALID_ARG);
    CHECK(neb_gi_set_visibility(ctx, nullptr, nullptr, 0, nullptr) == NEB_OK);
    CHECK(neb_gi_set_visibility(ctx, nullptr, vis, 1, nullptr) == NEB_ERR_INVALID_ARG);
    CHECK(neb_gi_set_visibility(ctx, idx, nullptr, 1, nullptr) == NEB_ERR_INVALID_ARG);
    CHECK(neb_gi_set_visibility(ctx, idx + 5, vis, 1, nullptr) == NEB_ERR_OUT_OF_RANGE);
    CHECK(neb_gi_set_visibility(ctx, idx, vis, 5, nullptr) == NEB_ERR_INVALID_ARG); // (0 named twice)
    CHECK(neb_gi_set_visibility(ctx, idx, vis, 6, nullptr) == NEB_ERR_INVALID_ARG); // (more entries than geometries: the duplicate comes first)
    CHECK(ctx->last_error.find("neb_gi_set_visibility") != std::string::npos);
    // entries that change nothing are dropped: nothing is enqueued, no device is asked for
    CHECK(neb_gi_set_visibility(ctx, idx, vis, 4, nullptr) == NEB_OK);
    CHECK(g->epoch == 0 && g->n_hidden == 0);
    // an entry that does change a flag reaches the device guard; whatever it answers here, a failure leaves the state as it was
    vis[1] = 0;
    const int rc = neb_gi_set_visibility(ctx, idx, vis, 4, nullptr);
    CHECK(rc == NEB_ERR_HIP || rc == NEB_OK);
    if (rc == NEB_ERR_HIP)
        CHECK(g->epoch == 0 && g->n_hidden == 0 && g->h_visible[1] == 1);
    // the flags as the host holds them: either output alone, a short buffer
    g->h_visible = {1, 0, 1, 0};
    CHECK(neb_gi_get_visibility(nullptr, out, 8, &n) == NEB_ERR_INVALID_ARG && n == 99);
    CHECK(neb_gi_get_visibility(ctx, nullptr, 0, &n) == NEB_OK && n == N);
    CHECK(neb_gi_get_visibility(ctx, nullptr, 2, nullptr) == NEB_ERR_INVALID_ARG);
    memset(out, 9, sizeof(out));
    CHECK(neb_gi_get_visibility(ctx, out, 3, nullptr) == NEB_OK && out[0] == 1 && out[1] == 0 && out[2] == 1 && out[3] == 9);
    CHECK(neb_gi_get_visibility(ctx, out, 8, &n) == NEB_OK && out[3] == 0 && out[4] == 9);
    // the box fold: visible geometries with triangles only; all of them for the build; the zero box when nothing is left
    float lo[3], hi[3];
    neb::gi_fold_scene_box(g, true, lo, hi);
    CHECK(lo[0] == 0.0f && hi[0] == 3.0f && lo[1] == -1.0f && hi[2] == 1.0f); // geometries 0 and 2 (1 is hidden, 3 has no triangle)
    neb::gi_fold_scene_box(g, false, lo, hi);
    CHECK(lo[0] == 0.0f && hi[0] == 3.0f);
    g->h_visible = {0, 1, 0, 1};
    neb::gi_fold_scene_box(g, true, lo, hi);
    CHECK(lo[0] == 1.0f && hi[0] == 2.0f);
    g->h_visible = {0, 0, 0, 1};
    neb::gi_fold_scene_box(g, true, lo, hi);
    for (int q = 0; q < 3; ++q)
        CHECK(lo[q] == 0.0f && hi[q] == 0.0f);
    ctx->gi = nullptr;
    delete g;
    delete ctx;
    printf("visibility_host_san: ok\n");
    return 0;
}
