// svgf.hip -- SVGF temporal accumulation and edge-stopping a-trous wavelet for gfx950.
//
// Reference arithmetic (paths relative to the reference checkout):
//   assets/shaders/svgf_temporal.hlsl:24-68  -> svgf_temporal_kernel, and the staging phase of the fused level-0 kernel
//   assets/shaders/svgf_atrous.hlsl:29-85    -> svgf_atrous_direct_kernel / svgf_atrous_lds_kernel
// This is not a transliteration of the 8x8-threadgroup texture-fetch shaders: the temporal
// pass is a coalesced stream (one pixel per lane, 16-B radiance accesses); the a-trous pass
// is tiled on the row lattice {r + step*j} so that a workgroup's taps are whole, contiguous
// image-row segments whatever the step, staged once into LDS with depth and normals already
// decoded, and each lane filters a column of R lattice rows so every staged texel is
// read from LDS once per R outputs.  A whole frame's denoise (neb_svgf_temporal followed by neb_svgf_atrous) runs
// the temporal pass INSIDE the staging phase of level 0 and never writes the accumulated radiance.  See DESIGN.md "Kernels".
#pragma clang fp contract(off) // fused operations are explicit fmaf: see neb_device.h

#include <algorithm>
#include <atomic>

#include "neb_device.h"
#include "neb_internal.h"
#include "svgf_demod.h"
#include "svgf_reproject.h"

// Tuning knobs (tools/build_variant.sh): the product is built with none of them set.
#ifndef NEB_ATROUS_PER_CU_R2 // most workgroups per CU of the R = 2 tiles (= waves per SIMD = the register budget: 4 -> 128 registers)
#define NEB_ATROUS_PER_CU_R2 4
#endif
#ifndef NEB_ATROUS_XGROUP // pixels per column group of the x lattice (see AtrousTile); >= 64 = consecutive columns at every step
#define NEB_ATROUS_XGROUP 8
#endif

namespace neb {

// ------------------------------------------------------------------------------------------
// Temporal accumulation: 60 B read + 22 B written per pixel, pure stream.
// ------------------------------------------------------------------------------------------
struct TemporalArgs {
    float4* rad_cur;
    const float4* rad_hist;
    const uint32_t* depth_cur;
    const uint32_t* depth_hist;
    const uint2* normal_cur;
    const uint2* normal_hist;
    const uint32_t* mom_hist;
    uint32_t* mom_cur;
    uint16_t* variance;
    float4* geometry;               // {decoded shading normal, depth} of the current frame for the a-trous levels, or null
    uint32_t W, Wd, row_off, nrows; // row_off = row0 - row_begin
    float neg_inv_two_sigma2_log2e, alpha, varianceEps;
};

// The temporal pass's arithmetic, shared word for word by svgf_temporal_kernel and by the staging phase of the fused
// level-0 a-trous kernel (so a frame denoised through either gives the same bits).
// lerp parameter of svgf_temporal.hlsl:44-51; also returns the decoded shading normal and depth of the current frame
__device__ __forceinline__ float temporal_blend(uint32_t dc, uint32_t dh, uint32_t nc, uint32_t nh, float neg_inv_two_sigma2_log2e, float alpha_param,
                                                float3& Nc, float& zc)
{
    Nc = oct16_unpack_zw(nc);
    const float3 Nh = oct16_unpack_zw(nh);
    zc = depth_unorm24(dc);
    const float dz = fabsf(zc - depth_unorm24(dh));
    // SVGF_DWeight: exp(-dz^2 / (2 sigma^2))   (svgf_common.hlsli:11-15)
    const float wDepth = fast_exp2(dz * dz * neg_inv_two_sigma2_log2e);
    // SVGF_NWeight: saturate(dot)               (svgf_common.hlsli:4-7)
    const float wNormal = __saturatef(fmaf(Nc.z, Nh.z, fmaf(Nc.y, Nh.y, Nc.x * Nh.x)));
    const float w = wDepth * wNormal;
    return fmaf(w, alpha_param - 1.0f, 1.0f); // lerp(1, alpha, w)  (:51)
}

// Caccum = lerp(Ccurr, Chist, alpha)  (:55); alpha channel carried from the current frame
__device__ __forceinline__ float4 temporal_accumulate(float4 Cc, float4 Ch, float alpha)
{
    float4 out;
    out.x = fmaf(alpha, Ch.x - Cc.x, Cc.x);
    out.y = fmaf(alpha, Ch.y - Cc.y, Cc.y);
    out.z = fmaf(alpha, Ch.z - Cc.z, Cc.z);
    out.w = Cc.w;
    return out;
}

// moments and variance (:57-67), as the typed R16G16_FLOAT / R16_FLOAT stores leave them: {moments bits, variance bits}
// (history moments as floats: the reprojecting pass resamples them)
__device__ __forceinline__ uint2 temporal_moments_f(float4 Cc, float Mh0, float Mh1, float alpha, float varianceEps)
{
    const float Y = luminance(Cc.x, Cc.y, Cc.z);
    const float M1 = fmaf(alpha, Mh0 - Y, Y);
    const float Y2 = Y * Y;
    const float M2 = fmaf(alpha, Mh1 - Y2, Y2);
    const float var = fmaxf(fmaf(-M1, M1, M2), varianceEps);
    return make_uint2(float_to_half_bits(M1) | (float_to_half_bits(M2) << 16), float_to_half_bits(var));
}

__device__ __forceinline__ uint2 temporal_moments(float4 Cc, uint32_t mh, float alpha, float varianceEps)
{
    return temporal_moments_f(Cc, half_bits_to_float(mh & 0xffffu), half_bits_to_float(mh >> 16), alpha, varianceEps);
}

// DEMOD (option svgf_demodulate): the pixel's own radiance is divided by its albedo divisor on load -- the albedo word is one more
// load of the pixel's single round trip -- and a.rad_hist is the demod plane, which needs no albedo.  Moments, variance and the accumulated
// colour are then those of the demodulated signal.  DEMOD = false is the kernel as it was: `albedo` is not read and the code is the same.
template <bool DEMOD>
__device__ __forceinline__ void temporal_pixel(const TemporalArgs& a, const uint32_t* __restrict__ albedo)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= a.Wd * a.nrows)
        return;
    const uint32_t ry = gid / a.Wd;
    const uint32_t x = gid - ry * a.Wd;
    const size_t i = (size_t)(a.row_off + ry) * a.W + x;

    float4 Cc = a.rad_cur[i];
    const float4 Ch = a.rad_hist[i];
    const uint32_t dc = a.depth_cur[i], dh = a.depth_hist[i];
    const uint32_t nc = a.normal_cur[i].y, nh = a.normal_hist[i].y; // .zw = shading normal
    const uint32_t mh = a.mom_hist[i];
    if constexpr (DEMOD)
        Cc = demodulate(Cc, albedo[i]);

    float3 Nc;
    float zc;
    const float alpha = temporal_blend(dc, dh, nc, nh, a.neg_inv_two_sigma2_log2e, a.alpha, Nc, zc);
    if (a.geometry) // decoded once here instead of once per a-trous level and staged texel
        a.geometry[i] = make_float4(Nc.x, Nc.y, Nc.z, zc);
    const uint2 mv = temporal_moments(Cc, mh, alpha, a.varianceEps);
    a.rad_cur[i] = temporal_accumulate(Cc, Ch, alpha);
    a.mom_cur[i] = mv.x;
    a.variance[i] = (uint16_t)mv.y;
}

__global__ __launch_bounds__(256) void svgf_temporal_kernel(TemporalArgs a) { temporal_pixel<false>(a, nullptr); }
__global__ __launch_bounds__(256) void svgf_temporal_demod_kernel(TemporalArgs a, const uint32_t* __restrict__ albedo) { temporal_pixel<true>(a, albedo); }

// Option svgf_demodulate: the stand-in history of a frame whose demod plane does not hold the last denoised frame (see the validity rule in
// nebulae_hip.h) -- radiance[hist] over its own albedo, exact for a static camera.  Every resident pixel, 36 B each.
__global__ __launch_bounds__(256) void svgf_demod_seed_kernel(const float4* __restrict__ rad_hist, const uint32_t* __restrict__ albedo,
                                                              float4* __restrict__ demod, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    demod[i] = demodulate(rad_hist[i], albedo[i]);
}

hipError_t launch_demod_seed(const float4* rad_hist, const uint32_t* albedo, float4* demod, size_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(svgf_demod_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rad_hist, albedo, demod, n);
    return hipGetLastError();
}

hipError_t launch_temporal(const SvgfLaunch& L, float4* rad_cur, const float4* rad_hist, const uint32_t* depth_cur,
                           const uint32_t* depth_hist, const uint2* normal_cur, const uint2* normal_hist,
                           const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance, float4* geometry, hipStream_t s,
                           const uint32_t* demod_albedo)
{
    const uint32_t Wd = (L.W / 8u) * 8u, Hd = (L.H / 8u) * 8u; // Dispatch(W/8,H/8): SVGFDenoiser.cpp:116
    const uint32_t row1 = L.row1 < Hd ? L.row1 : Hd;
    if (L.row0 >= row1 || Wd == 0)
        return hipSuccess;
    TemporalArgs a;
    a.rad_cur = rad_cur;
    a.rad_hist = rad_hist;
    a.depth_cur = depth_cur;
    a.depth_hist = depth_hist;
    a.normal_cur = normal_cur;
    a.normal_hist = normal_hist;
    a.mom_hist = mom_hist;
    a.mom_cur = mom_cur;
    a.variance = variance;
    a.geometry = geometry;
    a.W = L.W;
    a.Wd = Wd;
    a.row_off = L.row0 - L.row_begin;
    a.nrows = row1 - L.row0;
    a.neg_inv_two_sigma2_log2e = -kLog2e / (2.0f * L.p.depthSigma * L.p.depthSigma);
    a.alpha = L.p.alpha;
    a.varianceEps = L.p.varianceEps;
    const uint64_t n = (uint64_t)Wd * a.nrows;
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    if (demod_albedo)
        hipLaunchKernelGGL(svgf_temporal_demod_kernel, dim3(blocks), dim3(256), 0, s, a, demod_albedo);
    else
        hipLaunchKernelGGL(svgf_temporal_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Reprojecting temporal accumulation (option svgf_reproject; the mode is documented at neb_svgf_set_camera in nebulae_hip.h).
// One pixel per lane, an 8x8 tile per wave (the 2x2 history gathers of neighbouring lanes then fall on the same lines), four
// tiles side by side per 256-lane workgroup; cameras are kernel arguments (SGPRs); every operation is an IEEE fp32 one in the
// order tests/reproject_ref.py repeats (explicit fmaf, correctly rounded divisions), so the CPU reference reaches the same
// tap positions bit for bit.  No LDS.
// ------------------------------------------------------------------------------------------
struct ReprojCam {
    float ex, ey, ez;             // eye
    float xx, xy, xz;             // x axis
    float yx, yy, yz;             // y axis
    float zx, zy, zz;             // z axis (points from the target to the eye)
    float sx, sy;                 // aspect * tan(vfov / 2), tan(vfov / 2): NDC -> view plane
    float m22, m32;               // depth mapping of XMMatrixPerspectiveFovRH
};

struct ReprojArgs {
    float4* rad_cur;
    const float4* rad_hist;
    const uint32_t* depth_cur;
    const uint32_t* depth_hist;
    const uint2* normal_cur;
    const uint2* normal_hist;
    const uint32_t* mom_hist;
    uint32_t* mom_cur;
    uint16_t* variance;
    const uint8_t* hlen_hist;
    uint8_t* hlen_cur;
    float4* geometry;             // as TemporalArgs::geometry (null: not written)
    uint32_t W, tiles_x, n_tiles;
    int Wd, Hd;
    float inv_W, inv_H, half_W, half_H;
    float alpha, varianceEps;
    int hist_ok;                  // 0: no camera for the history slot -- no history anywhere
    ReprojCam cc, ch;             // cameras of cur and hist
};

// world point of pixel (x, y) at stored depth d (D24 unorm) seen by camera c: gbuffer_kernel's mapping inverted
__device__ __forceinline__ float3 reproj_world_point(const ReprojCam& c, float inv_W, float inv_H, int x, int y, float d)
{
    const float ndc_x = fmaf(((float)x + 0.5f) * inv_W, 2.0f, -1.0f);
    const float ndc_y = fmaf(((float)y + 0.5f) * inv_H, -2.0f, 1.0f);
    const float a = ndc_x * c.sx, b = ndc_y * c.sy;
    const float z = c.m32 / (d + c.m22); // linear depth -z_view
    const float vx = fmaf(c.xx, a, fmaf(c.yx, b, -c.zx));
    const float vy = fmaf(c.xy, a, fmaf(c.yy, b, -c.zy));
    const float vz = fmaf(c.xz, a, fmaf(c.yz, b, -c.zz));
    return make_float3(fmaf(vx, z, c.ex), fmaf(vy, z, c.ey), fmaf(vz, z, c.ez));
}

__device__ __forceinline__ bool d24_surface(uint32_t d) { return (d & 0xffffffu) != 0xffffffu; }

// Option svgf_motion: the per-geometry delta table.  One lane per geometry; the two slots' 4x4 (row-vector convention: world =
// (p, 1) . M, upper 3x3 A, translation t in row 3) -> flag, D = M_cur^-1 . M_hist (4x3) and K = (A_hist^-1 . A_cur)^T.  Double
// precision in ONE written-down order, which tests/motion_ref.py repeats in float64 and must meet bit for bit:
//   inverse of a 3x3: the nine cofactors, each "product - product"; det = (a00 c00 + a01 c01) + a02 c02; r = 1 / det;
//                     inv[i][j] = c[j][i] * r
//   3x3 product:      (X Y)[i][j] = (x[i][0] y[0][j] + x[i][1] y[1][j]) + x[i][2] y[2][j]
//   D rows 0..2 = inv(A_cur) A_hist;  translation last: D row 3 [j] = t_hist[j] - ((t_cur[0] D[0][j] + t_cur[1] D[1][j]) + t_cur[2] D[2][j])
//   K[i][j] = (inv(A_hist) A_cur)[j][i];  one rounding to fp32 at the end.
// No contraction: this file is compiled with fp contract off, so every product and sum is a v_mul_f64 / v_add_f64 of its own
// (checked in the ISA: the kernel holds no v_fma_f64 outside the division's expansion).
struct Mat3d { double m[3][3]; };
__device__ __forceinline__ bool delta_inverse(const Mat3d& a, Mat3d& inv)
{
    double c[3][3];
    c[0][0] = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
    c[0][1] = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
    c[0][2] = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
    c[1][0] = a.m[0][2] * a.m[2][1] - a.m[0][1] * a.m[2][2];
    c[1][1] = a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0];
    c[1][2] = a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1];
    c[2][0] = a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1];
    c[2][1] = a.m[0][2] * a.m[1][0] - a.m[0][0] * a.m[1][2];
    c[2][2] = a.m[0][0] * a.m[1][1] - a.m[0][1] * a.m[1][0];
    const double det = (a.m[0][0] * c[0][0] + a.m[0][1] * c[0][1]) + a.m[0][2] * c[0][2];
    const double r = 1.0 / det;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            inv.m[i][j] = c[j][i] * r;
    return det != 0.0 && fabs(det) <= 1.7e308 && fabs(r) <= 1.7e308; // (false for NaN too)
}
__device__ __forceinline__ Mat3d delta_product(const Mat3d& x, const Mat3d& y)
{
    Mat3d o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.m[i][j] = (x.m[i][0] * y.m[0][j] + x.m[i][1] * y.m[1][j]) + x.m[i][2] * y.m[2][j];
    return o;
}

__global__ __launch_bounds__(64) void reproj_delta_kernel(const float* __restrict__ xf_cur, const float* __restrict__ xf_hist,
                                                          float4* __restrict__ delta, uint32_t n)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= n)
        return;
    const float4* mc4 = reinterpret_cast<const float4*>(xf_cur) + 4 * (size_t)g;
    const float4* mh4 = reinterpret_cast<const float4*>(xf_hist) + 4 * (size_t)g;
    float mc[16], mh[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 c = mc4[r], h = mh4[r];
        mc[4 * r] = c.x, mc[4 * r + 1] = c.y, mc[4 * r + 2] = c.z, mc[4 * r + 3] = c.w;
        mh[4 * r] = h.x, mh[4 * r + 1] = h.y, mh[4 * r + 2] = h.z, mh[4 * r + 3] = h.w;
    }
    bool same = true, finite = true;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        same = same && __float_as_uint(mc[q]) == __float_as_uint(mh[q]);
        finite = finite && fabsf(mc[q]) <= 3.0e38f && fabsf(mh[q]) <= 3.0e38f;
    }
    float d[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    float k[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    uint32_t flag = kReprojDeltaSame;
    if (!same) {
        Mat3d ac, ah, ic, ih;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ac.m[i][j] = (double)mc[4 * i + j];
                ah.m[i][j] = (double)mh[4 * i + j];
            }
        const bool ok_c = delta_inverse(ac, ic), ok_h = delta_inverse(ah, ih);
        const Mat3d L = delta_product(ic, ah), Q = delta_product(ih, ac);
        bool ok = finite && ok_c && ok_h;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double tj = (double)mh[12 + j] - (((double)mc[12] * L.m[0][j] + (double)mc[13] * L.m[1][j]) + (double)mc[14] * L.m[2][j]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                d[3 * i + j] = (float)L.m[i][j];
                k[3 * i + j] = (float)Q.m[j][i];
            }
            d[9 + j] = (float)tj;
        }
#pragma unroll
        for (int q = 0; q < 12; ++q)
            ok = ok && fabsf(d[q]) <= 3.0e38f;
#pragma unroll
        for (int q = 0; q < 9; ++q)
            ok = ok && fabsf(k[q]) <= 3.0e38f;
        flag = ok ? kReprojDeltaMoved : kReprojDeltaSingular;
        if (!ok) {
#pragma unroll
            for (int q = 0; q < 12; ++q)
                d[q] = 0.f;
#pragma unroll
            for (int q = 0; q < 9; ++q)
                k[q] = 0.f;
        }
    }
    float4* e = delta + (size_t)kReprojDeltaFloat4 * g;
    e[0] = make_float4(__uint_as_float(flag), 0.f, 0.f, 0.f);
    e[1] = make_float4(d[0], d[1], d[2], d[3]);
    e[2] = make_float4(d[4], d[5], d[6], d[7]);
    e[3] = make_float4(d[8], d[9], d[10], d[11]);
    e[4] = make_float4(k[0], k[1], k[2], k[3]);
    e[5] = make_float4(k[4], k[5], k[6], k[7]);
    e[6] = make_float4(k[8], 0.f, 0.f, 0.f);
    e[7] = make_float4(0.f, 0.f, 0.f, 0.f);
}

hipError_t launch_reproj_delta(const float* xf_cur, const float* xf_hist, float4* delta, uint32_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(reproj_delta_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, xf_cur, xf_hist, delta, n);
    return hipGetLastError();
}

// MOTION (option svgf_motion): the pixel's world point and geometric normal are carried to where that surface point
// was in the history frame by its submesh's delta entry before anything else looks at them, and a tap counts only if the history
// frame saw the same submesh there.  MODE = Off is the kernel as it was: `m` is not read and the code is the same.
// MODE = Vertex (option svgf_vertex_motion) on top of Submesh: the pixel's entry of NEB_PLANE_PREV_POINT is read in the
// same round trip as its id; where its .w is not the sentinel it IS the previous point and geometric normal and the delta entry is not
// read, where it is the sentinel the Submesh rule applies unchanged.  Everything behind P and Ng is shared by the three arms.
// The three ...Demod modes (option svgf_demodulate on top of each arm): as temporal_pixel's DEMOD -- the albedo word
// (m.demod_albedo) is loaded with the pixel's own planes (the same first round trip), Cc is demodulated before anything reads it, and
// a.rad_hist is the demod plane for all four taps.  The first three modes are the kernels as they were: m.demod_albedo is not read.
enum class ReprojMode { Off, Submesh, Vertex, OffDemod, SubmeshDemod, VertexDemod };
template <ReprojMode MODE>
__global__ __launch_bounds__(256) void svgf_temporal_reproject_kernel(ReprojArgs a, ReprojMotion m)
{
    constexpr bool DEMOD = MODE == ReprojMode::OffDemod || MODE == ReprojMode::SubmeshDemod || MODE == ReprojMode::VertexDemod;
    constexpr bool VERTEX = MODE == ReprojMode::Vertex || MODE == ReprojMode::VertexDemod;
    constexpr bool MOTION = VERTEX || MODE == ReprojMode::Submesh || MODE == ReprojMode::SubmeshDemod;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= a.n_tiles)
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = (int)(tx * 8u + (lane & 7u)), y = (int)(ty * 8u + (lane >> 3));
    const size_t i = (size_t)y * a.W + (uint32_t)x;

    float4 Cc = a.rad_cur[i];
    const uint32_t dc = a.depth_cur[i];
    const uint2 nc = a.normal_cur[i];
    uint32_t g = kReprojNoSubmesh;
    if constexpr (MOTION)
        g = m.id_cur[i];
    float4 pv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (VERTEX)
        pv = m.prev_point[i];
    if constexpr (DEMOD)
        Cc = demodulate(Cc, m.demod_albedo[i]);
    const float zc = depth_unorm24(dc);

    float4 Ch = Cc; // (with no history: a = 0 and lerp(Cc, Cc, 0) = Cc exactly)
    float Mh0 = 0.0f, Mh1 = 0.0f;
    uint32_t n = 0;
    if (a.hist_ok && d24_surface(dc)) {
        float3 P = reproj_world_point(a.cc, a.inv_W, a.inv_H, x, y, zc);
        float3 Ng = oct16_unpack_zw(nc.x); // geometric normal (.xy)
        bool frozen = false; // MOTION: the submesh's transform cannot be inverted -- no history
        bool per_vertex = false; // VERTEX: the plane holds this pixel's previous point and normal
        if constexpr (VERTEX) {
            per_vertex = __float_as_uint(pv.w) != kReprojNoPrevPoint;
            if (per_vertex) {
                P = make_float3(pv.x, pv.y, pv.z);
                Ng = oct16_unpack_zw(__float_as_uint(pv.w));
            }
        }
        if constexpr (MOTION) {
            if (!per_vertex && g < m.n_delta) { // (no entry, no id: the point did not move -- P and Ng as they are)
                const float4* e = m.delta + (size_t)kReprojDeltaFloat4 * g;
                const uint32_t flag = __float_as_uint(e[0].x);
                frozen = flag == kReprojDeltaSingular;
                if (flag == kReprojDeltaMoved) { // the 96 bytes of D and K: only lanes on moved geometry (a tile on one object shares the lines)
                    const float4 d0 = e[1], d1 = e[2], d2 = e[3], k0 = e[4], k1 = e[5], k2 = e[6];
                    // P_h = (P, 1) . D, N_h = normalise(N . K): D = {d0.xyz | d0.w d1.xy | d1.zw d2.x | d2.yzw}, K = {k0.xyz | k0.w k1.xy | k1.zw k2.x}
                    const float hx = fmaf(P.z, d1.z, fmaf(P.y, d0.w, fmaf(P.x, d0.x, d2.y)));
                    const float hy = fmaf(P.z, d1.w, fmaf(P.y, d1.x, fmaf(P.x, d0.y, d2.z)));
                    const float hz = fmaf(P.z, d2.x, fmaf(P.y, d1.y, fmaf(P.x, d0.z, d2.w)));
                    const float nx = fmaf(Ng.z, k1.z, fmaf(Ng.y, k0.w, Ng.x * k0.x));
                    const float ny = fmaf(Ng.z, k1.w, fmaf(Ng.y, k1.x, Ng.x * k0.y));
                    const float nz = fmaf(Ng.z, k2.x, fmaf(Ng.y, k1.y, Ng.x * k0.z));
                    const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))); // (the correctly rounded one, as the divisions)
                    P = make_float3(hx, hy, hz);
                    Ng = make_float3(nx / len, ny / len, nz / len); // (len = 0: NaN, and no tap passes the normal test)
                }
            }
        }
        // project P with the history camera
        const float rx = P.x - a.ch.ex, ry = P.y - a.ch.ey, rz = P.z - a.ch.ez;
        const float zl = -fmaf(rz, a.ch.zz, fmaf(ry, a.ch.zy, rx * a.ch.zx)); // linear depth of P in the history camera
        const float cx = fmaf(rz, a.ch.xz, fmaf(ry, a.ch.xy, rx * a.ch.xx));
        const float cy = fmaf(rz, a.ch.yz, fmaf(ry, a.ch.yy, rx * a.ch.yx));
        const float ndc_x = cx / (zl * a.ch.sx), ndc_y = cy / (zl * a.ch.sy);
        const float fx = fmaf(ndc_x, a.half_W, a.half_W) - 0.5f; // continuous pixel position - 0.5: the taps are floor + {0, 1}
        const float fy = fmaf(-ndc_y, a.half_H, a.half_H) - 0.5f;
        if (!frozen && zl > 0.0f && fx > -1.0f && fx < (float)a.Wd && fy > -1.0f && fy < (float)a.Hd) { // (false for NaN too)
            const float x0f = floorf(fx), y0f = floorf(fy);
            const float wx = fx - x0f, wy = fy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;
            const float tol = kReprojPlaneTol * zl;
            // every tap's planes are loaded up front, at a clamped address (in bounds whatever the position), so that the wave has ONE
            // round trip to memory for the history instead of three dependent ones (tap depth -> tap normal -> tap radiance);
            // out-of-region taps are then simply not counted
            const int cx0 = min(max(x0, 0), a.Wd - 1), cx1 = min(max(x0 + 1, 0), a.Wd - 1);
            const int cy0 = min(max(y0, 0), a.Hd - 1), cy1 = min(max(y0 + 1, 0), a.Hd - 1);
            size_t j[4];
            j[0] = (size_t)cy0 * a.W + (uint32_t)cx0;
            j[1] = (size_t)cy0 * a.W + (uint32_t)cx1;
            j[2] = (size_t)cy1 * a.W + (uint32_t)cx0;
            j[3] = (size_t)cy1 * a.W + (uint32_t)cx1;
            const uint32_t* normal32 = reinterpret_cast<const uint32_t*>(a.normal_hist);
            uint32_t dt[4], nt[4], mh[4], hl[4], gt[4];
            float4 rt[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if constexpr (MOTION)
                    gt[t] = m.id_hist[j[t]];
                dt[t] = a.depth_hist[j[t]];
                nt[t] = normal32[2 * j[t]]; // .xy: geometric normal
                rt[t] = a.rad_hist[j[t]];
                mh[t] = a.mom_hist[j[t]];
                hl[t] = a.hlen_hist[j[t]];
            }
            float sw = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f, m0 = 0.0f, m1 = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int px = x0 + (t & 1), py = y0 + (t >> 1);
                if (px < 0 || px >= a.Wd || py < 0 || py >= a.Hd || !d24_surface(dt[t]))
                    continue;
                if constexpr (MOTION)
                    if (gt[t] != g) // the history frame saw another submesh there (every pixel, moved or not)
                        continue;
                const float3 Nt = oct16_unpack_zw(nt[t]);
                if (!(fmaf(Ng.z, Nt.z, fmaf(Ng.y, Nt.y, Ng.x * Nt.x)) >= kReprojNormalCos))
                    continue;
                const float3 Pt = reproj_world_point(a.ch, a.inv_W, a.inv_H, px, py, depth_unorm24(dt[t]));
                const float dist = fmaf(Pt.z - P.z, Ng.z, fmaf(Pt.y - P.y, Ng.y, (Pt.x - P.x) * Ng.x));
                if (!(fabsf(dist) <= tol))
                    continue;
                const float w = ((t & 1) ? wx : 1.0f - wx) * ((t >> 1) ? wy : 1.0f - wy);
                sw += w;
                ax = fmaf(w, rt[t].x, ax);
                ay = fmaf(w, rt[t].y, ay);
                az = fmaf(w, rt[t].z, az);
                m0 = fmaf(w, half_bits_to_float(mh[t] & 0xffffu), m0);
                m1 = fmaf(w, half_bits_to_float(mh[t] >> 16), m1);
                n = hl[t] > n ? hl[t] : n;
            }
            if (sw > 1e-4f) {
                const float inv = 1.0f / sw;
                Ch = make_float4(ax * inv, ay * inv, az * inv, Cc.w);
                Mh0 = m0 * inv;
                Mh1 = m1 * inv;
            } else {
                n = 0;
            }
        }
    }
    const float alpha = n == 0 ? 0.0f : fminf(a.alpha, 1.0f - 1.0f / (float)(n + 1u));
    if (a.geometry) {
        const float3 Ns = oct16_unpack_zw(nc.y);
        a.geometry[i] = make_float4(Ns.x, Ns.y, Ns.z, zc);
    }
    const uint2 mv = temporal_moments_f(Cc, Mh0, Mh1, alpha, a.varianceEps);
    a.rad_cur[i] = temporal_accumulate(Cc, Ch, alpha);
    a.mom_cur[i] = mv.x;
    a.variance[i] = (uint16_t)mv.y;
    a.hlen_cur[i] = (uint8_t)(n < 255u ? n + 1u : 255u);
}

static ReprojCam reproj_cam(const CameraBasis& b)
{
    ReprojCam c;
    c.ex = b.eye[0], c.ey = b.eye[1], c.ez = b.eye[2];
    c.xx = b.xaxis[0], c.xy = b.xaxis[1], c.xz = b.xaxis[2];
    c.yx = b.yaxis[0], c.yy = b.yaxis[1], c.yz = b.yaxis[2];
    c.zx = b.zaxis[0], c.zy = b.zaxis[1], c.zz = b.zaxis[2];
    c.sx = b.aspect * b.tan_half; // (gbuffer_kernel: ndc_x * aspect * tan_half, evaluated left to right)
    c.sy = b.tan_half;
    c.m22 = b.m22;
    c.m32 = b.m32;
    return c;
}

static hipError_t launch_reproject(const SvgfLaunch& L, const CameraBasis& cam_cur, const CameraBasis* cam_hist, float4* rad_cur,
                                   const float4* rad_hist, const uint32_t* depth_cur, const uint32_t* depth_hist, const uint2* normal_cur,
                                   const uint2* normal_hist, const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance,
                                   const uint8_t* hlen_hist, uint8_t* hlen_cur, float4* geometry, const ReprojMotion* motion, hipStream_t s,
                                   const uint32_t* demod_albedo)
{
    const uint32_t Wd = (L.W / 8u) * 8u, Hd = (L.H / 8u) * 8u; // the same-pixel pass's Dispatch(W/8, H/8) region
    if (Wd == 0 || Hd == 0)
        return hipSuccess;
    ReprojArgs a;
    a.rad_cur = rad_cur;
    a.rad_hist = rad_hist;
    a.depth_cur = depth_cur;
    a.depth_hist = depth_hist;
    a.normal_cur = normal_cur;
    a.normal_hist = normal_hist;
    a.mom_hist = mom_hist;
    a.mom_cur = mom_cur;
    a.variance = variance;
    a.hlen_hist = hlen_hist;
    a.hlen_cur = hlen_cur;
    a.geometry = geometry;
    a.W = L.W;
    a.tiles_x = Wd / 8u;
    a.n_tiles = a.tiles_x * (Hd / 8u);
    a.Wd = (int)Wd;
    a.Hd = (int)Hd;
    a.inv_W = 1.0f / (float)L.W;
    a.inv_H = 1.0f / (float)L.H;
    a.half_W = 0.5f * (float)L.W;
    a.half_H = 0.5f * (float)L.H;
    a.alpha = L.p.alpha;
    a.varianceEps = L.p.varianceEps;
    a.hist_ok = cam_hist != nullptr;
    a.cc = reproj_cam(cam_cur);
    a.ch = reproj_cam(cam_hist ? *cam_hist : cam_cur);
    const dim3 grid((a.n_tiles + 3u) / 4u);
    if (demod_albedo) {
        ReprojMotion mo = motion ? *motion : ReprojMotion{};
        mo.demod_albedo = demod_albedo;
        if (motion && motion->prev_point)
            hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::VertexDemod>, grid, dim3(256), 0, s, a, mo);
        else if (motion)
            hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::SubmeshDemod>, grid, dim3(256), 0, s, a, mo);
        else
            hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::OffDemod>, grid, dim3(256), 0, s, a, mo);
        return hipGetLastError();
    }
    if (motion && motion->prev_point)
        hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::Vertex>, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, s, a, *motion);
    else if (motion)
        hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::Submesh>, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, s, a, *motion);
    else
        hipLaunchKernelGGL(svgf_temporal_reproject_kernel<ReprojMode::Off>, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, s, a, ReprojMotion{});
    return hipGetLastError();
}

hipError_t launch_temporal_reproject(const SvgfLaunch& L, const CameraBasis& cam_cur, const CameraBasis* cam_hist, float4* rad_cur,
                                     const float4* rad_hist, const uint32_t* depth_cur, const uint32_t* depth_hist, const uint2* normal_cur,
                                     const uint2* normal_hist, const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance,
                                     const uint8_t* hlen_hist, uint8_t* hlen_cur, float4* geometry, hipStream_t s, const uint32_t* demod_albedo)
{
    return launch_reproject(L, cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, mom_cur, variance,
                            hlen_hist, hlen_cur, geometry, nullptr, s, demod_albedo);
}

hipError_t launch_temporal_reproject_motion(const SvgfLaunch& L, const CameraBasis& cam_cur, const CameraBasis* cam_hist, float4* rad_cur,
                                            const float4* rad_hist, const uint32_t* depth_cur, const uint32_t* depth_hist, const uint2* normal_cur,
                                            const uint2* normal_hist, const uint32_t* mom_hist, uint32_t* mom_cur, uint16_t* variance,
                                            const uint8_t* hlen_hist, uint8_t* hlen_cur, float4* geometry, const ReprojMotion& motion, hipStream_t s,
                                            const uint32_t* demod_albedo)
{
    return launch_reproject(L, cam_cur, cam_hist, rad_cur, rad_hist, depth_cur, depth_hist, normal_cur, normal_hist, mom_hist, mom_cur, variance,
                            hlen_hist, hlen_cur, geometry, &motion, s, demod_albedo);
}

// The same decode for rows the temporal pass did not cover (halo rows of a strip; ragged images; a level run on its own).
__global__ __launch_bounds__(256) void svgf_decode_geometry_kernel(const uint32_t* __restrict__ depth, const uint32_t* __restrict__ normal32,
                                                                   float4* __restrict__ geometry, size_t first, size_t n)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n)
        return;
    const size_t i = first + k;
    const float3 N = oct16_unpack_zw(normal32[2 * i + 1]); // .zw = shading normal
    geometry[i] = make_float4(N.x, N.y, N.z, depth_unorm24(depth[i]));
}

// ... of two row ranges in one launch (the halo rows above and below a strip's own: one launch where two tiny ones cost their latency twice)
__global__ __launch_bounds__(256) void svgf_decode_geometry2_kernel(const uint32_t* __restrict__ depth, const uint32_t* __restrict__ normal32,
                                                                    float4* __restrict__ geometry, size_t first_a, size_t n_a, size_t first_b, size_t n_b)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_a + n_b)
        return;
    const size_t i = k < n_a ? first_a + k : first_b + (k - n_a);
    const float3 N = oct16_unpack_zw(normal32[2 * i + 1]);
    geometry[i] = make_float4(N.x, N.y, N.z, depth_unorm24(depth[i]));
}

hipError_t launch_decode_geometry2(uint32_t W, uint32_t row_begin, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, const uint32_t* depth,
                                   const uint2* normal, float4* geometry, hipStream_t s)
{
    const size_t n_a = a0 < a1 ? (size_t)(a1 - a0) * W : 0, n_b = b0 < b1 ? (size_t)(b1 - b0) * W : 0;
    if (n_a + n_b == 0)
        return hipSuccess;
    hipLaunchKernelGGL(svgf_decode_geometry2_kernel, dim3((unsigned)((n_a + n_b + 255) / 256)), dim3(256), 0, s, depth,
                       reinterpret_cast<const uint32_t*>(normal), geometry, n_a ? (size_t)(a0 - row_begin) * W : 0, n_a,
                       n_b ? (size_t)(b0 - row_begin) * W : 0, n_b);
    return hipGetLastError();
}

hipError_t launch_decode_geometry(uint32_t W, uint32_t row_begin, uint32_t row0, uint32_t row1, const uint32_t* depth, const uint2* normal,
                                  float4* geometry, hipStream_t s)
{
    if (row0 >= row1)
        return hipSuccess;
    const size_t first = (size_t)(row0 - row_begin) * W, n = (size_t)(row1 - row0) * W;
    hipLaunchKernelGGL(svgf_decode_geometry_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, depth, reinterpret_cast<const uint32_t*>(normal),
                       geometry, first, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// A-trous: 5x5 taps at spacing `step`, edge-stopped by depth, normal and luminance.
// ------------------------------------------------------------------------------------------
struct AtrousArgs {
    const float4* src;
    float4* dst;
    const uint16_t* variance;
    const float4* geometry;     // {decoded shading normal.xyz, depth}: NEB_PLANE_GEOMETRY
    const float4* alpha_src;    // kInLum with OUT_ALPHA: the plane whose centre .w the output carries (the destination itself)
    int W, H, Wd;               // image size and floor-dispatched width
    int row_begin, row_end;     // resident image rows [row_begin, row_end)
    int row0, row1;             // image rows to write (row1 already clipped to (H/8)*8)
    int step;
    int tiles_x, tiles_j;       // LDS kernel: tiles per row segment / per residue class
    uint32_t nblocks;           // real block count (grid is padded to a multiple of 8)
    float cz;                   // log2e / (phiDepth * step)
    float phiColor, phiNormal;
    // kInFused only: the temporal pass's own planes (src = radiance[cur] as rendered) and constants.  The remodulating arms (kInClassicDemod and
    // the direct kernel's) never run fused and keep their two planes in members of it, so that the layout every other kernel reads stays as it is:
    // `albedo` = NEB_PLANE_ALBEDO, `demod_out` = NEB_PLANE_DEMOD.
    const float4* rad_hist;
    union {
        const uint32_t* depth_cur;
        const uint32_t* albedo;
    };
    const uint32_t* depth_hist;
    const uint2* normal_cur;
    const uint2* normal_hist;
    const uint32_t* mom_hist;
    uint32_t* mom_cur;
    uint16_t* variance_out;
    union {
        float4* geometry_out;
        float4* demod_out;
    };
    float t_neg_inv_two_sigma2_log2e, t_alpha, t_varianceEps;
};

// log2(K[abs(dx)] * K[abs(dy)]) with K = {1/16, 1/4, 3/8, 1/4, 1/16} indexed by abs(d): centre 1/16, +-1 -> 1/4, +-2 -> 3/8
// (svgf_atrous.hlsl:35,54,60 -- reproduced as written): the kernel weight is folded into the exponent
// of the edge-stopping exp2.
__host__ __device__ constexpr float atrous_log2k(int dx, int dy)
{
    // log2(1/16) = -4, log2(1/4) = -2, log2(3/8) = log2(3) - 3
    const float lx = (dx < 0 ? -dx : dx) == 0 ? -4.0f : ((dx < 0 ? -dx : dx) == 1 ? -2.0f : -1.4150374992788437f);
    const float ly = (dy < 0 ? -dy : dy) == 0 ? -4.0f : ((dy < 0 ? -dy : dy) == 1 ? -2.0f : -1.4150374992788437f);
    return lx + ly;
}

// max(0, dot(n0, n)) of svgf_atrous.hlsl:74 at no instruction: the centre normal arrives HALVED (exact), so the dot product is
// d / 2 and the free [0, 1] clamp of its last fma is max(0, d) / 2 for every d <= 2 -- normals decoded from RGBA16F are unit
// only to ~1e-3, d does exceed 1, and pow(d, 128) is then up to 1.14, which a clamp of d itself to [0, 1] would lose (rounds 1-2
// had that divergence; a bare max(x, 0) is a separate v_max per tap).  log2(d / 2) = log2(d) - 1: the tap's constant carries the
// + phiNormal that undoes it (`tap_constant`).
__device__ __forceinline__ float half_dot_max0(float dh) { return fminf(fmaxf(dh, 0.0f), 1.0f); }
__device__ __forceinline__ float tap_constant(float phiN, int dx, int dy) { return phiN + atrous_log2k(dx, dy); }

__device__ __forceinline__ float lum_scale(float var_f, float phiColor)
{
    const float varScale = phiColor * __fsqrt_rn(fmaxf(var_f, 1e-8f)); // :41
    return kLog2e * fast_rcp(fmaxf(varScale, 1e-6f));                  // :75 (as log2e / denom)
}

// One tap (svgf_atrous.hlsl:67-81): w = Kx*Ky * exp(-|dz|/(phiDepth*step)) * pow(max(0,d), phiNormal) * exp(-|dl|/denL) as ONE
// exp2: exponent = log2(Kx*Ky) + phiNormal*log2(d) - |dz|*cz - |dl|*cl   (d <= 0 -> -inf -> weight 0)
// h0 = the centre normal halved, lkp = tap_constant(phiN, dx, dy) = log2(Kx*Ky) + phiN.
__device__ __forceinline__ float tap_weight(float h0x, float h0y, float h0z, float z0, float lum0, float cl, float4 tA, float4 tB, float phiN, float cz,
                                            float lkp)
{
    const float dh = half_dot_max0(fmaf(h0z, tB.z, fmaf(h0y, tB.y, h0x * tB.x)));
    float e = fmaf(phiN, fast_log2(dh), lkp);
    e = fmaf(-fabsf(z0 - tB.w), cz, e);
    e = fmaf(-fabsf(lum0 - tA.w), cl, e);
    return fast_exp2(e);
}

// the same with MINUS the centre depth and luminance (what the packed form keeps in its register pairs): |t + (-z0)| = |z0 - t| exactly
__device__ __forceinline__ float tap_weight_neg(float h0x, float h0y, float h0z, float nz0, float nl0, float cl, float4 tA, float4 tB, float phiN, float cz,
                                                float lkp)
{
    const float dh = half_dot_max0(fmaf(h0z, tB.z, fmaf(h0y, tB.y, h0x * tB.x)));
    float e = fmaf(phiN, fast_log2(dh), lkp);
    e = fmaf(-fabsf(tB.w + nz0), cz, e);
    e = fmaf(-fabsf(tA.w + nl0), cl, e);
    return fast_exp2(e);
}

// ---- two output rows per instruction (round 4) ----
// A lane filters R = 2 output rows of one column, and four of the six staged rows it walks are taps of BOTH: the two taps share the
// texel and differ in the centre pixel only.  gfx950's packed fp32 forms do two IEEE operations per instruction at 2.09 ns per
// wave-instruction where a plain v_fma_f32 takes 1.24 and v_mul / v_add / v_sub 1.35-1.38 (tools/ubench_bank.hip): 16-25 % less issue
// time per operation, and every lane of a pair rounds exactly as the scalar instruction does -- `tap2_geometry` + `tap2_weight` are `tap_weight` twice,
// bit for bit (the direct kernel keeps the scalar form and agrees with the LDS kernel).
// The texel's component is broadcast to both halves by op_sel; what the compiler does not match by itself (a high-half broadcast
// in v_pk_add_f32, the free [0, 1] clamp on the packed fma) is written out.
typedef float neb_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ neb_f2 bc2(float s) { return (neb_f2){s, s}; }
__device__ __forceinline__ neb_f2 pk_fma(neb_f2 x, neb_f2 y, neb_f2 z) { return __builtin_elementwise_fma(x, y, z); }
// {p.y + q.x, p.y + q.y}
__device__ __forceinline__ neb_f2 pk_add_hi(neb_f2 p, neb_f2 q)
{
    neb_f2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(p), "v"(q));
    return r;
}
// clamp01({x.x * p.x + z.x, x.y * p.x + z.y})
__device__ __forceinline__ neb_f2 pk_fma_lo_clamp(neb_f2 x, neb_f2 p, neb_f2 z)
{
    neb_f2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] clamp" : "=v"(r) : "v"(x), "v"(p), "v"(z));
    return r;
}
// {c.x * l.x + k.a, c.x * l.y + k.b}: (a, b) = (x, y), or (y, x) when SWAP.  l comes out of v_log_f32, and a transcendental's result needs a wait
// state before an ordinary VALU instruction may read it: the compiler inserts one for its own instructions and cannot see into an `asm` (the
// first version of this function read the registers BEFORE the logarithm had landed), so the asm carries its own s_nop.  Why asm at all: c and
// k are loop-invariant, and written as vector code the broadcast {c.x, c.x} and the swapped {k.y, k.x} are hoisted out of the tile loop as
// fourteen more registers (two of the last-level kernels then spill) instead of being the op_sel bits of this one instruction.
template <bool SWAP>
__device__ __forceinline__ neb_f2 pk_fma_const(neb_f2 c, neb_f2 l, neb_f2 k)
{
    neb_f2 r;
    if constexpr (SWAP)
        asm("s_nop 0\n\tv_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(c), "v"(l), "v"(k));
    else
        asm("s_nop 0\n\tv_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(c), "v"(l), "v"(k));
    return r;
}
// The taps of one texel for the lane's two output rows, in three phases so that the caller can run each phase for all texels of a group before the next
// (a v_log / v_exp result needs a wait state before it is read, and the wave really waits: with a texel's phases back to back the level ran 1.1 us longer):
// h0* = the two centre normals halved, nz0 / nl0 = MINUS the centre depths / luminances (|t - z0| = |z0 - t| exactly), pc = {phiNormal, cz},
// lk = the two taps' constants in the order SWAP says.
struct Tap2 {
    neb_f2 l, dz, dl; // log2 of the halved, clamped dot products; depth and luminance differences (sign irrelevant)
};
__device__ __forceinline__ Tap2 tap2_geometry(neb_f2 h0x, neb_f2 h0y, neb_f2 h0z, neb_f2 nz0, neb_f2 nl0, float4 tA, float4 tB)
{
    const neb_f2 bxy = {tB.x, tB.y}, bzw = {tB.z, tB.w}, azw = {tA.z, tA.w};
    neb_f2 d = h0x * __builtin_shufflevector(bxy, bxy, 0, 0);
    d = pk_fma(h0y, __builtin_shufflevector(bxy, bxy, 1, 1), d);
    d = pk_fma_lo_clamp(h0z, bzw, d);
    Tap2 t;
    t.l = (neb_f2){fast_log2(d.x), fast_log2(d.y)};
    t.dz = pk_add_hi(bzw, nz0);
    t.dl = pk_add_hi(azw, nl0);
    return t;
}
template <bool SWAP, bool KS>
__device__ __forceinline__ neb_f2 tap2_weight(const Tap2& t, neb_f2 cl, neb_f2 pc, neb_f2 lk)
{
    neb_f2 e;
    if constexpr (KS) { // the constants are scalar operands (the fused kernel, at its register budget): two plain fmas, one SGPR source each
        e.x = fmaf(pc.x, t.l.x, SWAP ? lk.y : lk.x);
        e.y = fmaf(pc.x, t.l.y, SWAP ? lk.x : lk.y);
    } else {
        e = pk_fma_const<SWAP>(pc, t.l, lk);
    }
    e.x = fmaf(-fabsf(t.dz.x), pc.y, e.x);
    e.y = fmaf(-fabsf(t.dz.y), pc.y, e.y);
    e.x = fmaf(-fabsf(t.dl.x), cl.x, e.x);
    e.y = fmaf(-fabsf(t.dl.y), cl.y, e.y);
    return (neb_f2){fast_exp2(e.x), fast_exp2(e.y)};
}

// The a-trous output store, written through (sc1).  A plain store leaves its line dirty in the XCD's L2, and what is dirty when
// the kernel ends is written back before the next kernel starts (MI355X_MICROARCH.md, "boundary"); written through, the 33 MB
// of a level leave beside the arithmetic instead.
typedef float neb_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_output(float4* p, float4 v)
{
    const neb_f4 d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(d) : "memory");
}

// Direct kernel: one pixel per lane, 25 taps straight from global memory (L1/L2 absorb the reuse).
// Used for steps too wide for the LDS tile (>= 64) and as the in-library A/B arm (option atrous_variant = 0).
__global__ __launch_bounds__(256) void svgf_atrous_direct_kernel(AtrousArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = a.row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wd || y >= a.row1)
        return;
    const size_t i = (size_t)(y - a.row_begin) * a.W + x;
    const float4 c0 = a.src[i];
    const float lum0 = luminance(c0.x, c0.y, c0.z);
    const float cl = lum_scale(half_bits_to_float(a.variance[i]), a.phiColor);
    const float4 g0 = a.geometry[i];
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = min(max(y + dy * a.step, 0), a.H - 1); // :65 clamp to the image
        const size_t rowoff = (size_t)(qy - a.row_begin) * a.W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = min(max(x + dx * a.step, 0), a.W - 1);
            const float4 c = a.src[rowoff + qx];
            const float4 g = a.geometry[rowoff + qx];
            const float w = tap_weight(0.5f * g0.x, 0.5f * g0.y, 0.5f * g0.z, g0.w, lum0, cl, make_float4(c.x, c.y, c.z, luminance(c.x, c.y, c.z)), g,
                                       a.phiNormal, a.cz, tap_constant(a.phiNormal, dx, dy));
            sr = fmaf(w, c.x, sr);
            sg = fmaf(w, c.y, sg);
            sb = fmaf(w, c.z, sb);
            sw += w;
        }
    }
    const float inv = fast_rcp(fmaxf(sw, 1e-4f)); // :84
    a.dst[i] = make_float4(sr * inv, sg * inv, sb * inv, c0.w);
}

// The same as the chain's last level under option svgf_demodulate: the filtered colour goes unmodulated to a.demod_out and times the output
// pixel's divisor to a.dst; the albedo word is loaded with the centre texel.  A kernel of its own, the taps written out a second time: the
// kernel above called through a shared body comes out of the compiler with operands commuted, and it is pinned to stay as it was.
__global__ __launch_bounds__(256) void svgf_atrous_direct_demod_kernel(AtrousArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = a.row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wd || y >= a.row1)
        return;
    const size_t i = (size_t)(y - a.row_begin) * a.W + x;
    const float4 c0 = a.src[i];
    const uint32_t alb = a.albedo[i];
    const float lum0 = luminance(c0.x, c0.y, c0.z);
    const float cl = lum_scale(half_bits_to_float(a.variance[i]), a.phiColor);
    const float4 g0 = a.geometry[i];
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = min(max(y + dy * a.step, 0), a.H - 1);
        const size_t rowoff = (size_t)(qy - a.row_begin) * a.W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = min(max(x + dx * a.step, 0), a.W - 1);
            const float4 c = a.src[rowoff + qx];
            const float4 g = a.geometry[rowoff + qx];
            const float w = tap_weight(0.5f * g0.x, 0.5f * g0.y, 0.5f * g0.z, g0.w, lum0, cl, make_float4(c.x, c.y, c.z, luminance(c.x, c.y, c.z)), g,
                                       a.phiNormal, a.cz, tap_constant(a.phiNormal, dx, dy));
            sr = fmaf(w, c.x, sr);
            sg = fmaf(w, c.y, sg);
            sb = fmaf(w, c.z, sb);
            sw += w;
        }
    }
    const float inv = fast_rcp(fmaxf(sw, 1e-4f));
    const float3 d = demod_divisor(alb);
    const float r = sr * inv, g = sg * inv, b = sb * inv;
    a.demod_out[i] = make_float4(r, g, b, c0.w);
    a.dst[i] = make_float4(r * d.x, g * d.y, b * d.z, c0.w);
}

// LDS kernel: row-lattice tiles, persistent workgroups.
//   Workgroup = 256 lanes = 4 waves.  Output tile = BW (64) columns x BH (= 4R)
//   rows of the lattice {r + S*j}.  Taps of a lattice row are lattice rows j-2..j+2, so the
//   tile needs only BH+4 image rows for any step S; its columns are consecutive up to S = 8 (BW + 4 S staged) and a lattice of
//   8-pixel groups beyond (BW + 32 staged at any step, AtrousTile below): read amplification (1 + 4/BH)(1 + 32/BW) instead
//   of (1 + 4S/T)^2.
//   Two float4 LDS planes, lane-contiguous (ds_read_b128, conflict-free): A = {r, g, b, lum} and B = {nx, ny, nz, z}
//   (= the texels of the frame's decoded geometry plane).  Wave w filters lattice rows [w*R, w*R+R): a lane walks its
//   column's R+4 staged rows once and feeds each staged texel to every output row it is a tap of.
//
//   How a tile's texels reach LDS -- template parameter IN:
//   kInClassic  the source plane holds {r, g, b, alpha} (any radiance plane of the ABI).  The radiance of the NEXT tile is
//               loaded into registers while the current tile is filtered (its latency hides under ~1.6k VALU
//               instructions per wave); staging adds the luminance and writes A; B comes by LDS-DMA
//               (global_load_lds_dwordx4: per-lane source address, destination = wave-uniform base + lane * 16 B = exactly
//               the staging order; no registers, no VALU).
//   kInLum      the source plane holds {r, g, b, lum}: an intermediate plane of a whole-frame denoise, written by the level
//               before with OUT_ALPHA = false.  Both planes are verbatim copies: two LDS-DMAs per staged texel, no staging
//               arithmetic and no staging registers at all.
//   kInFused    level 0 of a whole-frame denoise (S = 1): src = radiance[cur] as rendered.  Staging IS the temporal pass
//               (svgf_temporal.hlsl:24-68): cur / history radiance arrive by LDS-DMA in the slots of A / B, depth and normals of
//               both frames in registers; every staged texel (halo included) is accumulated and decoded in place; the
//               tile's own pixels also write moments, variance and the decoded geometry plane -- and the accumulated
//               radiance is never written to memory (the filtered output is the next frame's history).
//   OUT_ALPHA: the output's .w is the centre pixel's alpha (the ABI's radiance planes) -- false: lum(output), for a
//   following kInLum level.  The alpha comes from src (kInClassic), from alpha_src = the destination itself (kInLum: the
//   last level writes radiance[cur], which still holds the frame's input) or from the fused staging (kInFused).
//   kInClassicDemod  kInClassic as the chain's last level under option svgf_demodulate (OUT_ALPHA = true): the output pixel's albedo word is
//               fetched one tile ahead with its variance; the filtered colour goes unmodulated to demod_out and times the pixel's divisor
//               (svgf_demod.h) to dst.  Staging, taps and schedule are kInClassic's.
enum : int { kInClassic = 0, kInLum = 1, kInFused = 2, kInClassicDemod = 3 };

// The columns of a tile.  Up to S = 8 a tile's 64 output columns are consecutive and it stages 64 + 4 S of them.  Beyond, that halo
// doubles and triples the tile (128 staged columns per 64 outputs at S = 16), so the columns form a lattice too, in GROUPS of
// XS = 8 pixels (128 bytes of a plane = one L2 line: every load and store instruction still touches whole lines): local column c is
// pixel x0 + xcol(c) = x0 + (c / XS - 2) S + c % XS.  A tap at +-S, +-2 S is then one or two groups = XS or 2 XS local columns away
// for every lane, the halo is 4 XS = 32 columns at any step (S = 16: 96 staged columns instead of 128, four workgroups per CU instead
// of three), and S / XS tiles whose x0 differ by XS interleave over the same span of (64 / XS) S pixels.  For S <= XS this is the
// plain layout.  Measured inside the frame (same box): S = 16 33.2 us against 34.9; with groups of 4 pixels (64 bytes, 80 staged
// columns) 35.6 -- an LDS-DMA instruction then touches sixteen half lines instead of eight whole ones.
template <int S, int IN>
struct AtrousTile {
    // R = 2 rows per lane at every step, level 0 with the temporal pass included: 8-row tiles of 68 - 96 staged columns (26 - 37 KB)
    // fit four workgroups per CU at 128 registers per lane, and the fused kernel's staging then holds four texels per lane, not six,
    // which is what lets it fit 128 registers at all.  Two rows are also what the packed tap arithmetic pairs (tap2_geometry).
    static constexpr int R = 2;
    static constexpr int THREADS = 256;
    static constexpr int XS = S < NEB_ATROUS_XGROUP ? S : NEB_ATROUS_XGROUP; // pixels per column group = the tap stride in local columns
    static constexpr int XM = S / XS;                                        // interleaved tiles per span
    static constexpr int BW = 64, SPAN = (BW / XS) * S;                      // output columns of a tile (one per lane), and the pixels they span
    static constexpr int BH = 4 * R, COLS = BW + 4 * XS, ROWS = BH + 4, TOTAL = ROWS * COLS;
    static_assert(S % XS == 0 && 64 % XS == 0, "column groups tile both the step and the wave");
    // pixel column (relative to the tile's x0) of local column c
    __host__ __device__ static constexpr int xcol(int c) { return (c / XS - 2) * S + c % XS; }
    static constexpr int NLOAD = (TOTAL + THREADS - 1) / THREADS;
    // kInFused keeps {variance, alpha} of the tile's own pixels in a third, small plane
    static constexpr int LDS_BYTES = TOTAL * 2 * 16 + (IN == kInFused ? BH * BW * 8 : 0);
    // workgroups per CU: what the 160 KB of LDS hold, at most NEB_ATROUS_PER_CU_R2 (4: 128 registers per lane) -- also the register budget the kernel is
    // compiled for
    static constexpr int PER_CU = NEB_ATROUS_PER_CU_R2 < (160 * 1024) / LDS_BYTES ? NEB_ATROUS_PER_CU_R2 : (160 * 1024) / LDS_BYTES;
    static constexpr int WAVES_PER_SIMD = PER_CU < 8 ? PER_CU : 8; // launch bound: k blocks of 256 threads per CU <=> k waves per SIMD
};

template <int S, int IN, bool OUT_ALPHA>
__global__ __launch_bounds__(256, (AtrousTile<S, IN>::WAVES_PER_SIMD)) void svgf_atrous_lds_kernel(AtrousArgs a)
{
    using T = AtrousTile<S, IN>;
    constexpr int R = T::R, BW = T::BW, BH = T::BH, COLS = T::COLS, ROWS = T::ROWS, TOTAL = T::TOTAL, NLOAD = T::NLOAD, THREADS = T::THREADS;
    constexpr int XS = T::XS, XM = T::XM, SPAN = T::SPAN;
    static_assert(IN != kInFused || S == 1, "the fused temporal staging is level 0");
    static_assert(IN != kInClassicDemod || OUT_ALPHA, "the remodulating level writes the chain's result");
    constexpr bool kClassic = IN == kInClassic || IN == kInClassicDemod, kDemod = IN == kInClassicDemod;
    extern __shared__ float4 lds[];
    float4* __restrict__ A = lds;               // {r, g, b, lum}
    float4* __restrict__ B = lds + ROWS * COLS; // {nx, ny, nz, z}
    float2* __restrict__ V = reinterpret_cast<float2*>(lds + 2 * ROWS * COLS); // kInFused: {variance as stored (fp16), alpha} [BH][BW]

    const float4* __restrict__ src = a.src;
    const float4* __restrict__ geometry = a.geometry;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (wave-uniform: row bases and row addresses become scalar)
    // the wave's row group (R lattice rows) and 64-column block of the tile.  A tile is one wave wide, so cb is always 0 and rg = wv, but the
    // compiler cannot see wv < 4 through readfirstlane: written without cb, every LDS kernel is scheduled differently.
    const int rg = wv & 3, cb = wv >> 2;

    // Tile walk, XCD-aware: workgroups b, b+8, ... share an XCD (and its L2); each XCD takes a contiguous
    // run of tiles, and the workgroups of an XCD interleave inside that run.  Speed only.
    // (Handing the tiles out dynamically instead -- one ticket counter per XCD, tickets requested a tile ahead -- was
    // measured at 46 us per level against 35: a device-scope atomic is a round trip to the memory side of the fabric, and
    // the static split is already balanced where it matters, per CU: 8 tiles on all but 8 CUs against 7.97 on average.)
    const uint32_t per_xcd = (a.nblocks + 7u) >> 3;
    const uint32_t xcd = blockIdx.x & 7u, wg_in_xcd = blockIdx.x >> 3, wgs_per_xcd = gridDim.x >> 3;
    const uint32_t t_end = min((xcd + 1u) * per_xcd, a.nblocks);

    // Byte offsets of this lane's staged texels from the element Tile::first.  A tile whose staged rectangle lies inside
    // the image (and the resident rows) -- nine in ten -- needs no clamping: the offsets are the same for every such tile
    // and its loads are "uniform tile base + offset" (scalar base, 32-bit vector offset: no address arithmetic on the VALU
    // at all).  An edge tile overwrites them with its clamped positions (the reference's edge rule), counted from the
    // plane's first element; the next interior tile puts the regular ones back.
    uint32_t toff[NLOAD];
    bool toff_regular = false;
    float4 pc[kClassic ? NLOAD : 1];

    struct Tile {
        int r, jbase, x0;
        size_t first; // element index the offsets in toff[] count from
    };
    auto tile_origin = [&](uint32_t t, Tile& o) -> bool {
        // Tile order inside an XCD's run.  The levels: along the lattice fastest, then columns, then residues -- the tiles that share
        // staged rows (j and j + 1 of one column and residue: 4 of a tile's 12 rows) and columns (neighbouring column tiles) are in
        // flight on the same XCD at the same time and its L2 serves the second reader (S = 16: 30.6 us against 32.7; 8: 28.0 / 28.8;
        // 4: 27.9 / 28.7).  Level 0 with the temporal pass, bound by memory, keeps columns fastest: narrow vertical runs cost it
        // 53.2 us against 50.8 with 16-row tiles, 50.1 against 47.6 with 8-row ones (short row segments of many rows: the DRAM pages).  Blocks of 2 / 4 / 8 tiles along the lattice with
        // the columns in between lose at the wide steps (the padded tile count unbalances the XCDs).
        int tx_tile, jt;
        if constexpr (IN == kInFused) {
            tx_tile = (int)(t % (uint32_t)a.tiles_x);
            const int rest = (int)(t / (uint32_t)a.tiles_x);
            o.r = rest % S; // residue class of the lattice rows
            jt = rest / S;  // tile index along the lattice
        } else {
            jt = (int)(t % (uint32_t)a.tiles_j);
            const int rest = (int)(t / (uint32_t)a.tiles_j);
            tx_tile = rest % a.tiles_x;
            o.r = rest / a.tiles_x;
        }
        const int jmin = (a.row0 - o.r + S - 1) / S > 0 ? (a.row0 - o.r + S - 1) / S : 0; // first lattice index inside [row0,row1)
        o.jbase = jmin + jt * BH;
        o.x0 = (tx_tile / XM) * SPAN + (tx_tile % XM) * XS;
        return o.r + S * o.jbase < a.row1; // false: whole tile below the row range
    };
    // fills toff[] / o.first for a tile about to be loaded
    auto tile_offsets = [&](Tile& o) {
        const int y_first = o.r + S * (o.jbase - 2), y_last = o.r + S * (o.jbase + ROWS - 3), x_first = o.x0 + T::xcol(0);
        const bool interior = y_first >= max(0, a.row_begin) && y_last < min(a.H, a.row_end) && x_first >= 0 && o.x0 + T::xcol(COLS - 1) < a.W;
        if (interior) {
            o.first = (size_t)(y_first - a.row_begin) * a.W + x_first;
            if (!toff_regular) {
                // (the lane index made opaque: computed from threadIdx.x these loop-invariant offsets are hoisted out of the tile
                // loop and held in NLOAD more registers for the whole kernel -- which the fused kernel does not have)
                int tid = threadIdx.x;
                asm volatile("" : "+v"(tid));
#pragma unroll
                for (int k = 0; k < NLOAD; ++k) {
                    const int i = tid + THREADS * k;
                    const int lr = i / COLS;
                    toff[k] = (uint32_t)(lr * S * a.W + (T::xcol(i - lr * COLS) - T::xcol(0))) * 16u;
                }
                toff_regular = true;
            }
        } else {
            o.first = 0;
            toff_regular = false;
            int tid = threadIdx.x; // (opaque for the same reason: lr and lc of every k would be held for the whole kernel)
            asm volatile("" : "+v"(tid));
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const int i = tid + THREADS * k;
                const int lr = i / COLS, lc = i - lr * COLS;
                // clamp to the image (svgf_atrous.hlsl:65), then to the resident rows: a partial tile also stages rows
                // that no valid output taps; on a row strip those may lie outside the allocation, so they are
                // redirected to a resident row (their values are never used)
                int y = min(max(o.r + S * (o.jbase + lr - 2), 0), a.H - 1);
                y = min(max(y, a.row_begin), a.row_end - 1);
                const int x = min(max(o.x0 + T::xcol(lc), 0), a.W - 1);
                toff[k] = (uint32_t)((y - a.row_begin) * a.W + x) * 16u; // (a plane is < 4 GB: checked at launch)
            }
        }
    };
    // kInClassic: the next tile's radiance, into registers
    auto issue_load = [&](int k, const Tile& o) {
        if constexpr (kClassic) {
            if (threadIdx.x + THREADS * k < TOTAL)
                pc[k] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(src + o.first) + toff[k]);
        }
    };
    // a 16-byte plane's texels of the tile, global -> LDS directly.  Issued once the whole workgroup has finished reading
    // the previous tile, and complete before the barrier that precedes the filter.
    auto issue_dma = [&](const float4* plane, float4* dst_lds, const Tile& o) {
#pragma unroll
        for (int k = 0; k < NLOAD; ++k) {
            if (threadIdx.x + THREADS * k < TOTAL) {
                const char* g = reinterpret_cast<const char*>(plane + o.first) + toff[k];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                 (__attribute__((address_space(3))) void*)(dst_lds + THREADS * k + 64 * wv), 16, 0, 0);
            }
        }
    };

    // The centre pixel's variance and alpha (the per-pixel inputs that are not staged) are fetched one tile ahead as
    // well: loaded at the start of the filter phase they were a dependent global round trip in front of every tile's
    // arithmetic (2.5 us per level).  (kInFused has both in LDS.)
    uint32_t nvar[R], nalb[kDemod ? R : 1];
    float nalpha[R];
    auto issue_centre_loads = [&](const Tile& o) {
        if constexpr (IN != kInFused) {
            const int xo = o.x0 + T::xcol(cb * 64 + lane + 2 * XS);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int yo = o.r + S * (o.jbase + rg * R + k);
                nvar[k] = 0u;
                nalpha[k] = 0.f;
                if (xo < a.Wd && yo < a.row1) {
                    const size_t i = (size_t)(yo - a.row_begin) * a.W + xo;
                    nvar[k] = a.variance[i];
                    if constexpr (OUT_ALPHA)
                        nalpha[k] = reinterpret_cast<const float*>(kClassic ? src : a.alpha_src)[4 * i + 3];
                    if constexpr (kDemod)
                        nalb[k] = a.albedo[i];
                }
            }
        }
    };

    // (Re-measured in round 3 with the co-residency known -- blocks b, b + 256, b + 512 share a CU: the 2nd / 3rd workgroup asking for
    // its first tile 1 / 2 us later than the first changes nothing measurable, 183-189 us per frame against 186.)
    uint32_t t = xcd * per_xcd + wg_in_xcd;
    Tile nt{0, 0, 0, 0};
    bool have = false;
    while (t < t_end && !(have = tile_origin(t, nt)))
        t += wgs_per_xcd;
    if (have) {
        tile_offsets(nt);
#pragma unroll
        for (int k = 0; k < NLOAD; ++k)
            issue_load(k, nt);
        issue_centre_loads(nt);
    }

    // per-launch constants of the tap arithmetic as VGPR operands (in isolation an SGPR source costs a v_fma about 0.6 ns more
    // than a third VGPR source does, tools/ubench_bank.hip: 1.83 against 1.25 ns per wave-instruction at three waves per SIMD;
    // in this kernel the difference does not show: 192.5 against 192.0 us per frame)
    float cz = a.cz, phiN = a.phiNormal;
    // log2(Kx Ky) + phiN of the six tap classes (|dx|, |dy| in {0, 1, 2}), set up once: computed per tap it would be an add each.
    // The levels of the fused chain (kInLum) hold them in vector registers.  The fused kernel and the kernels that prefetch the next
    // tile's radiance into registers run at their register budget (with the constants in registers the fused kernel spilled, and a
    // kernel that needs scratch memory right after the GI kernels, which use theirs at another size, waits for the queue's scratch
    // set-up): there they are scalar operands, and a texel's taps are evaluated one texel at a time (kLkScalar).
    constexpr bool kLkScalar = IN != kInLum;
    float lkp[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            lkp[i][j] = tap_constant(phiN, i, j);
            if constexpr (kLkScalar)
                lkp[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lkp[i][j])));
            else
                asm volatile("" : "+v"(lkp[i][j]));
            lkp[j][i] = lkp[i][j];
        }
    if constexpr (!kLkScalar)
        asm volatile("" : "+v"(cz), "+v"(phiN));
    // the packed tap's constants: {phiNormal, cz}, and per |dx| the pairs {lkp[.][0], lkp[.][1]} and {lkp[.][1], lkp[.][2]} (read straight
    // or swapped by op_sel)
    neb_f2 pcz = {phiN, cz}, lkq[3][2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        lkq[i][0] = (neb_f2){lkp[i][0], lkp[i][1]};
        lkq[i][1] = (neb_f2){lkp[i][1], lkp[i][2]};
        if constexpr (!kLkScalar)
            asm volatile("" : "+v"(lkq[i][0]), "+v"(lkq[i][1]));
    }
    if constexpr (!kLkScalar)
        asm volatile("" : "+v"(pcz));

    while (have) {
        // The SIMD's arbiter serves its oldest wave first: of the three workgroups of a CU the first-dispatched one races
        // ahead and the youngest is left to finish alone, one wave per SIMD, at half the issue rate.  Priority = tiles still
        // to do lets the workgroups finish together.
        {
            const uint32_t remaining = (t_end - t + wgs_per_xcd - 1u) / wgs_per_xcd; // (this tile included)
            // (four levels: with 8-row tiles a workgroup has four tiles or more, and a separate level for them finishes the
            // workgroups closer together than "three and more" as one)
            if (remaining >= 4u)
                __builtin_amdgcn_s_setprio(3);
            else if (remaining == 3u)
                __builtin_amdgcn_s_setprio(2);
            else if (remaining == 2u)
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
        const int cr = nt.r, cjbase = nt.jbase, cx0 = nt.x0;
        // ---- stage the tile ----
        if constexpr (kClassic) {
            issue_dma(geometry, B, nt); // first: its flight overlaps the wait for the prefetched radiance and the luminance arithmetic
            float lum[NLOAD];
#pragma unroll
            for (int k = 0; k < NLOAD; ++k)
                lum[k] = luminance(pc[k].x, pc[k].y, pc[k].z);
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const int i = threadIdx.x + THREADS * k;
                if (i < TOTAL)
                    A[i] = make_float4(pc[k].x, pc[k].y, pc[k].z, lum[k]);
            }
        } else if constexpr (IN == kInLum) {
            issue_dma(src, A, nt);
            issue_dma(geometry, B, nt);
        } else {
            // temporal accumulation as the staging step: cur -> A's slots, history -> B's slots by DMA; depth and normals of
            // both frames (and the moments history of the tile's own pixels) through registers; then every thread turns ITS
            // texels (the ones its own wave's DMA wrote: no barrier needed, only the wave's own vmcnt) into {accumulated
            // rgb, lum} and {decoded normal, depth} in place.
            issue_dma(src, A, nt);
            issue_dma(a.rad_hist, B, nt);
            uint32_t dc[NLOAD], dh[NLOAD], nc[NLOAD], nh[NLOAD], mh[NLOAD];
            bool own[NLOAD];
            size_t gi[NLOAD];
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const int i = threadIdx.x + THREADS * k;
                own[k] = false;
                if (i < TOTAL) {
                    const size_t e = nt.first + (toff[k] >> 4);
                    gi[k] = e;
                    dc[k] = a.depth_cur[e];
                    dh[k] = a.depth_hist[e];
                    nc[k] = a.normal_cur[e].y; // .zw = shading normal
                    nh[k] = a.normal_hist[e].y;
                    const int lr = i / COLS, lc = i - lr * COLS;
                    const int x = cx0 + T::xcol(lc), y = cr + S * (cjbase + lr - 2);
                    // one of the tile's own output pixels (never a clamped position: those lie outside the image)
                    own[k] = lr >= 2 && lr < BH + 2 && lc >= 2 * XS && lc < BW + 2 * XS && x < a.Wd && y >= a.row0 && y < a.row1;
                    mh[k] = own[k] ? a.mom_hist[e] : 0u;
                }
            }
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const int i = threadIdx.x + THREADS * k;
                if (i < TOTAL) {
                    const float4 Cc = A[i], Ch = B[i];
                    float3 Nc;
                    float zc;
                    const float alpha = temporal_blend(dc[k], dh[k], nc[k], nh[k], a.t_neg_inv_two_sigma2_log2e, a.t_alpha, Nc, zc);
                    const float4 acc = temporal_accumulate(Cc, Ch, alpha);
                    const float4 geo = make_float4(Nc.x, Nc.y, Nc.z, zc);
                    A[i] = make_float4(acc.x, acc.y, acc.z, luminance(acc.x, acc.y, acc.z));
                    B[i] = geo;
                    if (own[k]) {
                        const uint2 mv = temporal_moments(Cc, mh[k], alpha, a.t_varianceEps);
                        a.mom_cur[gi[k]] = mv.x;
                        a.variance_out[gi[k]] = (uint16_t)mv.y;
                        a.geometry_out[gi[k]] = geo;
                        const int lr = i / COLS, lc = i - lr * COLS;
                        V[(lr - 2) * BW + (lc - 2 * XS)] = make_float2(half_bits_to_float(mv.y), Cc.w); // (the variance as the levels read it back)
                    }
                }
            }
        }
        __syncthreads(); // (also waits for this wave's DMA: an LDS-DMA is a pending LDS write on the VM counter)

        // ---- next tile: issue its loads now, consume them after this tile is filtered ----
        uint32_t cvar[R], calb[kDemod ? R : 1];
        float calpha[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            cvar[k] = nvar[k], calpha[k] = nalpha[k];
            if constexpr (kDemod)
                calb[k] = nalb[k];
        }
        bool have_next = false;
        t += wgs_per_xcd;
        while (t < t_end && !(have_next = tile_origin(t, nt)))
            t += wgs_per_xcd;
        if (have_next) {
            tile_offsets(nt); // (the current tile's DMA has been issued: toff[] is free)
            issue_centre_loads(nt);
        }
        // The next tile's loads are spread over the row iterations of the filter below (one batch per row) so
        // that, chip-wide, memory traffic and arithmetic overlap instead of alternating in bursts; batches
        // beyond the R+4 row iterations go out first.
        if (have_next) {
#pragma unroll
            for (int k = R + 4; k < NLOAD; ++k)
                issue_load(k, nt);
        }

        // ---- filter the current tile ----
        const int xo = cx0 + T::xcol(cb * 64 + lane + 2 * XS);
        float z0[R], n0x[R], n0y[R], n0z[R], lum0[R], cl[R], alpha0[R];
        float sr[R], sg[R], sb[R], sw[R];
        bool valid[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int lr = rg * R + k + 2;
            const float4 cA = A[lr * COLS + cb * 64 + lane + 2 * XS];
            const float4 cB = B[lr * COLS + cb * 64 + lane + 2 * XS];
            z0[k] = cB.w;
            n0x[k] = 0.5f * cB.x; // halved: see half_dot_max0
            n0y[k] = 0.5f * cB.y;
            n0z[k] = 0.5f * cB.z;
            lum0[k] = cA.w;
            const int yo = cr + S * (cjbase + rg * R + k);
            valid[k] = (xo < a.Wd) && (yo < a.row1);
            if constexpr (IN == kInFused) {
                const float2 va = V[(rg * R + k) * BW + lane]; // (a pixel that is not valid holds stale values: never stored)
                alpha0[k] = va.y;
                cl[k] = lum_scale(va.x, a.phiColor);
            } else {
                alpha0[k] = calpha[k];
                cl[k] = lum_scale(half_bits_to_float((uint16_t)cvar[k]), a.phiColor); // (an invalid pixel holds 0: never stored)
            }
            sr[k] = sg[k] = sb[k] = sw[k] = 0.f;
        }
        // LDS reads software-pipelined by hand: a row's ten ds_read_b128 go out in two groups (dx = -2..0, dx = 1..2), each
        // one group ahead of its taps, into the registers the group before last has just released -- left to itself the
        // compiler (at its register budget) issues each read right in front of its use and every wave pays the LDS round
        // trip five times per row.
        float4 gA[2][3], gB[2][3];
        auto load_group = [&](int g) {
            const int ir = g >> 1, lrow_base = (rg * R + ir) * COLS + cb * 64 + lane + 2 * XS;
            if ((g & 1) == 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gA[0][j] = A[lrow_base + (j - 2) * XS];
                    gB[0][j] = B[lrow_base + (j - 2) * XS];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    gA[1][j] = A[lrow_base + (j + 1) * XS];
                    gB[1][j] = B[lrow_base + (j + 1) * XS];
                }
            }
        };
        // The lane's output rows side by side in PAIRS (see tap2_geometry): pair p = rows 2 p, 2 p + 1; staged row ir is row lir = ir - 2 p of the
        // pair's own six, tap dy = lir - 2 of its first row and lir - 3 of its second.  (R = 2 makes it one pair; written without the pair loop,
        // the fused chain's kernels are scheduled differently.)
        constexpr int NP = R / 2;
        neb_f2 h0x[NP], h0y[NP], h0z[NP], nz0[NP], nl0[NP], cl2[NP], sr2[NP], sg2[NP], sb2[NP], sw2[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            h0x[p] = (neb_f2){n0x[2 * p], n0x[2 * p + 1]}, h0y[p] = (neb_f2){n0y[2 * p], n0y[2 * p + 1]}, h0z[p] = (neb_f2){n0z[2 * p], n0z[2 * p + 1]};
            nz0[p] = (neb_f2){-z0[2 * p], -z0[2 * p + 1]}, nl0[p] = (neb_f2){-lum0[2 * p], -lum0[2 * p + 1]}, cl2[p] = (neb_f2){cl[2 * p], cl[2 * p + 1]};
            sr2[p] = sg2[p] = sb2[p] = sw2[p] = (neb_f2){0.f, 0.f};
        }
        load_group(0);
#pragma unroll
        for (int g = 0; g < 2 * (R + 4); ++g) {
            const int ir = g >> 1;
            if ((g & 1) == 0 && ir < NLOAD && have_next)
                issue_load(ir, nt);
            if (g + 1 < 2 * (R + 4))
                load_group(g + 1);
            __builtin_amdgcn_sched_barrier(0);
            constexpr int kMaxGroup = 3;
            const int ng = (g & 1) ? 2 : 3; // texels of this group: dx = -2, -1, 0 or 1, 2
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int lir = ir - 2 * p;
                if (lir == 0 || lir == 5) { // taps of one row only (dy = -2 of the pair's first row, dy = +2 of its second)
                    const int k = lir == 0 ? 0 : 1;
#pragma unroll
                    for (int j = 0; j < ng; ++j) {
                        const int dx = (g & 1) ? j + 1 : j - 2, adx = dx < 0 ? -dx : dx;
                        const float4 tA = gA[g & 1][j];
                        const float4 tB = gB[g & 1][j];
                        const float w = tap_weight_neg(h0x[p][k], h0y[p][k], h0z[p][k], nz0[p][k], nl0[p][k], cl2[p][k], tA, tB, pcz.x, pcz.y, lkq[adx][1].y);
                        sr2[p][k] = fmaf(w, tA.x, sr2[p][k]);
                        sg2[p][k] = fmaf(w, tA.y, sg2[p][k]);
                        sb2[p][k] = fmaf(w, tA.z, sb2[p][k]);
                        sw2[p][k] += w;
                    }
                } else if constexpr (kLkScalar) {
                    // one texel at a time (the fused kernel's staging phase leaves no registers for a whole group's intermediate values)
#pragma unroll
                    for (int j = 0; j < ng; ++j) {
                        const int dx = (g & 1) ? j + 1 : j - 2, adx = dx < 0 ? -dx : dx;
                        const float4 tA = gA[g & 1][j];
                        const Tap2 t = tap2_geometry(h0x[p], h0y[p], h0z[p], nz0[p], nl0[p], tA, gB[g & 1][j]);
                        const neb_f2 w = (lir == 1)   ? tap2_weight<false, true>(t, cl2[p], pcz, lkq[adx][1])
                                         : (lir == 2) ? tap2_weight<false, true>(t, cl2[p], pcz, lkq[adx][0])
                                         : (lir == 3) ? tap2_weight<true, true>(t, cl2[p], pcz, lkq[adx][0])
                                                      : tap2_weight<true, true>(t, cl2[p], pcz, lkq[adx][1]);
                        const neb_f2 axy = {tA.x, tA.y}, azw = {tA.z, tA.w};
                        sr2[p] = pk_fma(w, __builtin_shufflevector(axy, axy, 0, 0), sr2[p]);
                        sg2[p] = pk_fma(w, __builtin_shufflevector(axy, axy, 1, 1), sg2[p]);
                        sb2[p] = pk_fma(w, __builtin_shufflevector(azw, azw, 0, 0), sb2[p]);
                        sw2[p] += w;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    // the whole group phase by phase: geometry, weights, sums (see tap2_geometry)
                    Tap2 t[kMaxGroup];
                    neb_f2 w[kMaxGroup];
#pragma unroll
                    for (int j = 0; j < ng; ++j)
                        t[j] = tap2_geometry(h0x[p], h0y[p], h0z[p], nz0[p], nl0[p], gA[g & 1][j], gB[g & 1][j]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < ng; ++j) {
                        const int dx = (g & 1) ? j + 1 : j - 2, adx = dx < 0 ? -dx : dx;
                        // (|dy0|, |dy1|) = (1, 2), (0, 1), (1, 0), (2, 1) for lir = 1 .. 4: the constant pairs {0, 1} and {1, 2}, straight or swapped
                        w[j] = (lir == 1)   ? tap2_weight<false, false>(t[j], cl2[p], pcz, lkq[adx][1])
                               : (lir == 2) ? tap2_weight<false, false>(t[j], cl2[p], pcz, lkq[adx][0])
                               : (lir == 3) ? tap2_weight<true, false>(t[j], cl2[p], pcz, lkq[adx][0])
                                            : tap2_weight<true, false>(t[j], cl2[p], pcz, lkq[adx][1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < ng; ++j) {
                        const float4 tA = gA[g & 1][j];
                        const neb_f2 axy = {tA.x, tA.y}, azw = {tA.z, tA.w};
                        sr2[p] = pk_fma(w[j], __builtin_shufflevector(axy, axy, 0, 0), sr2[p]);
                        sg2[p] = pk_fma(w[j], __builtin_shufflevector(axy, axy, 1, 1), sg2[p]);
                        sb2[p] = pk_fma(w[j], __builtin_shufflevector(azw, azw, 0, 0), sb2[p]);
                        sw2[p] += w[j];
                    }
                }
                // Pin the partial sums here: they only feed the predicated store below, so LLVM would otherwise sink ALL the arithmetic
                // under that branch and keep every staged texel live (spilling ~1.3 KB per lane).  The sched_barrier keeps one group's
                // ds_reads per region.
                asm volatile("" : "+v"(sr2[p]), "+v"(sg2[p]), "+v"(sb2[p]), "+v"(sw2[p]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            sr[k] = sr2[k >> 1][k & 1];
            sg[k] = sg2[k >> 1][k & 1];
            sb[k] = sb2[k >> 1][k & 1];
            sw[k] = sw2[k >> 1][k & 1];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (!valid[k])
                continue;
            const int yo = cr + S * (cjbase + rg * R + k);
            const float inv = fast_rcp(fmaxf(sw[k], 1e-4f)); // :84
            const float r = sr[k] * inv, g = sg[k] * inv, b = sb[k] * inv;
            if constexpr (kDemod) {
                const float3 d = demod_divisor(calb[k]);
                const size_t o = (size_t)(yo - a.row_begin) * a.W + xo;
                store_output(a.demod_out + o, make_float4(r, g, b, alpha0[k]));
                store_output(a.dst + o, make_float4(r * d.x, g * d.y, b * d.z, alpha0[k]));
                continue;
            }
            store_output(a.dst + ((size_t)(yo - a.row_begin) * a.W + xo), make_float4(r, g, b, OUT_ALPHA ? alpha0[k] : luminance(r, g, b)));
        }
        have = have_next;
        if (have)
            __syncthreads(); // everyone is done reading LDS before the next tile overwrites it
    }
}

// (Measured and dropped: a double-buffered LDS variant that weaves the staging of tile i+1 into the row loop of
// tile i, one barrier per tile -- 45-94 us per level against 41-49 us for the kernel above; the longer live
// ranges cost more than the barrier and the exposed decode they remove.  Round 3: the geometry texels prefetched into
// registers like the radiance instead of the DMA at the tile boundary: 45 us per level against 35.)
template <int S, int IN, bool OUT_ALPHA>
static hipError_t launch_lds(AtrousArgs a, int device, int num_cus, hipStream_t s)
{
    using T = AtrousTile<S, IN>;
    constexpr size_t lds_bytes = (size_t)T::LDS_BYTES;
    // the dynamic-LDS limit is a per-device function attribute: remember which devices have it (one bit each; a
    // device ordinal beyond the mask just sets it on every launch)
    static std::atomic<uint64_t> attr_set{0};
    const uint64_t bit = (device >= 0 && device < 64) ? (1ull << device) : 0ull;
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&svgf_atrous_lds_kernel<S, IN, OUT_ALPHA>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess)
            return e;
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    a.tiles_x = ((a.Wd + T::SPAN - 1) / T::SPAN) * T::XM;
    const int max_lattice_rows = (a.row1 - a.row0 + S - 1) / S; // per residue class, upper bound
    a.tiles_j = (max_lattice_rows + T::BH - 1) / T::BH;
    a.nblocks = (uint32_t)a.tiles_x * (uint32_t)S * (uint32_t)a.tiles_j;
    // persistent grid: as many workgroups as fit (LDS-limited, at most 3 per CU by the launch bounds)
    static_assert(T::PER_CU >= 1, "tile too large for the LDS");
    const uint32_t per_cu = (uint32_t)T::PER_CU;
    uint32_t grid = (uint32_t)num_cus * (per_cu ? per_cu : 1u);
    if (grid > a.nblocks)
        grid = a.nblocks;
    grid = ((grid + 7u) / 8u) * 8u;
    hipLaunchKernelGGL((svgf_atrous_lds_kernel<S, IN, OUT_ALPHA>), dim3(grid), dim3(T::THREADS), lds_bytes, s, a);
    return hipGetLastError();
}

template <int IN, bool OUT_ALPHA>
static hipError_t launch_lds_step(const AtrousArgs& a, uint32_t step, int device, int num_cus, hipStream_t s)
{
    switch (step) {
    case 1: return launch_lds<1, IN, OUT_ALPHA>(a, device, num_cus, s);
    case 2: return launch_lds<2, IN, OUT_ALPHA>(a, device, num_cus, s);
    case 4: return launch_lds<4, IN, OUT_ALPHA>(a, device, num_cus, s);
    case 8: return launch_lds<8, IN, OUT_ALPHA>(a, device, num_cus, s);
    case 16: return launch_lds<16, IN, OUT_ALPHA>(a, device, num_cus, s);
    case 32: return launch_lds<32, IN, OUT_ALPHA>(a, device, num_cus, s);
    default: return hipErrorInvalidValue;
    }
}

bool atrous_lds_serves(const SvgfLaunch& L, int variant, uint32_t step)
{
    // wider steps do not fit the LDS tile; the LDS kernel addresses a plane with 32-bit byte offsets: a resident plane of
    // 4 GB or more -- 16 k x 16 k -- takes the direct kernel
    return variant >= 1 && step <= 32u && (step & (step - 1u)) == 0u && (uint64_t)(L.row_end - L.row_begin) * L.W < (1ull << 28);
}

static bool atrous_args(const SvgfLaunch& L, uint32_t step, const float4* src, float4* dst, const uint16_t* variance, const float4* geometry,
                        AtrousArgs& a)
{
    const uint32_t Wd = (L.W / 8u) * 8u, Hd = (L.H / 8u) * 8u; // SVGFDenoiser.cpp:185
    const uint32_t row1 = L.row1 < Hd ? L.row1 : Hd;
    if (L.row0 >= row1 || Wd == 0)
        return false;
    a = AtrousArgs{};
    a.src = src;
    a.dst = dst;
    a.variance = variance;
    a.geometry = geometry;
    a.W = (int)L.W;
    a.H = (int)L.H;
    a.Wd = (int)Wd;
    a.row_begin = (int)L.row_begin;
    a.row_end = (int)L.row_end;
    a.row0 = (int)L.row0;
    a.row1 = (int)row1;
    a.step = (int)step;
    a.cz = kLog2e / (L.p.phiDepth * (float)step);
    a.phiColor = L.p.phiColor;
    a.phiNormal = L.p.phiNormal;
    return true;
}

hipError_t launch_atrous(const SvgfLaunch& L, int variant, uint32_t step, const float4* src, float4* dst,
                         const uint16_t* variance, const float4* geometry, hipStream_t s)
{
    AtrousArgs a;
    if (!atrous_args(L, step, src, dst, variance, geometry, a))
        return hipSuccess;
    if (atrous_lds_serves(L, variant, step))
        return launch_lds_step<kInClassic, true>(a, step, L.device, L.num_cus > 0 ? L.num_cus : 256, s);
    dim3 grid((a.Wd + 63) / 64, (a.row1 - a.row0 + 3) / 4);
    hipLaunchKernelGGL(svgf_atrous_direct_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_atrous_remodulate(const SvgfLaunch& L, int variant, uint32_t step, const float4* src, float4* dst, const uint16_t* variance,
                                    const float4* geometry, const uint32_t* albedo, float4* demod_out, hipStream_t s)
{
    AtrousArgs a;
    if (!atrous_args(L, step, src, dst, variance, geometry, a))
        return hipSuccess;
    a.albedo = albedo;
    a.demod_out = demod_out;
    if (atrous_lds_serves(L, variant, step))
        return launch_lds_step<kInClassicDemod, true>(a, step, L.device, L.num_cus > 0 ? L.num_cus : 256, s);
    dim3 grid((a.Wd + 63) / 64, (a.row1 - a.row0 + 3) / 4);
    hipLaunchKernelGGL(svgf_atrous_direct_demod_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_atrous_lum(const SvgfLaunch& L, uint32_t step, bool last, const float4* src, float4* dst, const uint16_t* variance,
                             const float4* geometry, hipStream_t s)
{
    AtrousArgs a;
    if (!atrous_args(L, step, src, dst, variance, geometry, a))
        return hipSuccess;
    a.alpha_src = dst; // the last level writes the plane that still holds the frame's input: its alpha is carried
    const int num_cus = L.num_cus > 0 ? L.num_cus : 256;
    // (the last level's alpha read from its destination -- 4 of every 16 bytes -- is hidden under the arithmetic: 35.9 us with it,
    // 35.6 without)
    return last ? launch_lds_step<kInLum, true>(a, step, L.device, num_cus, s) : launch_lds_step<kInLum, false>(a, step, L.device, num_cus, s);
}

hipError_t launch_atrous_fused_temporal(const SvgfLaunch& L, bool only_level, const float4* rad_cur, const float4* rad_hist, const uint32_t* depth_cur,
                                        const uint32_t* depth_hist, const uint2* normal_cur, const uint2* normal_hist, const uint32_t* mom_hist,
                                        uint32_t* mom_cur, uint16_t* variance, float4* geometry, float4* dst, hipStream_t s)
{
    AtrousArgs a;
    if (!atrous_args(L, 1u, rad_cur, dst, variance, geometry, a))
        return hipSuccess;
    a.rad_hist = rad_hist;
    a.depth_cur = depth_cur;
    a.depth_hist = depth_hist;
    a.normal_cur = normal_cur;
    a.normal_hist = normal_hist;
    a.mom_hist = mom_hist;
    a.mom_cur = mom_cur;
    a.variance_out = variance;
    a.geometry_out = geometry;
    a.t_neg_inv_two_sigma2_log2e = -kLog2e / (2.0f * L.p.depthSigma * L.p.depthSigma);
    a.t_alpha = L.p.alpha;
    a.t_varianceEps = L.p.varianceEps;
    const int num_cus = L.num_cus > 0 ? L.num_cus : 256;
    return only_level ? launch_lds<1, kInFused, true>(a, L.device, num_cus, s) : launch_lds<1, kInFused, false>(a, L.device, num_cus, s);
}

} // namespace neb
