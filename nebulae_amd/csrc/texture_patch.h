// texture_patch.h -- the arithmetic of a texel update in place (neb_gi_update_textures, gi_material.hip).
//
// The device holds no images, only bilinear-footprint tables (gi_build.hip): entry (ex, ey) of a w x h texture keeps the four texels
// {(ex,ey), (ex+1,ey), (ex,ey+1), (ex+1,ey+1)}, wrap applied -- slots 00, 10, 01, 11.  A texel (tx, ty) therefore lives in FOUR entries:
// (tx, ty) slot 00, (tx-1, ty) slot 10, (tx, ty-1) slot 01, (tx-1, ty-1) slot 11, all mod (w, h).  Replacing the rectangle
// [x, x+rw) x [y, y+rh) touches the rectangle of entries grown by one column to the left and one row upwards, with wrap, capped at
// w x h positions so that a full-width or full-height rectangle visits no entry twice.  This header answers, for one such entry, which
// of its four slots take a new texel and from where in the source rectangle; and it holds the bit layout of a material bundle's
// 32-byte entry as material_bundle_kernel packs it, per role.
//
// Plain C++ (no HIP types) so that the CPU prototype (tools/texture_patch_proto.cpp) compiles the very same code.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define NEB_TP_HD __host__ __device__ inline
#else
#define NEB_TP_HD inline
#endif

namespace neb {
namespace texpatch {

// which of a material's three maps a texture is (a texture may be more than one of them): bits of a role mask
constexpr uint32_t kRoleAlbedo = 1u, kRoleNormal = 2u, kRoleRoughMetal = 4u;

// One texel of a bundle entry is the pair {lo, hi}:
//   lo = albedo.r | albedo.g << 8 | albedo.b << 16 | normal.r << 24,  hi = normal.g | normal.b << 8 | rm.g << 16 | rm.b << 24
// (alpha and rm.r are not kept).  The bits of {lo, hi} that belong to the roles in `roles`:
NEB_TP_HD uint32_t role_mask_lo(uint32_t roles) { return ((roles & kRoleAlbedo) ? 0x00ffffffu : 0u) | ((roles & kRoleNormal) ? 0xff000000u : 0u); }
NEB_TP_HD uint32_t role_mask_hi(uint32_t roles) { return ((roles & kRoleNormal) ? 0x0000ffffu : 0u) | ((roles & kRoleRoughMetal) ? 0xffff0000u : 0u); }
// ... and the RGBA8 texel t placed on them (t = r | g << 8 | b << 16 | a << 24)
NEB_TP_HD uint32_t role_bits_lo(uint32_t t, uint32_t roles) { return ((t & 0x00ffffffu) | (t << 24)) & role_mask_lo(roles); }
NEB_TP_HD uint32_t role_bits_hi(uint32_t t, uint32_t roles)
{
    const uint32_t gb = (t >> 8) & 0xffffu;
    return (gb | (gb << 16)) & role_mask_hi(roles);
}

struct Patch {
    uint32_t w, h;   // the texture
    uint32_t x, y;   // the rectangle's first texel: x < w, y < h
    uint32_t rw, rh; // its size: 1 <= rw <= w - x, 1 <= rh <= h - y (inside the texture, no wrap)
};

// the affected entries: cols x rows positions, numbered (i, j) with i along x
NEB_TP_HD uint32_t patch_cols(const Patch& p) { return p.rw + 1u < p.w ? p.rw + 1u : p.w; }
NEB_TP_HD uint32_t patch_rows(const Patch& p) { return p.rh + 1u < p.h ? p.rh + 1u : p.h; }
// entry (i, j) of them: the column left of the rectangle first, the row above it first, both with wrap
NEB_TP_HD void patch_entry(const Patch& p, uint32_t i, uint32_t j, uint32_t& ex, uint32_t& ey)
{
    const uint32_t cx = p.x ? p.x - 1u : p.w - 1u, cy = p.y ? p.y - 1u : p.h - 1u;
    ex = cx + i < p.w ? cx + i : cx + i - p.w; // (i < cols <= w and cx < w: one subtraction is the wrap, and the sum cannot overflow
    ey = cy + j < p.h ? cy + j : cy + j - p.h; //  since set_scene keeps w * h below 2^32)
}
// Slot s (bit 0: x + 1, bit 1: y + 1) of entry (ex, ey): does its texel lie in the rectangle?  Then (sx, sy) is that texel's place
// in the source rectangle, row sy, column sx.
NEB_TP_HD bool patch_slot(const Patch& p, uint32_t ex, uint32_t ey, uint32_t s, uint32_t& sx, uint32_t& sy)
{
    uint32_t tx = ex + (s & 1u), ty = ey + (s >> 1);
    tx = tx >= p.w ? tx - p.w : tx;
    ty = ty >= p.h ? ty - p.h : ty;
    if (tx < p.x || tx - p.x >= p.rw || ty < p.y || ty - p.y >= p.rh)
        return false;
    sx = tx - p.x;
    sy = ty - p.y;
    return true;
}

// One entry of a STANDALONE table (4 words: the texels of slots 00, 10, 01, 11) patched from the source rectangle (rows of RGBA8 at
// pitch_bytes, a multiple of 4).  false: no slot of this entry is in the rectangle (cannot happen for an affected entry).
NEB_TP_HD bool patch_table_entry(const Patch& p, uint32_t ex, uint32_t ey, const uint8_t* src, uint32_t pitch_bytes, uint32_t e[4])
{
    bool any = false;
    for (uint32_t s = 0; s < 4u; ++s) {
        uint32_t sx, sy;
        if (patch_slot(p, ex, ey, s, sx, sy)) {
            e[s] = *reinterpret_cast<const uint32_t*>(src + (size_t)sy * pitch_bytes + 4u * (size_t)sx);
            any = true;
        }
    }
    return any;
}
// One entry of a BUNDLE (8 words: {lo, hi} of slots 00, 10, 01, 11), only the bits of `roles`.
NEB_TP_HD bool patch_bundle_entry(const Patch& p, uint32_t ex, uint32_t ey, const uint8_t* src, uint32_t pitch_bytes, uint32_t roles, uint32_t e[8])
{
    bool any = false;
    const uint32_t mlo = role_mask_lo(roles), mhi = role_mask_hi(roles);
    for (uint32_t s = 0; s < 4u; ++s) {
        uint32_t sx, sy;
        if (patch_slot(p, ex, ey, s, sx, sy)) {
            const uint32_t t = *reinterpret_cast<const uint32_t*>(src + (size_t)sy * pitch_bytes + 4u * (size_t)sx);
            e[2u * s] = (e[2u * s] & ~mlo) | role_bits_lo(t, roles);
            e[2u * s + 1u] = (e[2u * s + 1u] & ~mhi) | role_bits_hi(t, roles);
            any = true;
        }
    }
    return any;
}

} // namespace texpatch
} // namespace neb
