// svgf_demod.h -- the one constant and the one written-down order of albedo demodulation (option "svgf_demodulate", see the block next to
// neb_svgf_set_camera in include/nebulae_hip.h).  The only place the floor is defined: tests/demod_ref.py reads it from here.
//   d_c        = fmaxf(albedo_c, kDemodFloor)   per channel, albedo = the R11G11B10_FLOAT word of NEB_PLANE_ALBEDO decoded
//   demodulate   c / d_c                        (the correctly rounded IEEE division)
//   remodulate   c * d_c                        (one plain product)
#pragma once

namespace neb {

// A power of two, so that a black or sky pixel (albedo 0) round-trips exactly: (x * 32) * (1 / 32) == x.  About the dielectric F0 of 0.04:
// a surface darker than that returns mostly specular light, which its albedo does not scale.
constexpr float kDemodFloor = 0.03125f;

#if defined(__HIPCC__)
// The divisor of one pixel.  An unsigned 6e5 / 5e5 small float is the top 11 / 10 bits of a positive fp16, so the decode is a shift and
// v_cvt_f32_f16 (denormals, infinity and NaN included): the same values as unpack_r11g11b10 of gi_device.h, at three conversions.
// A NaN field takes the floor (fmaxf returns the other operand).
__device__ __forceinline__ float3 demod_divisor(uint32_t albedo_word)
{
    const float r = (float)__builtin_bit_cast(_Float16, (unsigned short)((albedo_word & 0x7ffu) << 4));
    const float g = (float)__builtin_bit_cast(_Float16, (unsigned short)(((albedo_word >> 11) & 0x7ffu) << 4));
    const float b = (float)__builtin_bit_cast(_Float16, (unsigned short)((albedo_word >> 22) << 5));
    return make_float3(fmaxf(r, kDemodFloor), fmaxf(g, kDemodFloor), fmaxf(b, kDemodFloor));
}

// rgb divided by the pixel's divisor, alpha as it is
__device__ __forceinline__ float4 demodulate(float4 c, uint32_t albedo_word)
{
    const float3 d = demod_divisor(albedo_word);
    return make_float4(c.x / d.x, c.y / d.y, c.z / d.z, c.w);
}
#endif

} // namespace neb
