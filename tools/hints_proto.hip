// tools/hints_proto.hip -- pack_hints / unpack_hints of nebulae_amd/csrc/gi_internal.h as host functions, for
// tests/test_sun_audit_cpu.py: the numpy decoding of the shading records (tests/sun_audit_ref.py) is held to them field for field.
// Build: hipcc -O1 -std=c++17 --offload-arch=gfx950 -shared -fPIC -I nebulae_amd/csrc -I include tools/hints_proto.hip -o liblit_hints.so
// (host code only is called; no device is touched)
#include "gi_internal.h"

extern "C" {

uint32_t hints_no_hint() { return neb::kNoHint; }
uint32_t hints_count() { return (uint32_t)neb::kHints; }
uint32_t hints_lit_shift() { return neb::kLitShift; }
uint32_t hints_geom_mask() { return neb::kGeomMask; }

// words = r7.yzw of a shading record
void hints_pack(const uint32_t* hint, uint32_t side, uint32_t* words)
{
    float4 r7 = {0.f, 0.f, 0.f, 0.f};
    neb::pack_hints(hint, side, r7);
    memcpy(words, &r7.y, 12);
}

void hints_unpack(const uint32_t* words, uint32_t* hint, uint32_t* side)
{
    float4 r7 = {0.f, 0.f, 0.f, 0.f};
    memcpy(&r7.y, words, 12);
    neb::unpack_hints(r7, hint, *side);
}

} // extern "C"
