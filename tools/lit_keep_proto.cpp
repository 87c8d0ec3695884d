// tools/lit_keep_proto.cpp -- CPU checker of a sun table KEPT across a scene update: lit::box_may_shadow (nebulae_amd/csrc/lit_predicate.h)
// applied the way a device pass over the shading records would apply it -- the lit bits of the updated submeshes go, and the lit bit of
// every other side whose shadow rays can reach into an updated submesh's new world box.  (The library itself still drops the table on every
// update: DESIGN.md 3.3a.)
// Build (with tools/lit_proto.cpp, which makes the flags): g++ -O2 -fopenmp -shared -fPIC -I nebulae_amd/csrc tools/lit_proto.cpp tools/lit_keep_proto.cpp
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lit_predicate.h"

using namespace neb::lit;

// verts / normals: the scene AFTER the update, 9 floats per triangle (an unmoved triangle is where it was when `flags` were made);
// built_abs_max: the largest |coordinate| of the scene the flags were built for (their Frame and margin); moved[i] != 0: triangle i belongs
// to an updated submesh; boxes: n_boxes x {lo xyz, hi xyz}, the new world boxes of the updated submeshes.
// Returns 1 (and clears every flag) when a box would make the certificate's margin grow -- bits proven with a smaller slack are no proofs
// under a larger one --, else 0.
// stats (may be null): {sides lit before, sides cleared because their triangle moved, sides cleared by a box, sides still lit}.
extern "C" int lit_keep_apply(int n, const float* verts, const float* normals, const float* sun_dir, float tan_half, double built_abs_max, unsigned char* flags,
                              int n_boxes, const float* boxes, const unsigned char* moved, double* stats)
{
    Frame F;
    make_frame(sun_dir, tan_half, built_abs_max, F);
    const double pad = std::max(1e-5, 1.1920928955078125e-7 * built_abs_max);
    std::vector<SunBox> B(n_boxes);
    bool grew = false;
    for (int k = 0; k < n_boxes; ++k) {
        double abs_max = 0.0;
        for (int q = 0; q < 6; ++q)
            abs_max = std::max(abs_max, std::fabs((double)boxes[6 * k + q]));
        grew = grew || !(margin_for(abs_max) <= F.margin);
        make_sun_box(F, boxes + 6 * k, boxes + 6 * k + 3, pad, B[k]);
    }
    double before = 0, own = 0, boxed = 0, after = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : before, own, boxed, after)
    for (int i = 0; i < n; ++i) {
        const unsigned f = flags[i];
        if (!f)
            continue;
        before += (f & 1u) + (f >> 1 & 1u);
        unsigned clear = 0;
        if (grew || moved[i]) {
            clear = 3u;
            own += (f & 1u) + (f >> 1 & 1u);
        } else {
            double v[3][3], g[3][3];
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c)
                    v[k][c] = verts[9 * i + 3 * k + c], g[k][c] = normals[9 * i + 3 * k + c];
            for (int side = 0; side < 2; ++side) {
                if (!(f >> side & 1u))
                    continue;
                Receiver R;
                make_receiver(F, v, g, side == 0 ? +1 : -1, R);
                bool may = !R.valid;
                for (int k = 0; k < n_boxes && !may; ++k)
                    may = box_may_shadow(F, R, B[k]);
                if (may) {
                    clear |= 1u << side;
                    boxed += 1;
                }
            }
        }
        flags[i] = (unsigned char)(f & ~clear);
        after += (flags[i] & 1u) + (flags[i] >> 1 & 1u);
    }
    if (stats)
        stats[0] = before, stats[1] = own, stats[2] = boxed, stats[3] = after;
    return grew ? 1 : 0;
}
