// path_segments.h -- the segment loop of a path query, included as text by its two kernels in gi_query.hip:
// ray_path_kernel (neb_gi_trace_paths) and probe_bake_kernel (neb_gi_bake_probes, 3.8c).  One text, so that a probe's sample follows the
// path neb_gi_trace_paths follows for the same ray bit for bit; text and not a function, because as an inlined function the loop gives
// ray_path_kernel's VERTICES instantiations other register figures than 3.8b's table (3.8c).  No include guard: it is included twice.
// Reads: S, heads, sun, L, Bv, T (the sun frame), last (segments a path can have), stack, i (the index that seeds the stream), the template
// parameters FAST and VERTICES, vrec (VERTICES).  Takes over o, dir, tmin, tmax (the first segment).  Leaves: sum, first_t,
// first_geometry, first_primitive, path_flags, segments.
// TAIL (0: none of it is compiled): the path's last possible vertex, where no further segment is sampled, ends in the
// probe grid `tail` (TailArgs) instead.  The loop only leaves behind what that vertex knows -- tail_live, its point (tail_p, tail_n), the
// weight tail_k, its direct term tail_added, its flags and pdiff (tail_flags, tail_pd), and `sum` WITHOUT that vertex -- and the gather
// runs after the loop, where the loop-carried state is dead and every lane of the wave arrives together (gather_wave ballots).
    bool alive = ray_walkable(o, dir, tmin, tmax);
    uint32_t rng = jenkins(i ^ jenkins(sun.frame_index));
    float3 throughput = f3(1.0f, 1.0f, 1.0f), sum = f3(0.0f, 0.0f, 0.0f);
    float first_t = __builtin_inff();
    uint32_t first_geometry = kNoId, first_primitive = kNoId, path_flags = alive ? 0u : (uint32_t)NEB_HIT_NOT_WALKED, segments = 0u;
    uint32_t k = 1u;
    [[maybe_unused]] bool tail_live = false;
    [[maybe_unused]] float3 tail_p = f3(0.0f, 0.0f, 0.0f), tail_n = tail_p, tail_k = tail_p, tail_added = tail_p;
    [[maybe_unused]] float tail_pd = 0.0f;
    [[maybe_unused]] uint32_t tail_flags = 0u;
    for (; k <= last; ++k) {
        if (__ballot(alive) == 0ull)
            break;
        Hit h;
        const bool found = traverse(S, o, alive ? dir : f3(0.0f, 0.0f, 0.0f), tmin, tmax, false, stack, h);
        // (a later segment the traverser refuses -- a direction that is not finite -- is a miss, as it is one in the frame)
        uint32_t flags = alive && k > 1u && !ray_walkable(o, dir, tmin, tmax) ? (uint32_t)NEB_HIT_NOT_WALKED : 0u;
        float t = __builtin_inff(), bu = 0.0f, bv = 0.0f;
        uint32_t geometry = kNoId, primitive = kNoId;
        float3 hitP = f3(0.0f, 0.0f, 0.0f);
        Surface surf;
        surf.GN = surf.SN = surf.albedo = f3(0.0f, 0.0f, 0.0f);
        surf.roughness = surf.metalness = 0.0f;
        if (found) { // (ray_shade_kernel's reconstruction, its flags)
            const float4 ids = S.tris[3 * h.tri + 2]; // {e2.z, geometry, primitive, -}
            const TriShade ts = load_tri_shade(S, h.tri);
            const ShadeHead head = load_shade_header(heads, ts.geom);
            float tex_u = 0.0f, tex_v = 0.0f;
            t = h.t, bu = h.u, bv = h.v;
            geometry = __float_as_uint(ids.y), primitive = __float_as_uint(ids.z);
            hitP = o + dir * h.t;
            flags |= NEB_HIT_FOUND;
            const bool has_material = reconstruct_geometry<FAST>(head, ts, h.u, h.v, surf, tex_u, tex_v);
            if (head.valid)
                flags |= NEB_HIT_ATTRIBUTES | (dot3(surf.GN, dir) > 0.0f ? (uint32_t)NEB_HIT_BACKFACE : 0u);
            if (has_material) {
                MapSamples maps;
                sample_material_maps<FAST>(S, head.mat, tex_u, tex_v, maps);
                reconstruct_material<FAST>(head.mat, ts, h.u, h.v, maps, surf);
                flags |= NEB_HIT_MATERIAL;
            }
        }
        const bool shaded = (flags & NEB_HIT_MATERIAL) != 0;
        // shade_pixel's shadow ray, its exact-arithmetic sequence under both policies; the two disk draws advance the path's stream
        // where there is a surface to shade
        const uint32_t rng_in = rng;
        const float3 throughput_in = throughput;
        uint32_t rng_disk = rng;
        const float a0 = rand01(rng_disk), a1 = rand01(rng_disk);
        const float angle = a0 * 2.0f * 3.1415926535f, dist = fsqrt<false>(a1);
        float sn_a, cs_a;
        det_sincosf(angle, sn_a, cs_a);
        const float3 inc = normalize3<false>(L + (Bv * sn_a + T * cs_a) * sun.tan_half * dist);
        const bool transition = dot3(surf.GN, inc) <= 0.0f;
        const float3 so = hitP + (transition ? -surf.GN : surf.GN) * 1e-2f;
        Hit sh;
        const bool occluded = traverse(S, so, shaded ? inc : f3(0.0f, 0.0f, 0.0f), 0.001f, kTraceMax, true, stack, sh);
        float3 added = f3(0.0f, 0.0f, 0.0f);
        const float3 V = normalize3<FAST>(-dir); // :522
        if (alive && !found) { // :508
            added = f3(sun.sky[0], sun.sky[1], sun.sky[2]) * throughput;
            path_flags |= NEB_PATH_ESCAPED;
        }
        if (shaded) {
            rng = rng_disk;
            if (!occluded) {
                added = evaluate_direct_brdf<FAST>(surf, V, L) * f3(sun.radiance[0], sun.radiance[1], sun.radiance[2]) * throughput; // :573-574
                flags |= NEB_HIT_SUN_VISIBLE;
            }
        }
        const bool ends_in_grid = TAIL != 0 && shaded && k == last; // (its `added` enters the sum after the loop, with the tail)
        if (alive) {
            if (!ends_in_grid)
                sum = k == 1u ? added : sum + added;
            ++segments;
        }
        if (k == 1u) {
            first_t = t, first_geometry = geometry, first_primitive = primitive;
            path_flags |= flags;
        }
        float4 seg_o = make_float4(o.x, o.y, o.z, tmin), seg_d = make_float4(dir.x, dir.y, dir.z, t);
        const float seg_tmax = tmax;
        float pdiff = 0.0f;
        const bool bounce = shaded && k < last; // (:579-583; `shaded` implies `alive`)
        if (bounce) {
            // EvaluateIndirectBRDF (:230-259) takes rng BY VALUE: the Rand(rng) of :614 returns the same number as the first of its draws
            uint32_t rng_copy = rng;
            const float3 SNn = normalize3<FAST>(surf.SN);
            const float e0 = rand01(rng_copy), e1 = rand01(rng_copy);
            const float3 Ld = cosine_hemisphere_aligned<FAST>(e0, e1, SNn);
            pdiff = 1.0f - specular_probability<FAST>(saturate1(dot3(V, SNn)), specular_f0(surf.albedo, surf.metalness), surf.albedo);
            o = hitP + surf.GN * 1e-2f; // :607
            dir = Ld;
            tmin = 0.001f, tmax = kTraceMax;
            throughput = throughput * (surf.albedo * (1.0f - surf.metalness)); // :613
            if (rand01(rng) < pdiff) {
                throughput = f3(fdiv<FAST>(throughput.x, pdiff), fdiv<FAST>(throughput.y, pdiff), fdiv<FAST>(throughput.z, pdiff)); // :614-618
                flags |= NEB_PATH_DIVIDED;
            }
        }
        if constexpr (TAIL != 0) {
            if (ends_in_grid) {
                // the point: the hit as the path forms it, the shading normal turned toward the ray (a terminal backface hit is lit too)
                const float sd = __fadd_rn(__fadd_rn(rounded_mul(surf.SN.x, dir.x), rounded_mul(surf.SN.y, dir.y)), rounded_mul(surf.SN.z, dir.z));
                tail_live = true;
                tail_p = hitP;
                tail_n = sd <= 0.0f ? surf.SN : -surf.SN;
                tail_k = throughput_in * (surf.albedo * (1.0f - surf.metalness)); // the two products of :613, had the path gone on
                tail_added = added;
                tail_flags = flags;
                if (tail.frame_weight) { // the pdiff of the bounce that is not taken, and NEB_INDIRECT_FRAME_WEIGHT's reasoning: E[factor] = 2 - pd
                    const float3 SNn = normalize3<FAST>(surf.SN);
                    tail_pd = 1.0f - specular_probability<FAST>(saturate1(dot3(V, SNn)), specular_f0(surf.albedo, surf.metalness), surf.albedo);
                    const float factor = tail_pd > 0.0f ? __fsub_rn(2.0f, tail_pd) : 1.0f;
                    tail_k = f3(rounded_mul(tail_k.x, factor), rounded_mul(tail_k.y, factor), rounded_mul(tail_k.z, factor));
                }
            }
        }
        if constexpr (VERTICES) {
            float4* rec = vrec + 6 * (size_t)(k - 1u);
            if (alive) {
                rec[0] = seg_o;
                rec[1] = seg_d;
                rec[2] = make_float4(throughput_in.x, throughput_in.y, throughput_in.z, __uint_as_float(rng_in));
                rec[3] = make_float4(added.x, added.y, added.z, __uint_as_float(flags));
                rec[4] = make_float4(__uint_as_float(geometry), __uint_as_float(primitive), bu, bv);
                rec[5] = make_float4(seg_tmax, pdiff, 0.0f, 0.0f);
            } else {
                for (int q = 0; q < 6; ++q)
                    rec[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        alive = bounce;
    }
    if constexpr (VERTICES) {
        for (; k <= last; ++k) // (the wave left the loop early: every record is written)
            for (int q = 0; q < 6; ++q)
                vrec[6 * (size_t)(k - 1u) + q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if constexpr (TAIL != 0) {
        // every lane that entered the loop is here: one gather for the wave, its uniform or its per-lane route as the points fall
        GatherPoint tail_point;
        const bool tail_usable = locate_point(tail.G, make_float4(tail_p.x, tail_p.y, tail_p.z, 0.0f), make_float4(tail_n.x, tail_n.y, tail_n.z, 0.0f), tail_live,
                                              tail_point);
        float3 tail_E;
        float tail_W;
        uint32_t tail_corners;
        gather_wave<TAIL == 2>(tail.G, tail.records, tail_point, tail_usable, tail_E, tail_W, tail_corners, tail.visibility, tail.normal_bias);
        if (tail_live) {
            if (tail_usable && tail_W > 0.0f) { // (else NEB_GATHER_NOT_GATHERED or NEB_GATHER_NO_PROBE: the plain call's record)
                tail_added = f3(__fadd_rn(tail_added.x, rounded_mul(rounded_mul(tail_k.x, tail_E.x), kPiInv)),
                                __fadd_rn(tail_added.y, rounded_mul(rounded_mul(tail_k.y, tail_E.y), kPiInv)),
                                __fadd_rn(tail_added.z, rounded_mul(rounded_mul(tail_k.z, tail_E.z), kPiInv)));
                path_flags |= NEB_PATH_TAIL;
                if constexpr (VERTICES) {
                    float4* rec = vrec + 6 * (size_t)(last - 1u);
                    rec[3] = make_float4(tail_added.x, tail_added.y, tail_added.z, __uint_as_float(tail_flags | NEB_PATH_TAIL));
                    reinterpret_cast<float*>(rec + 5)[1] = tail_pd;
                }
            }
            sum = last == 1u ? tail_added : sum + tail_added;
        }
    }
