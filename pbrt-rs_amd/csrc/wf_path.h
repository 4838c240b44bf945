// wf_path.h — k_shade: PathIntegrator::li, one bounce per launch (part of wavefront.h)
#pragma once
#include "wf_lights.h"

namespace pb {

// Sort-by-material shading (north_star; the reference dispatches per hit to the material, interaction.rs:318-329 ->
// material.rs:16-55). Key of a shade-queue entry = what k_shade will branch on: 0 no continuation hit to shade (escaped /
// dead path, only the pending estimate is resolved), 1 + material type otherwise. PbrtRenderParams.shade_order selects:
//   0  queue order (one path per lane as the queue has them),
//   1  material order INSIDE each block of 256 queue entries: the block's entries are counting-sorted by key through LDS
//      before shading, so a wave shades (mostly) one material while the block still touches the same 256 paths' state —
//      the reads stay as coalesced as the queue is (round 3),
//   2  the whole queue radix-sorted by key (round 2's experiment: lane utilisation doubles, the 290 B of path state per
//      path become scattered gathers and the kernel gets slower). What is sorted are the queue POSITIONS (`order`): an
//      entry's position is the index of its transient records, the path number is looked up from it.
// Films are bit-identical in all three: a path's arithmetic does not depend on which lane runs it.
// p = the path, rec = its position in the shade queue (where its hit record is)
PB_DEV uint32_t shade_key(const ShadeConsts& sc, const PathState& ps, uint32_t p, uint32_t rec, int max_depth) {
    int fb = __float_as_int(ps.beta[p].w);
    uint32_t key = 0;
    if ((fb & PF_ALIVE) && (fb >> 8) < max_depth) {
        const size_t hb = hit_index(ps, rec, RS_CONT);
        int slot = __float_as_int(ps.hit[hb].x), inst = hit_instance(ps, hb);
        if (slot >= 0) {
            int mat = __float_as_int(sc.bvh.tris[3 * (size_t)slot + 2].z);
            if (sc.bvh.instanced && inst >= 0) {
                int over = __float_as_int(sc.bvh.instances[7 * (size_t)inst + 6].x);
                if (over >= 0) mat = over;
            }
            key = 1u + (uint32_t)sc.materials[mat].type;
        }
    }
    return key;
}
PB_PLAIN_KERNEL void k_shade_sort_keys(ShadeConsts sc, PathState ps, const uint32_t* __restrict__ shade_queue, uint32_t n, int max_depth,
                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ positions) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = shade_key(sc, ps, shade_queue[i], i, max_depth);
    positions[i] = i;
}

// keys: 0 nothing to shade, 1 + DevMaterial::type (none, matte, mirror, glass; level 1: plastic, metal as well; level 2: the
// three kinds of set_material rows as well; level 3: Disney rows as well; level 4: lobe rows as well), the last = no queue entry
// (block tail)
constexpr int shade_keys(int level) { return level == 4 ? 13 : level == 3 ? 12 : level == 2 ? 11 : level == 1 ? 8 : 6; }
template <int KEYS>
struct ShadeBins {
    uint32_t count[4][KEYS];  // per wave of the block, per key
    uint32_t path[256];
    uint32_t rec[256];  // the entry's queue position travels with it
};

#ifndef PB_SHADE_WAVES
#define PB_SHADE_WAVES 3  // 162 VGPRs; 4 waves (128 VGPRs, spills) measured in profiles/r04_wide_kernel_ladder.txt
#endif
// LEVEL: which non-specular BSDFs the scene's material table needs. 0: matte only. 1 (GLOSSY): plastic or metal as well
// (MicrofacetReflection lobes, wf_microfacet.h); matte then goes through the same general BSDF (bit for bit the Lambertian
// code), and the instantiations without it stay as they were. 2: a row of pbrt_hip_scene_set_material as well (OrenNayar,
// glossy transmission, FresnelBlend: GenBsdf, wf_bxdfs.h), the rows of level 1 through the functions of level 1. Level 2
// fits the same launch bounds without scratch: 162 / 164 VGPRs (profiles/r08_bxdf_set.txt). 3: a Disney row as well (DisneyBsdf,
// wf_disney.h). At three waves per SIMD the binned level 3 spills 12 bytes, so level 3 alone is bounded at two
// (profiles/r09_disney.txt). 4: a lobe row as well (LobeBsdf, wf_lobes.h: a list of specular and non-specular lobes matched by
// flags); only k_shade_lobes below is built at it, and the rows of every other kind go through level 3's code there.
// Thread i takes the shade-queue entry at position rec = i (order: rec = order[i], the queue in material order): the path
// p = qin.shade[rec] with its persistent state at p, and the transient records of this generation at rec. What the path
// hands to the next launch is staged in LDS and written to the next generation at its position in qout.shade.
// SHP: the scene may hold general quadric shapes (surface_from_hit, light_sample_li); k_shade_shapes below is that build, so the
// kernels of every other scene compile as they did without it. ML: it may hold a projection or goniometric light (light_sample_li);
// k_shade_maps below is that build, and k_shade_shapes takes it too. MOV: it holds moving instances (sc.motions): the surface is
// rebuilt through the instance's rows at the path's time, which rides in the fourth component of the ray's second float4 and is
// copied to every ray the path emits (spawn_ray keeps the time); k_shade_moving below is that build. CRV (with SHP): it holds curve
// segments (sc.curves): a curve's surface is rebuilt from the continuation ray (make_surface_curve); k_shade_curves below.
// HAIR (with CRV): the table holds a kMatHair row: the BSDF type is HairBsdf (wf_hair.h, which only hair_kernels.hip includes: the
// type is named through LevelBsdf<kHairBsdfLevel>, a dependent name), h comes from the hit record's v, and the bins have a key more.
constexpr int kHairBsdfLevel = 5;
template <bool BIN, int LEVEL, bool SHP, bool ML = false, bool MOV = false, bool CRV = false, bool HAIR = false>
PB_DEV void shade_bounce(const ShadeConsts& sc, const PathState& ps, const Queues& qin, const Queues& qout, const PassParams& pp,
                         const TileList& tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    constexpr bool GLOSSY = LEVEL >= 1;
    constexpr bool LOBES = LEVEL == 4;
    constexpr int kShadeKeys = HAIR ? 2 + kMatHair + 1 : shade_keys(LEVEL);  // HAIR: 0, 1 + type up to kMatHair, the block tail
    constexpr int BL = HAIR ? kHairBsdfLevel : LEVEL;                        // the BSDF type: LevelBsdf<BL>
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = i < n_in;
    uint32_t rec = (active && order) ? order[i] : i;
    uint32_t p = active ? qin.shade[rec] : 0u;
    __shared__ StagedRecords staged;
    const StageSink stage{staged};
    if (BIN) {
        // counting sort of the block's 256 entries by key: rank inside the wave by ballot + mbcnt, waves and keys through LDS
        __shared__ ShadeBins<kShadeKeys> bins;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint32_t key = active ? shade_key(sc, ps, p, rec, pp.max_depth) : (uint32_t)(kShadeKeys - 1);
        uint32_t rank = 0;
#pragma unroll
        for (int k = 0; k < kShadeKeys; ++k) {
            const unsigned long long m = __ballot(key == (uint32_t)k);
            if (key == (uint32_t)k) rank = lane_prefix(m);
            if (lane == 0) bins.count[wave][k] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t before = 0;  // entries of smaller keys in the block, and of this key in the waves before this one
        for (int k = 0; k < kShadeKeys; ++k)
            for (int w = 0; w < 4; ++w)
                before += ((uint32_t)k < key || ((uint32_t)k == key && w < wave)) ? bins.count[w][k] : 0u;
        bins.path[before + rank] = p;
        bins.rec[before + rank] = rec;
        uint32_t n_active = 0;
        for (int k = 0; k < kShadeKeys - 1; ++k)
            for (int w = 0; w < 4; ++w) n_active += bins.count[w][k];
        __syncthreads();
        p = bins.path[threadIdx.x];
        rec = bins.rec[threadIdx.x];
        active = threadIdx.x < n_active;
    }
    bool emit_cont = false, emit_mis = false, emit_shadow = false, mis_bool = false;

    uint32_t cell = 0;  // sort cell of the rays this path emits
    float time = 0.0f;  // MOV: the path's time
    if (active) {
        float4 Lq = ps.L[p], bq = ps.beta[p];
        V3 L = V3{Lq.x, Lq.y, Lq.z};
        float eta_scale = Lq.w;
        V3 beta = V3{bq.x, bq.y, bq.z};
        int fb = __float_as_int(bq.w);
        int flags = fb & 0xff, bounces = fb >> 8;
        size_t rbase = ray_index(ps, rec, RS_CONT), hbase = hit_index(ps, rec, RS_CONT);

        // ---- (1) resolve the pending direct-lighting estimate (integrator.rs:136-266) ----
        if (flags & (PF_NEE_SHADOW | PF_NEE_MIS)) {
            float pick_pdf;
            V3 beta_v;
            V3 ld = estimate_direct_resolve<SHP>(sc, ps, rec, flags, &pick_pdf, &beta_v);
            ld = ld / pick_pdf;                 // integrator.rs:133
            L = L + mulv(beta_v, ld);           // path.rs:113-120
            flags &= ~(PF_NEE_SHADOW | PF_NEE_MIS);
        }

        // ---- (2) the continuation hit ----
        if (flags & PF_ALIVE) {
            flags &= ~PF_ALIVE;
            float4 r0 = ps.ray[rbase], r1 = ps.ray[rbase + 1];
            V3 rd = V3{r0.w, r1.x, r1.y};
            float4 h0 = ps.hit[hbase];
            int hslot = __float_as_int(h0.x);
            bool found = hslot >= 0;
            Surf sf;
            if (MOV) time = r1.w;
            if (found) {
                if constexpr (CRV)
                    sf = surface_from_hit_curves(sc.bvh, sc.curves, hslot, h0.y, h0.z, h0.w, V3{r0.x, r0.y, r0.z}, rd);
                else if constexpr (MOV)
                    sf = surface_from_hit_moving(sc.bvh, sc.motions, time, hslot, hit_instance(ps, hbase), h0.y, h0.z, h0.w, rd);
                else
                    sf = surface_from_hit<SHP>(sc.bvh, hslot, hit_instance(ps, hbase), h0.y, h0.z, h0.w, rd);
                if (qout.keys) cell = ray_sort_cell(sf.p.x, sf.p.y, sf.p.z, qout.key_lo, qout.key_inv);
            }
            // path.rs:80-88
            if (bounces == 0 || (flags & PF_SPECULAR_BOUNCE)) {
                if (found) {
                    L = L + mulv(beta, surface_le(sc, sf, -rd));
                } else {
                    for (int k = 0; k < sc.n_infinite; ++k) {
                        DevLight lt = sc.lights[sc.infinite_ids[k]];
                        V3 le = lt.slot >= 0 ? env_le(sc.env_maps[lt.slot], rd) : V3{lt.L[0], lt.L[1], lt.L[2]};
                        L = L + mulv(beta, le);
                    }
                }
            }
            if (found && bounces < pp.max_depth) {  // path.rs:90
                DevMaterial mat = sc.materials[sf.material];
                Samp sm = path_sampler(ps, pp, tiles, p);
                if (mat.type == PBRT_MAT_NONE) {
                    // path.rs:95-98: no BSDF -> continue through the surface, bounces unchanged
                    V3 o = offset_ray_origin(sf.p, sf.p_error, sf.n, rd);
                    stage.ray(RS_CONT, o, rd, kInf);
                    flags |= PF_ALIVE;
                    emit_cont = true;
                } else {
                    Frame fr = make_frame(sf);
                    V3 kd = V3{mat.kd[0], mat.kd[1], mat.kd[2]};
                    V3 kt = V3{mat.kt[0], mat.kt[1], mat.kt[2]};
                    V3 wo = -rd;  // path.rs:122 `let wo = -ray.d` (estimate_direct uses isect.wo = sf.wo)
                    bool has_lobe;  // which BxDFs the material adds: pbrt-v3 rules (matte / mirror / glass / plastic / metal; level 2: Oren-Nayar / rough glass / substrate rows)
                    bool nonspecular;
                    typename LevelBsdf<BL>::type nsb;
                    if (GLOSSY) {
                        load_bsdf(sc, sf.material, mat, &nsb);
                        if constexpr (HAIR) nsb.h = -1.0f + 2.0f * h0.z;  // the curve's hit record carries (u, v, 0)
                        nonspecular = nsb.n > 0;
                        if (mat.type == PBRT_MAT_GLASS) has_lobe = !(is_black(kd) && is_black(kt));
                        else if (mat.type == PBRT_MAT_MIRROR) has_lobe = !is_black(kd);
                        else has_lobe = nonspecular;
                        if constexpr (LOBES)
                            if (nsb.row) has_lobe = nsb.row->n > 0;  // nonspecular: num_components(BSDF_ALL & !BSDF_SPECULAR) > 0
                    } else {
                        if (mat.type == PBRT_MAT_GLASS) has_lobe = !(is_black(kd) && is_black(kt));
                        else has_lobe = !is_black(kd);
                        nonspecular = (mat.type == PBRT_MAT_MATTE) && has_lobe;
                    }

                    // ---- uniform_sample_one_light (integrator.rs:92-134) ----
                    if (nonspecular && sc.n_lights > 0) {
                        float u_pick = samp_1d(pp, sm);
                        DevDistribution1D distrib = light_distribution_lookup(sc, sf.p);  // path.rs:115
                        int light_num = find_interval_cdf(distrib.cdf, distrib.n + 1, u_pick);
                        float pick_pdf = distrib.func_int > 0.0f ? distrib.func[light_num] / (distrib.func_int * (float)distrib.n)
                                                                 : 0.0f;
                        if (pick_pdf != 0.0f) {
                            float ul0, ul1, us0, us1;
                            samp_2d(pp, sm, &ul0, &ul1);
                            samp_2d(pp, sm, &us0, &us1);
                            int nee_flags = GLOSSY ? estimate_direct_emit<SHP, ML>(sc, stage, sf, fr, true, nsb, light_num, ul0, ul1, us0,
                                                                                   us1, pick_pdf, beta)
                                                   : estimate_direct_emit<SHP, ML>(sc, stage, sf, fr, true, MatteBsdf{kd}, light_num, ul0, ul1,
                                                                                   us0, us1, pick_pdf, beta);
                            flags |= nee_flags & 0xff;
                            emit_shadow = (nee_flags & PF_NEE_SHADOW) != 0;
                            emit_mis = (nee_flags & PF_NEE_MIS) != 0;
                            mis_bool = (nee_flags & NEE_MIS_BOOL) != 0;
                        }
                    }

                    // ---- BSDF sampling for the next vertex (path.rs:123-152) ----
                    float u0 = 0.0f, u1 = 0.0f;
                    samp_2d(pp, sm, &u0, &u1);
                    V3 wi = V3{0.0f, 0.0f, 0.0f}, f = V3{0.0f, 0.0f, 0.0f};
                    float pdf = 0.0f;
                    bool sampled_specular = false, sampled_transmission = false;
                    bool lobe_row = false;
                    if constexpr (LOBES) lobe_row = nsb.row != nullptr;
                    if (lobe_row) {
                        // BSDF::sample_f(BSDF_ALL) over the row's list: the flag and eta_scale follow the SAMPLED lobe's type
                        if constexpr (LOBES) {
                            bool ok;
                            int sampled = 0;
                            f = lobes_sample_f(nsb.row, fr, wo, u0, u1, kBxdfAll, &wi, &pdf, &ok, &sampled);
                            if (!ok) pdf = 0.0f;
                            sampled_specular = ok && (sampled & kBxdfSpecular) != 0;
                            sampled_transmission = ok && (sampled & kBxdfTransmission) != 0;
                        }
                    } else if (has_lobe) {
                        if (GLOSSY && nonspecular) {  // glossy lobes, transmission included: not specular, PF_SPECULAR_BOUNCE stays clear
                            bool ok;
                            f = bsdf_sample_f(nsb, fr, wo, u0, u1, &wi, &pdf, &ok);
                            if (!ok) pdf = 0.0f;
                        } else if (!GLOSSY && mat.type == PBRT_MAT_MATTE) {
                            bool ok;
                            f = matte_sample_f(fr, kd, wo, u0, u1, &wi, &pdf, &ok);
                            if (!ok) pdf = 0.0f;
                        } else {
                            V3 wol = to_local(fr, wo);
                            float ur = fminr(u0 * 1.0f - 0.0f, kOneMinusEpsilon);
                            if (wol.z != 0.0f) {
                                V3 wil = V3{0.0f, 0.0f, 0.0f};
                                f = sample_specular_local(mat, kd, kt, wol, ur, 0, &wil, &pdf, &sampled_transmission);
                                sampled_specular = pdf != 0.0f;
                                if (pdf != 0.0f) wi = to_world(fr, wil);
                                else f = V3{0.0f, 0.0f, 0.0f};
                            }
                        }
                    }
                    if (!(is_black(f) || pdf == 0.0f)) {  // path.rs:136
                        beta = mulv(beta, f * (absdot(wi, fr.ns) / pdf));
                        flags = (flags & ~PF_SPECULAR_BOUNCE) | (sampled_specular ? PF_SPECULAR_BOUNCE : 0);
                        if (sampled_specular && sampled_transmission) {
                            float eta = mat.eta;  // a lobe row's DevMaterial::eta is its BSDF's eta
                            eta_scale *= (dot(wo, sf.n) > 0.0f) ? (eta * eta) : 1.0f / (eta * eta);
                        }
                        V3 o = offset_ray_origin(sf.p, sf.p_error, sf.n, wi);
                        bool alive = true;
                        // path.rs:200-207 Russian roulette (D27 intended)
                        V3 rr_beta = beta * eta_scale;
                        if (max_comp(rr_beta) < pp.rr_threshold && bounces > 3) {
                            float qq = fmaxr(0.05f, 1.0f - max_comp(rr_beta));
                            if (samp_1d(pp, sm) < qq) alive = false;
                            else beta = beta / (1.0f - qq);
                        }
                        if (alive) {
                            stage.ray(RS_CONT, o, wi, kInf);
                            flags |= PF_ALIVE;
                            emit_cont = true;
                            bounces += 1;
                        }
                    }
                }
                samp_store(ps, p, sm);
            }
        }
        ps.L[p] = make_float4(L.x, L.y, L.z, eta_scale);
        ps.beta[p] = make_float4(beta.x, beta.y, beta.z, __int_as_float((bounces << 8) | flags));
    }

    // ---- queue appends (block-aggregated): reserve, move the staged records to the reserved position, write the entries ----
    __shared__ BlockAppend sh;
    const bool again = emit_cont || emit_mis || emit_shadow;
    const AppendSlots slots = block_reserve(sh, qout, emit_cont, emit_mis, emit_shadow, again);
    if (MOV) {  // rays are only emitted from a continuation hit, where the time was read
        if (emit_cont) staged.ray[RS_CONT][1][threadIdx.x].w = time;
        if (emit_mis) staged.ray[RS_MIS][1][threadIdx.x].w = time;
        if (emit_shadow) staged.ray[RS_SHADOW][1][threadIdx.x].w = time;
    }
    stage.flush(ps, slots.shade, emit_cont, emit_mis, emit_shadow);
    block_write(qout, slots, p, slots.shade, emit_cont, emit_mis, emit_shadow, again, cell, mis_bool);
}
template <bool BIN, int LEVEL>
__global__ void __launch_bounds__(256, LEVEL == 3 ? 2 : PB_SHADE_WAVES) k_shade(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                 TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, LEVEL, false>(sc, ps, qin, qout, pp, tiles, n_in, order);
}
// scenes with general shapes: the level-3 BSDF set serves every material table (matte, plastic, metal and the set_material rows go
// through it bit for bit as through the lower levels)
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_shapes(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                        TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 3, true, true>(sc, ps, qin, qout, pp, tiles, n_in, order);
}
// scenes with a projection or goniometric light: the most general level only, bounded at two waves as level 3 is
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_maps(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                      TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 3, false, true>(sc, ps, qin, qout, pp, tiles, n_in, order);
}
// scenes with a lobe row (pbrt_hip_scene_set_lobe_material): level 4 only. Bounded at two waves per SIMD as level 3 is: the
// lobe loop's live state comes on top of level 3's, which spills at three (profiles/r12_lobe_materials.txt).
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_lobes(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                       TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 4, false, false>(sc, ps, qin, qout, pp, tiles, n_in, order);
}
// scenes with moving instances: the level-3 BSDF set, which serves every material table; bounded at two waves as level 3 is
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_moving(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                        TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 3, false, false, true>(sc, ps, qin, qout, pp, tiles, n_in, order);
}
// scenes with curve segments: the build for shapes with the curve's surface added (profiles/curve_resource_usage.txt)
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_curves(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                        TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 3, true, true, false, true>(sc, ps, qin, qout, pp, tiles, n_in, order);
}

// scenes with curve segments whose table holds a hair row (wf_hair.h): the curve build with HairBsdf (profiles/hair_resource_usage.txt).
// Instantiated in hair_kernels.hip alone.
template <bool BIN>
__global__ void __launch_bounds__(256, 2) k_shade_hair(ShadeConsts sc, PathState ps, Queues qin, Queues qout, PassParams pp,
                                                      TileList tiles, uint32_t n_in, const uint32_t* __restrict__ order) {
    shade_bounce<BIN, 3, true, true, false, true, true>(sc, ps, qin, qout, pp, tiles, n_in, order);
}

}  // namespace pb
