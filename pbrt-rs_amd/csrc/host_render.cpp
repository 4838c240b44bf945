// host_render.cpp — the host half of a render (host_render.h): parameter normalisation and the render's refusals, the tile set,
// the pass size, the sort switches, the light-sample prefix, the sampler's table layout and the HaltonSampler's constants and
// tables. Integer arithmetic over the caller's numbers that ends up as array sizes and subscripts on the device; no device call.
#include "host_render.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pb {

int round_up_pow2(int v) {  // pbrt.rs:174-182
    v -= 1;
    v |= v >> 1;
    v |= v >> 2;
    v |= v >> 4;
    v |= v >> 8;
    v |= v >> 16;
    return v + 1;
}

const char* sampler_spp(const PbrtRenderParams& rp, int32_t* spp) {
    *spp = rp.spp;
    if (rp.sampler == PBRT_SAMPLER_STRATIFIED) {
        if (rp.sampler_x < 1 || rp.sampler_y < 1 || (int64_t)rp.sampler_x * rp.sampler_y > 65536)
            return "stratified sampler: sampler_x * sampler_y must be in [1, 65536]";
        *spp = rp.sampler_x * rp.sampler_y;
    } else if (rp.sampler == PBRT_SAMPLER_ZEROTWO) {
        if (rp.spp > 65536) return "(0,2)-sequence sampler: spp too large";
        *spp = round_up_pow2(rp.spp);
    }
    return nullptr;
}

const char* export_ray_count(const PbrtRenderParams& rp, int64_t* n) {
    int32_t n_tiles = 0;
    const int world = rp.tile_world <= 0 ? 1 : rp.tile_world;
    if (pbrt_hip_tile_partition_order(rp.x0, rp.y0, rp.x1, rp.y1, rp.tile_rank, world, rp.tile_order, nullptr, 0, &n_tiles) != PBRT_HIP_OK)
        return "camera rays: bad tile_rank / tile_world / tile_order";
    int32_t spp = 0;
    if (const char* why = sampler_spp(rp, &spp)) return why;
    *n = (int64_t)n_tiles * kPlanTile * kPlanTile * spp;  // whole tiles: pixels outside the bounds carry pixel = (-1, -1)
    return nullptr;
}

// ---- HaltonSampler host side: prime tables and compute_radical_inverse_permutations (lowdiscrepancy.rs:11-170,
// 333-349: RNG::default + shuffle per prime), HaltonSampler::new constants (halton.rs:40-98) ----
namespace {
struct HostPcg {  // rng.rs
    uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
    uint32_t u32() {
        uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27), rot = (uint32_t)(old >> 59);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31u));
    }
    uint32_t bounded(uint32_t b) {
        uint32_t threshold = (~b + 1u) % b;
        for (;;) {
            uint32_t r = u32();
            if (r >= threshold) return r % b;
        }
    }
};
void extended_gcd(uint64_t a, uint64_t b, int64_t* x, int64_t* y) {  // halton.rs:51-61
    if (b == 0) {
        *x = 1;
        *y = 0;
        return;
    }
    int64_t d = (int64_t)(a / b), xp = 0, yp = 0;
    extended_gcd(b, a % b, &xp, &yp);
    *x = yp;
    *y = xp - d * yp;
}
}  // namespace

void halton_host_tables(std::vector<uint32_t>* primes_and_sums, std::vector<uint16_t>* perms) {
    std::vector<uint32_t> primes;
    for (uint32_t v = 2; primes.size() < 1000; ++v) {
        bool is_prime = true;
        for (uint32_t q : primes) {
            if (q * q > v) break;
            if (v % q == 0) {
                is_prime = false;
                break;
            }
        }
        if (is_prime) primes.push_back(v);
    }
    primes_and_sums->assign(2000, 0);
    uint32_t acc = 0;
    for (int i = 0; i < 1000; ++i) {
        (*primes_and_sums)[i] = primes[i];
        (*primes_and_sums)[1000 + i] = acc;
        acc += primes[i];
    }
    perms->resize(acc);
    HostPcg rng;
    uint16_t* p = perms->data();
    for (int i = 0; i < 1000; ++i) {
        int count = (int)primes[i];
        for (int j = 0; j < count; ++j) p[j] = (uint16_t)j;
        for (int j = 0; j < count; ++j) std::swap(p[j], p[j + (int)rng.bounded((uint32_t)(count - j))]);  // sampling.rs:280-287
        p += count;
    }
}
uint64_t multiplicative_inverse(int64_t a, int64_t n) {  // halton.rs:40-49
    int64_t x = 0, y = 0;
    extended_gcd((uint64_t)a, (uint64_t)n, &x, &y);
    int64_t r = x - (x / n) * n;
    return (uint64_t)(r < 0 ? r + n : r);
}

namespace {
int round_count(const PbrtRenderParams& rp, int n) { return rp.sampler == PBRT_SAMPLER_ZEROTWO ? round_up_pow2(n) : n; }  // Sampler::round_count

// stage 1: returns the first refusal, or null
const char* normalise_params(RenderPlan& p, const PbrtRenderParams& rp_in, RenderCall call, int64_t li_n) {
    PbrtRenderParams& rp = p.rp;
    rp = rp_in;
    p.li_mode = call == RenderCall::Li;
    p.export_mode = call == RenderCall::Export;
    if (p.li_mode) {  // the batch stands in for a 1-spp "frame" of n pixels in a row; nothing of the film plumbing is used
        if (li_n <= 0 || li_n > (1ll << 28)) return "li: batch size must be in [1, 2^28]";
        rp.width = (int32_t)li_n;
        rp.height = 1;
        rp.spp = 1;
        rp.x0 = rp.y0 = 0;
        rp.x1 = rp.width;
        rp.y1 = 1;
        rp.tile_rank = 0;
        rp.tile_world = 1;
        rp.spp_per_pass = 1;
        rp.sampler = PBRT_SAMPLER_RANDOM;  // the caller's Sampler is a RandomSampler stream per ray (sampler.rs:452, random.rs)
        rp.filter_table = nullptr;
    }
    if (rp.width <= 0 || rp.height <= 0 || rp.spp <= 0) return "width, height and spp must be positive";
    // ---- sampler: samples per pixel and Sampler::round_count (stratified.rs:30-33, zerotwosequence.rs:20, 62-64) ----
    if (rp.sampler < PBRT_SAMPLER_RANDOM || rp.sampler > PBRT_SAMPLER_HALTON) return "unknown sampler";
    p.tabulated = rp.sampler != PBRT_SAMPLER_RANDOM;
    if (p.tabulated && (rp.sampler_dims < 0 || rp.sampler_dims > 63)) return "sampler_dims must be in [0, 63]";
    if (const char* why = sampler_spp(rp, &rp.spp)) return why;
    if (rp.integrator == PBRT_INTEGRATOR_AO && rp.ao_samples >= 1 && rp.ao_samples <= 65535 && p.tabulated)
        rp.ao_samples = round_count(rp, rp.ao_samples);  // ao.rs:36
    p.frx = rp.filter_radius[0] > 0.0f ? rp.filter_radius[0] : 0.5f;
    p.fry = rp.filter_radius[1] > 0.0f ? rp.filter_radius[1] : 0.5f;
    p.box = true;
    if (rp.filter_table) {
        if (p.frx != 0.5f || p.fry != 0.5f) p.box = false;
        for (int i = 0; i < 256; ++i)
            if (rp.filter_table[i] != 1.0f) p.box = false;
    } else {
        p.frx = p.fry = 0.5f;
    }
    if (p.frx > 64.0f || p.fry > 64.0f) return "filter radius too large";
    pbrt_hip_sample_bounds(rp.width, rp.height, p.frx, p.fry, p.sb);
    if (rp.x0 < p.sb[0] || rp.y0 < p.sb[1] || rp.x1 > p.sb[2] || rp.y1 > p.sb[3] || rp.x0 > rp.x1 || rp.y0 > rp.y1)
        return "pixel bounds outside the film's sample bounds";
    if (rp.integrator < PBRT_INTEGRATOR_PATH || rp.integrator > PBRT_INTEGRATOR_AO) return "integrator must be a PbrtIntegratorKind";
    p.direct = rp.integrator != PBRT_INTEGRATOR_PATH;
    if (p.direct && rp.max_depth > 64) return "direct lighting / Whitted: max_depth > 64 (frame stack)";
    if (rp.integrator == PBRT_INTEGRATOR_AO && (rp.ao_samples < 1 || rp.ao_samples > 65535))
        return "ambient occlusion: ao_samples must be in [1, 65535]";
    if (rp.max_depth < 0 || rp.max_depth > 1 << 20) return "bad max_depth";
    p.world = rp.tile_world <= 0 ? 1 : rp.tile_world;
    p.rank = rp.tile_rank;
    if (p.rank < 0 || p.rank >= p.world) return "tile_rank outside [0, tile_world)";
    if (rp.tile_order != PBRT_TILE_ORDER_MORTON && rp.tile_order != PBRT_TILE_ORDER_ROW_MAJOR) return "tile_order must be a PbrtTileOrder";
    if (rp.samples_per_wave < 0 || rp.samples_per_wave > 64 || (rp.samples_per_wave & (rp.samples_per_wave - 1)) != 0)
        return "samples_per_wave must be 0 (library default) or a power of two up to 64";
    if (p.export_mode) rp.spp_per_pass = rp.spp;  // one pass: the export is indexed by the paths of that pass
    return nullptr;
}

// stage 2: the samples of a pixel one pass holds
int size_pass(const RenderPlan& p, size_t free_b) {
    const PbrtRenderParams& rp = p.rp;
    int spp_pass = rp.spp_per_pass > 0 ? rp.spp_per_pass : 0;
    if (spp_pass == 0) {
        // As many samples of a pixel in flight as two thirds of the free HBM hold (the other integrators: half of it, as
        // ever). The path integrator takes 500 B per path:
        // 192 B rays (two generations) + 96 B hits + 104 B pending estimates (two generations) + 52 B persistent state +
        // 32 B queues + 12 B sort pairs (one per path: keys in / out, sorted values) + 12 B special-list slots; 526 leaves
        // room for the sampler tables. The others keep one
        // generation and add their stage machine's frame stack. A whole 64-spp 1080p frame is 133 M paths = 67 GB of the
        // 288 GB and runs 6 large wavefronts instead of 48 small ones (+10 % on config 3: fewer launches and host round
        // trips, shorter tails). The share was one half while a path took 376 B; at 500 B a half of 280 GB free would just
        // admit the 265 M paths (133 GB) of a 32-spp pass of a 4K frame, two thirds (355 M paths) do with room to spare.
        // free_b counts the blocks kept from the previous render: they are available to this one.
        const int64_t per_path = rp.integrator == PBRT_INTEGRATOR_PATH ? 526 : 400 + 24 + 48ll * std::max(1, rp.max_depth);
        const size_t share = rp.integrator == PBRT_INTEGRATOR_PATH ? free_b / 3 * 2 : free_b / 2;
        const int64_t target_paths = std::max<int64_t>(1ll << 20, std::min<int64_t>(1ll << 28, (int64_t)share / per_path));
        spp_pass = (int)std::max<int64_t>(1, std::min<int64_t>(rp.spp, target_paths / p.n_pix));
    }
    return std::min(spp_pass, rp.spp);
}

// stage 4: SamplerParams of the render: the Halton constants, the requested 2D arrays, the table sizes. Returns the refusal, or null
const char* plan_sampler(RenderPlan& p, const RenderSceneFacts& scene) {
    const PbrtRenderParams& rp = p.rp;
    SamplerParams& smp = p.smp;
    p.prefix.assign(scene.n_lights + 1, 0);
    for (int i = 0; i < scene.n_lights; ++i)  // directlighting.rs:58-62: round_count with a tabulating sampler
        p.prefix[i + 1] = p.prefix[i] + (p.tabulated ? round_count(rp, scene.light_samples[i]) : scene.light_samples[i]);
    // ---- PixelSampler tables: n_dims 1D + n_dims 2D dimensions and the requested 2D arrays, per pixel ----
    smp.kind = rp.sampler;
    smp.n_dims = rp.sampler_dims;
    smp.nx = rp.sampler_x;
    smp.ny = rp.sampler_y;
    smp.jitter = rp.sampler_jitter;
    if (rp.sampler == PBRT_SAMPLER_HALTON) {
        smp.n_dims = 0;  // nothing is tabulated per pixel: every value is a function of (sample index, dimension)
        // HaltonSampler::new(spp, film.get_sample_bounds(), false) (halton.rs:63-98)
        const int res[2] = {p.sb[2] - p.sb[0], p.sb[3] - p.sb[1]};
        for (int i = 0; i < 2; ++i) {
            int base = i == 0 ? 2 : 3, scale = 1, exp = 0;
            while (scale < std::min(128, res[i])) {
                scale *= base;
                ++exp;
            }
            smp.h_scale[i] = scale;
            smp.h_exp[i] = exp;
        }
        smp.h_stride = smp.h_scale[0] * smp.h_scale[1];
        smp.h_minv[0] = (unsigned int)multiplicative_inverse(smp.h_scale[1], smp.h_scale[0]);
        smp.h_minv[1] = (unsigned int)multiplicative_inverse(smp.h_scale[0], smp.h_scale[1]);
    }
    if (p.tabulated) {
        int64_t elems = (int64_t)smp.n_dims * rp.spp * 3;
        smp.off2 = smp.n_dims * rp.spp;
        auto request_2d_array = [&](int n) {  // sampler.rs:41-46
            p.arrays.push_back(make_int2(n, (int)elems));
            elems += (int64_t)n * rp.spp * 2;
        };
        if (rp.integrator == PBRT_INTEGRATOR_DIRECT && rp.light_strategy == 0) {
            for (int i = 0; i < rp.max_depth; ++i)  // directlighting.rs:64-75
                for (int k = 0; k < scene.n_lights; ++k) {
                    request_2d_array(p.prefix[k + 1] - p.prefix[k]);
                    request_2d_array(p.prefix[k + 1] - p.prefix[k]);
                }
        } else if (rp.integrator == PBRT_INTEGRATOR_AO) {
            request_2d_array(rp.ao_samples);  // ao.rs:37
        }
        if (p.arrays.size() > 0x7fff) return "too many sample arrays (max_depth x lights)";
        if (elems * p.n_pix * 4 > (64ll << 30) || elems >= (1ll << 31))
            return "sampler tables exceed 64 GB: lower spp, sampler_dims or the light sample counts";
        smp.n_arrays = (int)p.arrays.size();
        smp.array_end_dim = 5 + 2 * smp.n_arrays;  // sampler.rs:344-345
        if (rp.sampler == PBRT_SAMPLER_HALTON) {
            // start_pixel fills the arrays' dimensions 5..array_end_dim (sampler.rs:355-368); the first one past the
            // prime table indexes PRIME_SUMS out of range (halton.rs:100-108) and the reference panics there
            if (smp.array_end_dim > 1000) return "Halton sampler: too many sample arrays for 1000 dimensions";
            elems = 0;
        }
        smp.n_elems = (int)elems;
    }
    return nullptr;
}
}  // namespace

RenderPlan plan_render(const PbrtRenderParams& params, RenderCall call, int64_t li_n, int32_t camera_kind, const RenderSceneFacts& scene,
                       size_t free_bytes) {
    RenderPlan p;
    const PbrtRenderParams& rp = p.rp;
    auto refuse = [&p](RenderStep at, const char* why) {
        p.refused_at = at;
        p.refusal = why;
    };
    if (const char* why = normalise_params(p, params, call, li_n)) return refuse(RenderStep::Params, why), p;

    // tiles of the sample bounds (integrator.rs:402-409), dealt round-robin in rp.tile_order to the GPUs
    if (p.li_mode) {
        p.origins.assign((size_t)((li_n + kPlanTile * kPlanTile - 1) / (kPlanTile * kPlanTile)), make_int2(0, 0));  // 256 rays per "tile"
    } else {
        int32_t n_mine = 0;
        if (pbrt_hip_tile_partition_order(rp.x0, rp.y0, rp.x1, rp.y1, p.rank, p.world, rp.tile_order, nullptr, 0, &n_mine) != PBRT_HIP_OK)
            return refuse(RenderStep::Tiles, "tile partition: too many tiles"), p;
        p.origins.resize(n_mine);
        pbrt_hip_tile_partition_order(rp.x0, rp.y0, rp.x1, rp.y1, p.rank, p.world, rp.tile_order, (int32_t*)p.origins.data(), n_mine, &n_mine);
    }
    if (p.origins.empty()) return p;
    p.n_pix = (int)p.origins.size() * kPlanTile * kPlanTile;
    for (const int2& o : p.origins)
        p.valid_pixels += (int64_t)(std::min(o.x + kPlanTile, rp.x1) - o.x) * (std::min(o.y + kPlanTile, rp.y1) - o.y);
    if (p.li_mode) p.valid_pixels = li_n;
    p.spp_pass = size_pass(p, free_bytes);
    if (p.export_mode && p.spp_pass != rp.spp) return refuse(RenderStep::ExportPass, "camera rays: too many samples for one pass"), p;
    p.N = (size_t)p.n_pix * p.spp_pass;
    if (p.N * 4 >= (1ull << 32))
        return refuse(RenderStep::QueueLimit, "too many concurrent paths for 32-bit queue entries; lower spp_per_pass"), p;

    // ray-queue sort (spatial order for the bounce rays)
    // only the path integrator's later bounces are incoherent; the stage machine of the other integrators keeps
    // shooting from the camera rays' hit points, which are already in pixel order (AO: -6 % with the sort).
    // PbrtRenderParams.ray_order = 1 leaves the queues as the shading kernel filled them (results do not depend on it).
    if (rp.ray_order < 0 || rp.ray_order > 1)
        return refuse(RenderStep::RayOrder, "ray_order must be 0 (Morton order from the second bounce on) or 1 (queue order)"), p;
    // What is sorted is one pair per path (wf_ray_expand.h), whose value packs the record index into kPathRecBits bits: the
    // passes size_pass makes stay within that; a caller's own spp_per_pass beyond it is traced in queue order.
    p.sort_rays = rp.ray_order == 0 && rp.integrator == PBRT_INTEGRATOR_PATH && p.N <= ((size_t)1 << kPlanPathRecBits);
    if (scene.trace_refusal) return refuse(RenderStep::Trace, scene.trace_refusal), p;
    // sort-by-material shading (wf_path.h): PbrtRenderParams.shade_order; 2 = the whole shade queue in material order
    if (rp.shade_order < 0 || rp.shade_order > 2)
        return refuse(RenderStep::ShadeOrder, "shade_order must be 0 (queue order), 1 (by material inside blocks) or 2 (sorted queue)"), p;
    p.sort_shade = rp.shade_order == 2 && rp.integrator == PBRT_INTEGRATOR_PATH;
    p.bin_shade = rp.shade_order == 1 && rp.integrator == PBRT_INTEGRATOR_PATH;

    if (const char* why = plan_sampler(p, scene)) return refuse(RenderStep::Sampler, why), p;
    if (p.direct) {
        p.ds_light_strategy = rp.light_strategy;
        p.ds_mode = rp.integrator;
        p.ds_ao_samples = rp.ao_samples;
        p.ds_ao_cos_sample = rp.light_strategy != 0;
        if (p.prefix.back() >= 0xfff0) return refuse(RenderStep::LightSamples, "too many light samples per vertex"), p;
    }
    if (camera_kind < PBRT_CAMERA_PERSPECTIVE || camera_kind > PBRT_CAMERA_ENVIRONMENT) return refuse(RenderStep::Camera, "unknown camera kind"), p;
    if (rp.integrator == PBRT_INTEGRATOR_PATH && (rp.light_strategy < 0 || rp.light_strategy > 2))
        return refuse(RenderStep::LightStrategy, "path: light_strategy must be 0 (uniform), 1 (power) or 2 (spatial)"), p;
    if (rp.integrator == PBRT_INTEGRATOR_PATH && rp.light_strategy == 2 && scene.n_lights > 1) {
        // create_light_sample_distribution("spatial") -> SpatialLightDistribution::new(scene, 64) (lightdistrib.rs:85-107, 228)
        p.spatial = true;
        const float *mn = scene.root_min, *mx = scene.root_max;
        float diag[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
        int ext = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : (diag[1] > diag[2] ? 1 : 2);
        for (int i = 0; i < 3; ++i) p.spatial_voxels[i] = std::max(1, (int)std::round(diag[i] / diag[ext] * 64.0f));
        size_t n_voxels = (size_t)p.spatial_voxels[0] * p.spatial_voxels[1] * p.spatial_voxels[2];
        size_t floats = n_voxels * (size_t)(2 * scene.n_lights + 2);
        if (floats > (1ull << 30)) return refuse(RenderStep::Spatial, "spatial light distribution: voxels x lights exceed 4 GB; use \"power\""), p;
    }
    return p;
}

// the PassParams of the pass that starts at sample s0
PassParams RenderPlan::pass_params(int s0) const {
    PassParams pp;
    pp.smp = smp;
    pp.n_pix = n_pix;
    pp.n_samples = std::min(spp_pass, rp.spp - s0);
    // PbrtRenderParams.samples_per_wave: the largest power of two <= the request that divides the pass's samples per pixel
    // default: a wave = the samples of ONE pixel (as many as the pass has, up to 64). The tabulating samplers keep the
    // old layout: their tables are [element][pixel], read coalesced when a wave's lanes are 64 pixels of one sample
    const int want = rp.samples_per_wave > 0 ? rp.samples_per_wave : ((tabulated && rp.sampler != PBRT_SAMPLER_HALTON) ? 1 : 64);
    pp.group_shift = 0;
    while ((2 << pp.group_shift) <= want && pp.group_shift < 6 && pp.n_samples % (2 << pp.group_shift) == 0) ++pp.group_shift;
    if (li_mode || export_mode) pp.group_shift = 0;  // batches of rays / the exported camera rays keep the caller's order
    pp.sample0 = s0;
    pp.spp = rp.spp;
    pp.width = rp.width;
    pp.height = rp.height;
    pp.x0 = rp.x0;
    pp.y0 = rp.y0;
    pp.x1 = rp.x1;
    pp.y1 = rp.y1;
    pp.sb_x0 = sb[0];
    pp.sb_y0 = sb[1];
    pp.sb_w = sb[2] - sb[0];
    pp.seed = rp.seed;
    pp.max_depth = rp.max_depth;
    pp.rr_threshold = rp.rr_threshold;
    pp.light_strategy = rp.light_strategy;
    pp.filter_rx = frx;
    pp.filter_ry = fry;
    pp.filter_table = nullptr;
    pp.max_sample_luminance = rp.max_sample_luminance > 0.0f ? rp.max_sample_luminance : INFINITY;
    pp.stream_keys = nullptr;
    return pp;
}

}  // namespace pb
