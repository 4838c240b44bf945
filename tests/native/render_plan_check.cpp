// render_plan_check.cpp — host-side check of the render's host half (test infrastructure, built and run by
// tests/test_render_plan_host.py under AddressSanitizer and UBSan; not part of the product library).
//
// Links the product's own pbrt-rs_amd/csrc/host_render.cpp and host_film.cpp and checks
//   - the message plan_render gives for every refusal of the render path, from the inputs the GPU tests feed pbrt_hip_render,
//     pbrt_hip_li and pbrt_hip_camera_rays (the messages are written out here as the entry points have always given them), and
//     which of two refusals a doubly wrong input reports;
//   - what the plan computes, against statements that do not restate it: the sampler's samples per pixel, the pass size from a
//     stated number of free bytes, group_shift of every pass, the sampler's table layout against a recomputation of its own, the
//     HaltonSampler's constants and tables, the tile set of a film whose size is no multiple of the tile.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../pbrt-rs_amd/csrc/host_render.h"

namespace {

using pb::plan_render;
using pb::RenderCall;
using pb::RenderPlan;
using pb::RenderSceneFacts;
using pb::RenderStep;

int g_failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++g_failures;                                  \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

constexpr size_t kFree280 = (size_t)280 << 30;

// a scene of the Cornell box's size with two lights of 4 and 9 samples
const int kLightSamples[2] = {4, 9};
RenderSceneFacts facts(int n_lights = 2) {
    RenderSceneFacts f;
    for (int a = 0; a < 3; ++a) f.root_min[a] = 0.0f, f.root_max[a] = 1.0f;
    f.n_lights = n_lights;
    f.light_samples = kLightSamples;
    return f;
}
// scene.render(cam, w, h, spp) of the Python binding with its defaults
PbrtRenderParams params(int w, int h, int spp) {
    PbrtRenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.integrator = PBRT_INTEGRATOR_PATH;
    rp.max_depth = 5;
    rp.rr_threshold = 1.0f;
    rp.spp = spp;
    rp.width = w;
    rp.height = h;
    rp.x1 = w;
    rp.y1 = h;
    rp.tile_world = 1;
    return rp;
}
RenderPlan frame(const PbrtRenderParams& rp, const RenderSceneFacts& f = facts(), size_t free_b = kFree280, int camera = PBRT_CAMERA_PERSPECTIVE) {
    return plan_render(rp, RenderCall::Frame, 0, camera, f, free_b);
}
void expect_refusal(const RenderPlan& p, RenderStep at, const char* want, const char* what) {
    const std::string got = p.refusal ? p.refusal : "";
    CHECK(got == want, "%s: expected \"%s\", got \"%s\"", what, want, got.c_str());
    CHECK(p.refused_at == at, "%s: refused at step %d, expected %d", what, (int)p.refused_at, (int)at);
}

const char* kStackless = "PBRT_TRAVERSAL_STACKLESS: single-level triangle scenes only";

// ---- every refusal of the render path, and which one of two wins ----
void check_refusals() {
    const PbrtRenderParams good = params(32, 32, 2);
    CHECK(frame(good).refusal == nullptr, "the good frame is refused: %s", frame(good).refusal);
    auto with = [&](auto edit) {
        PbrtRenderParams rp = good;
        edit(rp);
        return rp;
    };
    // tests/test_gpu_intersect.py: integrator 9, a stratified sampler of 0 x 4, bounds past the film, rank 3 of 2, light_strategy 7,
    // AO without samples, camera kind 5
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = 9; })), RenderStep::Params, "integrator must be a PbrtIntegratorKind", "integrator");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.sampler = PBRT_SAMPLER_STRATIFIED, r.sampler_x = 0, r.sampler_y = 4, r.sampler_dims = 4; })),
                   RenderStep::Params, "stratified sampler: sampler_x * sampler_y must be in [1, 65536]", "stratified");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.x1 = 64, r.y1 = 64; })), RenderStep::Params, "pixel bounds outside the film's sample bounds", "bounds");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.tile_rank = 3, r.tile_world = 2; })), RenderStep::Params, "tile_rank outside [0, tile_world)", "tile_rank");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.light_strategy = 7; })), RenderStep::LightStrategy,
                   "path: light_strategy must be 0 (uniform), 1 (power) or 2 (spatial)", "light_strategy");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_AO, r.ao_samples = 0; })), RenderStep::Params,
                   "ambient occlusion: ao_samples must be in [1, 65535]", "ao_samples");
    expect_refusal(frame(good, facts(), kFree280, 5), RenderStep::Camera, "unknown camera kind", "camera kind");
    // tests/test_gpu_render.py: shade_order 3, ray_order 2, samples_per_wave 3 / 128 / -1, Halton under UniformSampleAll
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.shade_order = 3; })), RenderStep::ShadeOrder,
                   "shade_order must be 0 (queue order), 1 (by material inside blocks) or 2 (sorted queue)", "shade_order");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.ray_order = 2; })), RenderStep::RayOrder,
                   "ray_order must be 0 (Morton order from the second bounce on) or 1 (queue order)", "ray_order");
    for (int bad : {3, 128, -1})
        expect_refusal(frame(with([bad](PbrtRenderParams& r) { r.samples_per_wave = bad; })), RenderStep::Params,
                       "samples_per_wave must be 0 (library default) or a power of two up to 64", "samples_per_wave");
    {
        std::vector<int> many(300, 1);  // 3 bounces x 300 lights x 2 arrays: dimension 5 + 2 * 1800 is past the prime table
        RenderSceneFacts f = facts(300);
        f.light_samples = many.data();
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_DIRECT, r.max_depth = 3, r.sampler = PBRT_SAMPLER_HALTON; }), f),
                       RenderStep::Sampler, "Halton sampler: too many sample arrays for 1000 dimensions", "halton arrays");
        std::vector<int> more(600, 1);  // 32 x 600 x 2 arrays > 0x7fff
        f.n_lights = 600, f.light_samples = more.data();
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_DIRECT, r.max_depth = 32, r.sampler = PBRT_SAMPLER_STRATIFIED, r.sampler_x = r.sampler_y = 1; }), f),
                       RenderStep::Sampler, "too many sample arrays (max_depth x lights)", "arrays");
    }
    // the rest of normalise_params
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.spp = 0; })), RenderStep::Params, "width, height and spp must be positive", "spp");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.sampler = 4; })), RenderStep::Params, "unknown sampler", "sampler");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.sampler = PBRT_SAMPLER_ZEROTWO, r.sampler_dims = 64; })), RenderStep::Params, "sampler_dims must be in [0, 63]", "sampler_dims");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.sampler = PBRT_SAMPLER_ZEROTWO, r.spp = 65537; })), RenderStep::Params, "(0,2)-sequence sampler: spp too large", "(0,2) spp");
    {
        float table[256];
        for (float& v : table) v = 0.5f;
        PbrtRenderParams r = good;
        r.filter_table = table;
        r.filter_radius[0] = 65.0f, r.filter_radius[1] = 2.0f;
        expect_refusal(frame(r), RenderStep::Params, "filter radius too large", "filter radius");
    }
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_WHITTED, r.max_depth = 65; })), RenderStep::Params,
                   "direct lighting / Whitted: max_depth > 64 (frame stack)", "frame stack");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.max_depth = -1; })), RenderStep::Params, "bad max_depth", "max_depth");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.tile_order = 2; })), RenderStep::Params, "tile_order must be a PbrtTileOrder", "tile_order");
    // sizes ("camera rays: too many samples for one pass" guards an export's single pass, which normalisation already fixes: no
    // input reaches it)
    expect_refusal(frame(params(1 << 20, 1 << 20, 1)), RenderStep::Tiles, "tile partition: too many tiles", "2^32 tiles");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.width = r.x1 = 32768, r.height = r.y1 = 32768, r.spp = r.spp_per_pass = 1, r.tile_order = PBRT_TILE_ORDER_ROW_MAJOR; })), RenderStep::QueueLimit,
                   "too many concurrent paths for 32-bit queue entries; lower spp_per_pass", "queue limit");
    expect_refusal(plan_render(with([](PbrtRenderParams& r) { r.width = r.x1 = 16384, r.height = r.y1 = 16384, r.spp = 8, r.tile_order = PBRT_TILE_ORDER_ROW_MAJOR; }), RenderCall::Export, 0,
                               PBRT_CAMERA_PERSPECTIVE, facts(), kFree280),
                   RenderStep::QueueLimit, "too many concurrent paths for 32-bit queue entries; lower spp_per_pass", "export: one pass of everything");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.sampler = PBRT_SAMPLER_STRATIFIED, r.sampler_x = r.sampler_y = 256, r.sampler_dims = 63, r.width = r.x1 = 1024, r.height = r.y1 = 1024; })),
                   RenderStep::Sampler, "sampler tables exceed 64 GB: lower spp, sampler_dims or the light sample counts", "tables");
    {
        const int heavy[2] = {40000, 30000};
        RenderSceneFacts f = facts();
        f.light_samples = heavy;
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_DIRECT, r.max_depth = 1; }), f), RenderStep::LightSamples,
                       "too many light samples per vertex", "light samples");
    }
    {
        std::vector<int> ones(400000, 1);  // 64^3 voxels x (2 x 400 000 + 2) floats
        RenderSceneFacts f = facts(400000);
        f.light_samples = ones.data();
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.light_strategy = 2; }), f), RenderStep::Spatial,
                       "spatial light distribution: voxels x lights exceed 4 GB; use \"power\"", "voxels");
        const RenderPlan ok = frame(with([](PbrtRenderParams& r) { r.light_strategy = 2; }));
        CHECK(ok.spatial && ok.spatial_voxels[0] == 64 && ok.spatial_voxels[1] == 64 && ok.spatial_voxels[2] == 64, "a cube has 64^3 voxels");
        CHECK(!frame(with([](PbrtRenderParams& r) { r.light_strategy = 2; }), facts(1)).spatial, "one light: uniform");
    }
    {  // tests/test_gpu_traversal_modes.py: the stackless walk refuses an instanced scene
        RenderSceneFacts f = facts();
        f.trace_refusal = kStackless;
        expect_refusal(frame(good, f), RenderStep::Trace, kStackless, "stackless");
        // ... between ray_order and shade_order
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.ray_order = 2, r.shade_order = 3; }), f), RenderStep::RayOrder,
                       "ray_order must be 0 (Morton order from the second bounce on) or 1 (queue order)", "ray_order before stackless");
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.shade_order = 3; }), f), RenderStep::Trace, kStackless, "stackless before shade_order");
    }
    // li: tests/test_gpu_li.py's batches are good; the batch size is the one refusal of its own
    expect_refusal(plan_render(good, RenderCall::Li, 0, 0, facts(), 0), RenderStep::Params, "li: batch size must be in [1, 2^28]", "li 0");
    expect_refusal(plan_render(good, RenderCall::Li, (1ll << 28) + 1, 0, facts(), 0), RenderStep::Params, "li: batch size must be in [1, 2^28]", "li 2^28 + 1");
    // precedence: the order the render has always reached them in
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = 9, r.ray_order = 2; })), RenderStep::Params, "integrator must be a PbrtIntegratorKind",
                   "params before ray_order");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.width = r.x1 = 32768, r.height = r.y1 = 32768, r.spp = r.spp_per_pass = 1, r.tile_order = PBRT_TILE_ORDER_ROW_MAJOR, r.ray_order = 2; })),
                   RenderStep::QueueLimit, "too many concurrent paths for 32-bit queue entries; lower spp_per_pass", "queue limit before ray_order");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.shade_order = 3, r.light_strategy = 7; })), RenderStep::ShadeOrder,
                   "shade_order must be 0 (queue order), 1 (by material inside blocks) or 2 (sorted queue)", "shade_order before light_strategy");
    expect_refusal(frame(with([](PbrtRenderParams& r) { r.light_strategy = 7; }), facts(), kFree280, 5), RenderStep::Camera, "unknown camera kind",
                   "camera before light_strategy");
    {
        std::vector<int> many(300, 250);
        RenderSceneFacts f = facts(300);
        f.light_samples = many.data();
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_DIRECT, r.max_depth = 3, r.sampler = PBRT_SAMPLER_HALTON; }), f, kFree280, 5),
                       RenderStep::Sampler, "Halton sampler: too many sample arrays for 1000 dimensions", "sampler before light samples and camera");
        expect_refusal(frame(with([](PbrtRenderParams& r) { r.integrator = PBRT_INTEGRATOR_DIRECT, r.max_depth = 1; }), f, kFree280, 5), RenderStep::LightSamples,
                       "too many light samples per vertex", "light samples before camera");
    }
    // a rank with no tile renders nothing and refuses nothing of what follows
    const RenderPlan idle = frame(with([](PbrtRenderParams& r) { r.tile_rank = 7, r.tile_world = 8, r.ray_order = 2; }));
    CHECK(idle.origins.empty() && !idle.refusal, "a 2 x 2 tile frame has no tile for rank 7 of 8");

    // pbrt_hip_camera_rays' own
    int64_t n = -1;
    CHECK(pb::export_ray_count(good, &n) == nullptr && n == 4 * 256 * 2, "32 x 32 x 2: %lld rays", (long long)n);
    CHECK(std::string(pb::export_ray_count(with([](PbrtRenderParams& r) { r.tile_rank = 3, r.tile_world = 2; }), &n)) ==
              "camera rays: bad tile_rank / tile_world / tile_order",
          "camera rays: rank");
}

// ---- the sampler's samples per pixel ----
void check_sampler_spp() {
    PbrtRenderParams rp = params(32, 32, 7);
    rp.sampler = PBRT_SAMPLER_STRATIFIED, rp.sampler_x = 3, rp.sampler_y = 5, rp.sampler_dims = 4;
    CHECK(frame(rp).rp.spp == 15, "stratified 3 x 5: %d", frame(rp).rp.spp);
    rp = params(32, 32, 5);
    rp.sampler = PBRT_SAMPLER_ZEROTWO, rp.sampler_dims = 4;
    CHECK(frame(rp).rp.spp == 8, "(0,2) at 5: %d", frame(rp).rp.spp);
    for (int sampler : {PBRT_SAMPLER_RANDOM, PBRT_SAMPLER_STRATIFIED, PBRT_SAMPLER_ZEROTWO, PBRT_SAMPLER_HALTON}) {
        rp = params(32, 32, 4);
        rp.integrator = PBRT_INTEGRATOR_AO, rp.ao_samples = 5;
        rp.sampler = sampler, rp.sampler_x = rp.sampler_y = 2, rp.sampler_dims = 4;
        const RenderPlan p = frame(rp);
        // Sampler::round_count is the identity but for the (0,2) sampler; the RandomSampler is never asked
        CHECK(p.rp.ao_samples == (sampler == PBRT_SAMPLER_ZEROTWO ? 8 : 5), "sampler %d: ao_samples %d", sampler, p.rp.ao_samples);
        CHECK(p.ds_ao_samples == p.rp.ao_samples && p.ds_mode == PBRT_INTEGRATOR_AO, "DirectState follows");
    }
}

// ---- the pass size from the free bytes ----
void check_pass_size() {
    PbrtRenderParams rp = params(1920, 1080, 64);
    RenderPlan p = frame(rp);
    CHECK(p.n_pix == 120 * 68 * 256, "1080p: %d pixels in whole tiles", p.n_pix);
    CHECK(p.spp_pass == 64 && p.N == (size_t)p.n_pix * 64, "1920 x 1080 x 64 at 280 GB free is one pass: %d", p.spp_pass);
    // two thirds of the free bytes at 526 B per path
    const size_t free_b = (size_t)30 << 30;
    p = frame(rp, facts(), free_b);
    const long long paths = (long long)(free_b / 3 * 2 / 526);
    CHECK(p.spp_pass == (int)(paths / p.n_pix) && p.spp_pass >= 1 && p.spp_pass < 64, "30 GB: %d samples per pass", p.spp_pass);
    CHECK(p.N == (size_t)p.n_pix * p.spp_pass, "N");
    // the others: 400 + 24 + 48 max_depth, one half
    rp.integrator = PBRT_INTEGRATOR_DIRECT, rp.max_depth = 3;
    p = frame(rp, facts(), free_b);
    CHECK(p.spp_pass == (int)((long long)(free_b / 2 / (400 + 24 + 48 * 3)) / p.n_pix), "direct at 30 GB: %d", p.spp_pass);
    // the floor of 2^20 paths (nothing free) and the cap of 2^28 (everything free)
    rp = params(64, 64, 1024);
    p = frame(rp, facts(), 0);
    CHECK(p.spp_pass == (1 << 20) / (64 * 64), "floor: %d", p.spp_pass);
    rp = params(16, 16, 1 << 22);
    p = frame(rp, facts(), (size_t)1 << 50);
    CHECK(p.spp_pass == (1 << 28) / 256, "cap: %d", p.spp_pass);
    // the caller's own
    rp = params(64, 64, 4);
    rp.spp_per_pass = 3;
    p = frame(rp, facts(), 0);
    CHECK(p.spp_pass == 3 && p.N == (size_t)p.n_pix * 3, "spp_per_pass 3");
    rp.spp_per_pass = 9;
    CHECK(frame(rp).spp_pass == 4, "spp_per_pass is clamped to the spp");
    // an export is one pass, a batch one sample
    CHECK(plan_render(rp, RenderCall::Export, 0, PBRT_CAMERA_PERSPECTIVE, facts(), 0).spp_pass == 4, "export");
    p = plan_render(rp, RenderCall::Li, 300, 0, facts(), 0);
    CHECK(p.spp_pass == 1 && p.n_pix == 512 && p.N == 512 && p.valid_pixels == 300 && !p.tabulated, "a batch of 300 rays: two tiles of one sample");
}

// ---- group_shift of every pass ----
void check_group_shift() {
    for (int sampler : {PBRT_SAMPLER_RANDOM, PBRT_SAMPLER_STRATIFIED, PBRT_SAMPLER_ZEROTWO, PBRT_SAMPLER_HALTON})
        for (int spp : {1, 3, 4, 6, 64, 96})
            for (int spw : {0, 1, 4, 64})
                for (int per_pass : {0, 1, 3, 4, 64})
                    for (RenderCall call : {RenderCall::Frame, RenderCall::Li, RenderCall::Export}) {
                        PbrtRenderParams rp = params(32, 32, spp);
                        rp.sampler = sampler, rp.sampler_dims = 2, rp.samples_per_wave = spw, rp.spp_per_pass = per_pass;
                        if (sampler == PBRT_SAMPLER_STRATIFIED) rp.sampler_x = spp, rp.sampler_y = 1;
                        const RenderPlan p = plan_render(rp, call, 300, PBRT_CAMERA_PERSPECTIVE, facts(), kFree280);
                        CHECK(!p.refusal, "refused: %s", p.refusal);
                        if (p.refusal) continue;
                        const bool table_sampler = call != RenderCall::Li && (sampler == PBRT_SAMPLER_STRATIFIED || sampler == PBRT_SAMPLER_ZEROTWO);
                        const int want = spw > 0 ? spw : table_sampler ? 1 : 64;
                        int covered = 0;
                        for (int s0 = 0; s0 < p.rp.spp; s0 += p.spp_pass) {
                            const pb::PassParams pp = p.pass_params(s0);
                            covered += pp.n_samples;
                            CHECK(pp.sample0 == s0 && pp.n_samples >= 1 && pp.n_samples <= p.spp_pass && pp.n_pix == p.n_pix && pp.spp == p.rp.spp, "pass at %d", s0);
                            const int g = 1 << pp.group_shift;
                            if (call != RenderCall::Frame) {
                                CHECK(pp.group_shift == 0, "li and export keep the caller's order");
                                continue;
                            }
                            int best = 1;  // the largest power of two within the request that divides the pass's samples
                            while (best * 2 <= want && best * 2 <= 64 && pp.n_samples % (best * 2) == 0) best *= 2;
                            CHECK(pp.n_samples % g == 0 && g == best, "sampler %d spp %d spw %d pass of %d samples: group %d, expected %d", sampler, spp, spw,
                                  pp.n_samples, g, best);
                        }
                        CHECK(covered == p.rp.spp, "the passes cover %d of %d samples", covered, p.rp.spp);
                    }
}

// ---- the sampler's table layout, recomputed here from sampler.rs ----
void check_layout(const RenderPlan& p, const std::vector<int>& array_sizes, const char* what) {
    const int spp = p.rp.spp;
    const bool halton = p.rp.sampler == PBRT_SAMPLER_HALTON;
    const int dims = halton ? 0 : p.rp.sampler_dims;
    CHECK(p.smp.kind == p.rp.sampler && p.smp.n_dims == dims, "%s: kind, n_dims", what);
    CHECK(p.smp.off2 == dims * spp, "%s: off2 %d", what, p.smp.off2);  // the 1D tables come first: dims x spp values
    CHECK(p.smp.n_arrays == (int)array_sizes.size() && p.arrays.size() == array_sizes.size(), "%s: %d arrays", what, p.smp.n_arrays);
    CHECK(p.smp.array_end_dim == 5 + 2 * (int)array_sizes.size(), "%s: array_end_dim %d", what, p.smp.array_end_dim);
    long long at = (long long)dims * spp + (long long)dims * spp * 2;  // ... then the 2D tables: dims x spp pairs
    for (size_t a = 0; a < array_sizes.size() && a < p.arrays.size(); ++a) {
        CHECK(p.arrays[a].x == array_sizes[a], "%s: array %zu holds %d, expected %d", what, a, p.arrays[a].x, array_sizes[a]);
        CHECK(p.arrays[a].y == at, "%s: array %zu starts at %d, expected %lld (no gap, no overlap)", what, a, p.arrays[a].y, at);
        at += (long long)array_sizes[a] * spp * 2;  // n pairs per pixel sample
    }
    CHECK(p.smp.n_elems == (halton ? 0 : at), "%s: n_elems %d, the arrays end at %lld", what, p.smp.n_elems, at);
}
void check_sampler_layout() {
    for (int sampler : {PBRT_SAMPLER_STRATIFIED, PBRT_SAMPLER_ZEROTWO, PBRT_SAMPLER_HALTON}) {
        // the direct integrator, UniformSampleAll, two lights of 4 and 9 samples at max_depth 3: per bounce and light two arrays
        PbrtRenderParams rp = params(33, 17, 4);
        rp.integrator = PBRT_INTEGRATOR_DIRECT, rp.max_depth = 3, rp.light_strategy = 0;
        rp.sampler = sampler, rp.sampler_x = rp.sampler_y = 2, rp.sampler_dims = 3;
        RenderPlan p = frame(rp);
        CHECK(!p.refusal, "refused: %s", p.refusal);
        const int n0 = sampler == PBRT_SAMPLER_ZEROTWO ? 4 : 4, n1 = sampler == PBRT_SAMPLER_ZEROTWO ? 16 : 9;  // round_count
        CHECK(p.prefix == std::vector<int>({0, n0, n0 + n1}), "prefix under sampler %d", sampler);
        std::vector<int> sizes;
        for (int bounce = 0; bounce < 3; ++bounce)
            for (int n : {n0, n1}) sizes.push_back(n), sizes.push_back(n);
        check_layout(p, sizes, "direct");
        // UniformSampleOne asks for no arrays
        rp.light_strategy = 1;
        check_layout(frame(rp), {}, "direct, one light per vertex");
        // AO: one array of ao_samples
        rp = params(33, 17, 4);
        rp.integrator = PBRT_INTEGRATOR_AO, rp.ao_samples = 6;
        rp.sampler = sampler, rp.sampler_x = rp.sampler_y = 2, rp.sampler_dims = 3;
        check_layout(frame(rp), {sampler == PBRT_SAMPLER_ZEROTWO ? 8 : 6}, "ao");
        // the path integrator: the dimensions alone
        rp.integrator = PBRT_INTEGRATOR_PATH;
        check_layout(frame(rp), {}, "path");
    }
    PbrtRenderParams rp = params(33, 17, 4);
    rp.integrator = PBRT_INTEGRATOR_DIRECT, rp.max_depth = 3;
    const RenderPlan p = frame(rp);  // the RandomSampler tabulates nothing and rounds nothing
    CHECK(!p.tabulated && p.arrays.empty() && p.smp.n_elems == 0 && p.prefix == std::vector<int>({0, 4, 13}), "random sampler");
}

// ---- HaltonSampler::new's constants and the radical-inverse tables ----
void check_halton() {
    for (std::pair<int, int> res : {std::pair<int, int>(33, 17), {1920, 1080}, {1, 1}, {128, 128}, {129, 100}, {64, 82}}) {
        PbrtRenderParams rp = params(res.first, res.second, 4);
        rp.sampler = PBRT_SAMPLER_HALTON;
        const RenderPlan p = frame(rp);
        CHECK(!p.refusal, "refused: %s", p.refusal);
        const int bases[2] = {2, 3}, extent[2] = {p.sb[2] - p.sb[0], p.sb[3] - p.sb[1]};
        CHECK(extent[0] == res.first && extent[1] == res.second, "box filter: the sample bounds are the film");
        for (int i = 0; i < 2; ++i) {
            const int scale = p.smp.h_scale[i], need = std::min(128, extent[i]);
            long long pw = 1;
            for (int e = 0; e < p.smp.h_exp[i]; ++e) pw *= bases[i];
            CHECK(pw == scale, "scale[%d] %d is not %d^%d", i, scale, bases[i], p.smp.h_exp[i]);
            CHECK(scale >= need && (scale == 1 || scale / bases[i] < need), "scale[%d] %d is not the smallest power >= %d", i, scale, need);
        }
        const long long s0 = p.smp.h_scale[0], s1 = p.smp.h_scale[1];
        CHECK(p.smp.h_stride == s0 * s1, "stride");
        // h_minv[0] inverts scale1 modulo scale0 and h_minv[1] scale0 modulo scale1 (halton.rs:89-92)
        CHECK(p.smp.h_minv[0] < (unsigned)std::max(1ll, s0) && (s1 * p.smp.h_minv[0]) % s0 == 1 % s0, "minv0 %u: %lld x it mod %lld", p.smp.h_minv[0], s1, s0);
        CHECK(p.smp.h_minv[1] < (unsigned)std::max(1ll, s1) && (s0 * p.smp.h_minv[1]) % s1 == 1 % s1, "minv1 %u: %lld x it mod %lld", p.smp.h_minv[1], s0, s1);
        CHECK(p.smp.n_elems == 0 && p.smp.n_dims == 0, "nothing is tabulated per pixel");
    }
    std::vector<uint32_t> primes;
    std::vector<uint16_t> perms;
    pb::halton_host_tables(&primes, &perms);
    CHECK(primes.size() == 2000 && primes[0] == 2 && primes[999] == 7919, "1000 primes from 2 to 7919");
    uint32_t sum = 0;
    bool sums = true, sorted = true, prime = true;
    for (int i = 0; i < 1000; ++i) {
        sums = sums && primes[1000 + i] == sum;
        sum += primes[i];
        sorted = sorted && (i == 0 || primes[i] > primes[i - 1]);
        for (uint32_t d = 2; d * d <= primes[i]; ++d) prime = prime && primes[i] % d != 0;
    }
    CHECK(sums && sorted && prime, "primes ascending, prime, with running sums");
    CHECK(perms.size() == sum, "one permutation entry per digit of every base: %zu of %u", perms.size(), sum);
    bool all_perms = perms.size() == sum;
    for (int i = 0; i < 1000 && all_perms; ++i) {
        std::vector<char> seen(primes[i], 0);
        for (uint32_t j = 0; j < primes[i]; ++j) {
            const uint16_t v = perms[primes[1000 + i] + j];
            if (v >= primes[i] || seen[v]) all_perms = false;
            else seen[v] = 1;
        }
    }
    CHECK(all_perms, "every block is a permutation of 0..p-1");
    CHECK(perms[0] + perms[1] == 1, "base 2");
}

// ---- tiles ----
long long in_bounds_pixels(const RenderPlan& p) {
    long long n = 0;
    for (const int2& o : p.origins)
        for (int y = o.y; y < o.y + 16; ++y)
            for (int x = o.x; x < o.x + 16; ++x) n += x >= p.rp.x0 && x < p.rp.x1 && y >= p.rp.y0 && y < p.rp.y1;
    return n;
}
void check_tiles() {
    PbrtRenderParams rp = params(33, 17, 2);
    RenderPlan p = frame(rp);
    CHECK(p.origins.size() == 6 && p.n_pix == 6 * 256, "33 x 17: 3 x 2 tiles, 256 pixels each (%zu, %d)", p.origins.size(), p.n_pix);
    CHECK(p.valid_pixels == 33 * 17 && in_bounds_pixels(p) == 33 * 17, "valid pixels %lld", (long long)p.valid_pixels);
    rp.x0 = 5, rp.y0 = 3, rp.x1 = 30, rp.y1 = 16;  // a crop window
    p = frame(rp);
    CHECK(p.origins.size() == 2 && p.origins[0].x == 5 && p.origins[0].y == 3 && p.origins[1].x == 21, "the crop's tiles start at its corner");
    CHECK(p.valid_pixels == 25 * 13 && in_bounds_pixels(p) == 25 * 13, "crop: valid pixels %lld", (long long)p.valid_pixels);
    for (int order : {PBRT_TILE_ORDER_MORTON, PBRT_TILE_ORDER_ROW_MAJOR}) {
        std::multiset<std::pair<int, int>> seen;
        long long valid = 0;
        for (int rank = 0; rank < 2; ++rank) {
            rp = params(33, 17, 2);
            rp.tile_world = 2, rp.tile_rank = rank, rp.tile_order = order;
            p = frame(rp);
            CHECK(p.origins.size() == 3 && p.world == 2 && p.rank == rank, "rank %d of 2 has 3 of the 6 tiles", rank);
            for (const int2& o : p.origins) seen.insert({o.x, o.y});
            valid += p.valid_pixels;
        }
        std::multiset<std::pair<int, int>> all;
        for (int y = 0; y < 17; y += 16)
            for (int x = 0; x < 33; x += 16) all.insert({x, y});
        CHECK(seen == all && valid == 33 * 17, "order %d: ranks 0 and 1 cover every tile once", order);
    }
    // a wider filter: the sample bounds reach outside the film and the pixels get numbers over them
    float table[256];
    for (float& v : table) v = 0.25f;
    rp = params(33, 17, 2);
    rp.filter_table = table, rp.filter_radius[0] = rp.filter_radius[1] = 2.0f;
    rp.x0 = rp.y0 = -2, rp.x1 = 35, rp.y1 = 19;
    p = frame(rp);
    CHECK(!p.refusal && !p.box && p.sb[0] == -2 && p.sb[1] == -2 && p.sb[2] == 35 && p.sb[3] == 19, "sample bounds under a radius of 2");
    const pb::PassParams pp = p.pass_params(0);
    CHECK(pp.sb_x0 == -2 && pp.sb_y0 == -2 && pp.sb_w == 37 && pp.filter_rx == 2.0f && std::isinf(pp.max_sample_luminance), "PassParams");
    CHECK(p.valid_pixels == 37 * 21 && in_bounds_pixels(p) == 37 * 21, "valid pixels over the sample bounds");
}

// ---- the sort switches ----
void check_sorts() {
    PbrtRenderParams rp = params(64, 64, 4);
    RenderPlan p = frame(rp);
    CHECK(p.sort_rays && !p.sort_shade && !p.bin_shade && !p.direct, "path: Morton order by default");
    rp.ray_order = 1, rp.shade_order = 2;
    p = frame(rp);
    CHECK(!p.sort_rays && p.sort_shade && !p.bin_shade, "queue order, sorted shading");
    rp.shade_order = 1;
    CHECK(frame(rp).bin_shade && !frame(rp).sort_shade, "binned shading");
    rp.integrator = PBRT_INTEGRATOR_WHITTED, rp.ray_order = 0;
    p = frame(rp);
    CHECK(p.direct && !p.sort_rays && !p.sort_shade && !p.bin_shade, "the stage machine sorts nothing");
    // a caller's pass past 2^28 paths is traced in queue order
    rp = params(4096, 4096, 32);
    rp.spp_per_pass = 17;
    p = frame(rp);
    CHECK(!p.refusal && p.N == ((size_t)17 << 24) && !p.sort_rays, "17 x 2^24 paths: no sort");
    rp.spp_per_pass = 16;
    CHECK(frame(rp).sort_rays, "2^28 paths: sorted");
}

}  // namespace

int main() {
    check_refusals();
    check_sampler_spp();
    check_pass_size();
    check_group_shift();
    check_sampler_layout();
    check_halton();
    check_tiles();
    check_sorts();
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
