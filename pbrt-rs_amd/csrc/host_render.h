// host_render.h — the host half of a render: everything pbrt_hip_render*, pbrt_hip_li* and pbrt_hip_camera_rays* decide about a
// call before the device is touched. plan_render maps the caller's parameters, the shape of the call, a few facts of the scene and
// the free device bytes to a RenderPlan (sizes, switches, the sampler's layout, the tile set) or to the first refusal, in the
// order the render has always reported them. Implemented in host_render.cpp, which makes no device call; RenderJob (render.hip)
// takes device blocks in the sizes the plan states, uploads its arrays and runs the passes. tests/native/render_plan_check.cpp
// runs all of it on a CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/pbrt_hip.h"
#include "wf_params.h"

namespace pb {

constexpr int kPlanTile = 16;         // wf_state.h: kTile
constexpr int kPlanPathRecBits = 28;  // wf_ray_expand.h: kPathRecBits (render.hip asserts that both agree)

enum class RenderCall { Frame, Li, Export };  // pbrt_hip_render*, pbrt_hip_li* (a batch of n rays), pbrt_hip_camera_rays*

// What the plan reads of the scene, from the host side of PbrtHipScene
struct RenderSceneFacts {
    float root_min[3], root_max[3];
    int n_lights = 0;
    const int* light_samples = nullptr;  // [n_lights]
    const char* trace_refusal = nullptr;  // kernel_select.h: choose_trace refused (its text), or null
};

// Where plan_render stopped, in the order the refusals have always been reached. RenderJob keeps its device queries (free
// memory, the rocPRIM scratch sizes) between the same refusals as before.
enum class RenderStep { None, Params, Tiles, ExportPass, QueueLimit, RayOrder, Trace, ShadeOrder, Sampler, LightSamples, Camera, LightStrategy, Spatial };

struct RenderPlan {
    const char* refusal = nullptr;  // the first refusal (every field computed before it holds), or null
    RenderStep refused_at = RenderStep::None;
    // the caller's parameters checked and normalised: li substitution, the sampler's samples per pixel, AO's round_count, an
    // export's single pass
    PbrtRenderParams rp;
    bool li_mode = false, export_mode = false;
    bool tabulated = false;  // not the RandomSampler
    bool direct = false;     // DirectLighting, Whitted and AO share the per-vertex stage machine of k_shade_direct
    bool box = true;         // the 0.5 box filter: exact in-order accumulation (k_film_accumulate)
    float frx = 0.5f, fry = 0.5f;
    int32_t sb[4] = {0, 0, 0, 0};  // pbrt_hip_sample_bounds of the film under the filter
    int world = 1, rank = 0;
    // tiles of the sample bounds (integrator.rs:402-409), dealt round-robin in rp.tile_order to the GPUs. Empty: nothing to render,
    // and nothing below is planned
    std::vector<int2> origins;
    int n_pix = 0, spp_pass = 0;
    int64_t valid_pixels = 0;
    size_t N = 0;  // concurrent paths of a pass
    bool sort_rays = false, sort_shade = false, bin_shade = false;
    std::vector<int> prefix;  // light-sample prefix sums, n_lights + 1
    // every SamplerParams field that is not a device pointer; smp.n_elems * n_pix floats of tables
    SamplerParams smp{};
    std::vector<int2> arrays;  // the requested 2D arrays: (n, first element)
    // DirectState's scalars
    int ds_light_strategy = 0, ds_mode = 0, ds_ao_samples = 0, ds_ao_cos_sample = 0;
    // path, light_strategy 2 with more than one light: SpatialLightDistribution::new(scene, 64) (lightdistrib.rs:85-107, 228)
    bool spatial = false;
    int spatial_voxels[3] = {1, 1, 1};

    // the PassParams of the pass that starts at sample s0, device pointers null (smp's, filter_table, stream_keys)
    PassParams pass_params(int s0) const;
};

// free_bytes: what the device can still give plus the context's idle cached blocks; read only where the caller leaves the pass
// size to the library (spp_per_pass <= 0). li_n: the batch size of RenderCall::Li.
RenderPlan plan_render(const PbrtRenderParams& params, RenderCall call, int64_t li_n, int32_t camera_kind, const RenderSceneFacts& scene,
                       size_t free_bytes);

int round_up_pow2(int v);  // pbrt.rs:174-182
// The samples per pixel the sampler takes (stratified.rs:30-33: nx * ny; zerotwosequence.rs:20: the next power of two). Returns the
// refusal, or null.
const char* sampler_spp(const PbrtRenderParams& rp, int32_t* spp);
// What pbrt_hip_camera_rays hands out for these parameters: the whole tiles of the rank's set times the sampler's samples per
// pixel, as plan_render will fix them. Returns the refusal, or null.
const char* export_ray_count(const PbrtRenderParams& rp, int64_t* n);

// HaltonSampler's host side: the first 1000 primes with their running sums ([0, 1000) and [1000, 2000)) and
// compute_radical_inverse_permutations (lowdiscrepancy.rs:11-170, 333-349: RNG::default + shuffle per prime)
void halton_host_tables(std::vector<uint32_t>* primes_and_sums, std::vector<uint16_t>* perms);
uint64_t multiplicative_inverse(int64_t a, int64_t n);  // halton.rs:40-49

}  // namespace pb
