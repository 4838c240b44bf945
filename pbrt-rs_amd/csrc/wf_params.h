// wf_params.h — the sampler's and the pass's parameters as the kernels of wavefront.h take them (part of wf_state.h). Two plain
// structs in a header of their own, so that the host half of a render (host_render.h) fills them without the kernels' headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pb {

// PixelSampler tables (sampler.rs:252-318) of this GPU's pixels, one column per pixel:
// tables[elem * n_pix + pix]; elem: 1D dimension d, sample s -> d*spp + s; 2D -> off2 + (d*spp + s)*2 + c;
// requested 2D array a (n values per pixel sample) -> arrays[a].y + (s*n + k)*2 + c.
struct SamplerParams {
    int kind;      // PbrtSamplerKind
    int n_dims;    // n_sampled_dimensions
    int nx, ny, jitter;
    int n_arrays;
    int off2;      // first element of the 2D tables
    int n_elems;   // elements per pixel
    float* tables;
    const int2* arrays;  // per requested array: (n, first element)
    // HaltonSampler (halton.rs:24-37, 63-98) + GlobalSampler::array_end_dim (sampler.rs:344-345)
    int h_scale[2], h_exp[2];
    int h_stride, array_end_dim;
    unsigned int h_minv[2];
    const uint16_t* perms;         // compute_radical_inverse_permutations (lowdiscrepancy.rs:333-349)
    const uint32_t* primes;        // [0, 1000): primes, [1000, 2000): prime sums
};

struct PassParams {
    SamplerParams smp;
    int n_pix;         // pixels in this GPU's tile set (n_tiles * 256)
    int n_samples;     // samples of this pass
    int group_shift;   // path layout: a wave of 64 paths = (64 >> group_shift) consecutive pixels x (1 << group_shift) consecutive
                       // samples of each (0: 64 pixels of one sample index; 6: the 64 samples of one pixel); n_samples is a
                       // multiple of 1 << group_shift (path_to_sample_pixel / sample_pixel_to_path)
    int sample0;       // first sample index of this pass
    int spp;           // total samples per pixel (RNG keying)
    int width, height;
    int x0, y0, x1, y1;
    int sb_x0, sb_y0, sb_w;  // Film::get_sample_bounds of the whole film: origin and width (pixel_number)
    uint64_t seed;
    int max_depth;
    float rr_threshold;
    int light_strategy;
    float filter_rx, filter_ry;       // reconstruction filter radius
    const float* filter_table;        // 16 x 16 table (device), nullptr = 0.5 box (exact in-order path)
    float max_sample_luminance;       // Film::max_sample_luminance (film.rs:24), +inf = no clamp
    // pbrt_hip_li: the caller's stream key of every path (RNG::set_sequence argument); nullptr = the (pixel, sample) keys
    const uint64_t* stream_keys;
};

}  // namespace pb
