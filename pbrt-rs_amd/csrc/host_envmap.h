// host_envmap.h — InfiniteAreaLight's image map on the host: MIPMap::new (src/core/mipmap.rs:76-183, ImageWrap::Repeat,
// no trilinear flag) over the texels x L, and the 2W x 2H sin-weighted Distribution2D (src/lights/infinite.rs:59-73,
// src/core/sampling.rs:62-215) as the device reads it (scene.h: DevEnvMap). Intended semantics: DESIGN.md, D33 / D40 / D48 / D59-D62.
#pragma once
#include <cstdint>
#include <vector>

namespace pb {

struct EnvTables {
    int w = 0, h = 0;            // level 0 after resampling (powers of two)
    std::vector<float> level0;   // w * h * 3, row 0 = t = 0 = theta 0 (light-space +z)
    int nu = 0, nv = 0;          // 2w, 2h
    std::vector<float> func;     // nv * nu: the conditional rows' functions
    std::vector<float> cdf;      // nv * (nu + 1): their cdfs
    std::vector<float> row_int;  // nv: their integrals = the marginal's function
    std::vector<float> marg_cdf; // nv + 1
    float marg_int = 0.0f;
    float power_rgb[3] = {0, 0, 0};  // lookup((0.5, 0.5), 0.5), before the pi r^2 of InfiniteAreaLight::power
};

// the resampled size of a width x height map, or a reason (null pointer, size < 1, table past 2^28 texels)
const char* envmap_resolution(int32_t width, int32_t height, int* res_w, int* res_h);
// validates and builds everything; returns null or the reason the input was refused (`out` untouched then)
const char* envmap_build(const float* rgb, int32_t width, int32_t height, const float L[3], EnvTables* out);

}  // namespace pb
