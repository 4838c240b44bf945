// host_envmap.h — InfiniteAreaLight's image map on the host: MIPMap::new (src/core/mipmap.rs:76-183, ImageWrap::Repeat,
// no trilinear flag) over the texels x L, and the 2W x 2H sin-weighted Distribution2D (src/lights/infinite.rs:59-73,
// src/core/sampling.rs:62-215) as the device reads it (scene.h: DevEnvMap). Intended semantics: DESIGN.md, D33 / D40 / D48 / D59-D62.
// What an edit makes of the tables (the light's transform and power, the texels, the power distribution): host_edit.h.
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

// ProjectionLight's / GonioPhotometricLight's map (src/lights/projection.rs:36-88, goniometric.rs:32-63): the MIPMap over the
// texels as they are (I multiplies the lookup), the projector's screen window and the light's power for I = 1 (D89)
struct LightMapTables {
    int w = 0, h = 0;                // level 0 after resampling; 0 x 0: no map
    std::vector<float> level0;       // w * h * 3
    float lookup_rgb[3] = {1, 1, 1};  // lookup((0.5, 0.5), 0.5); 1 without a map
    float screen_bounds[4] = {0, 0, 0, 0};  // projection: min.x, min.y, max.x, max.y
    float inv_tan = 0.0f;            // projection: 1 / tan(radians(fov) / 2)
    float cos_total_width = -1.0f;   // projection: z of the normalised light-space direction through the corner (max.x, max.y)
    float power_rgb[3] = {0, 0, 0};  // Light::power for I = (1, 1, 1)
};
// the projector's window and inv_tan for a width x height map (0 x 0: no map, aspect 1), in double, rounded once; returns
// cos_total_width (-1 for a goniometric light)
double light_map_geometry(int32_t type, float fov, int32_t width, int32_t height, float screen_bounds[4], float* inv_tan);
// validates and builds everything (rgb null: no map); returns null or the reason the input was refused (`out` untouched then)
const char* light_map_build(int32_t type, float fov, const float* rgb, int32_t width, int32_t height, LightMapTables* out);

}  // namespace pb
