// host_envmap.cpp — InfiniteAreaLight::new's tables (src/lights/infinite.rs:36-82) on the host, no device code:
// MIPMap::new / lookup / triangle / texel (src/core/mipmap.rs:76-296; ImageWrap::Repeat, no trilinear flag) over the texels
// x L, and the 2W x 2H sin-weighted Distribution2D over their luminance (src/core/sampling.rs:62-215). Evaluated in double
// and stored as float; the departures from the reference as written are DESIGN.md's D33, D40, D48 and D59-D62.
#include "host_envmap.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/pbrt_hip.h"
#include "abi_guard.h"

namespace pb {
namespace {

constexpr double kPiD = 3.14159265358979323846;
constexpr int64_t kMaxTableTexels = int64_t(1) << 28;

int64_t round_up_pow2(int64_t v) {  // pbrt.rs round_up_pow2_i32
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
int64_t wrap(int64_t i, int64_t n) {  // ImageWrap::Repeat with a signed index (D60)
    int64_t r = i % n;
    return r < 0 ? r + n : r;
}
double lanczos(double x, double tau) {  // texture.rs:200-212
    x = std::fabs(x);
    if (x < 1e-5) return 1.0;
    if (x > 1.0) return 0.0;
    x *= kPiD;
    double s = std::sin(x * tau) / (x * tau);
    return s * (std::sin(x) / x);
}
struct ResampleWeight {
    int64_t first_texel;
    double weight[4];
};
std::vector<ResampleWeight> resample_weights(int64_t old_res, int64_t new_res) {  // mipmap.rs:263-281
    std::vector<ResampleWeight> wt(new_res);
    const double filter_width = 2.0;
    for (int64_t i = 0; i < new_res; ++i) {
        double center = ((double)i + 0.5) * (double)old_res / (double)new_res;
        wt[i].first_texel = (int64_t)std::floor(center - filter_width + 0.5);
        double sum = 0.0;
        for (int j = 0; j < 4; ++j) {
            double pos = (double)wt[i].first_texel + j + 0.5;
            wt[i].weight[j] = lanczos((pos - center) / filter_width, 2.0);
            sum += wt[i].weight[j];
        }
        for (int j = 0; j < 4; ++j) wt[i].weight[j] /= sum;
    }
    return wt;
}

// one level of the box pyramid, RGB in double
struct Level {
    int64_t w, h;
    std::vector<double> v;  // w * h * 3
    const double* texel(int64_t s, int64_t t) const { return &v[3 * (wrap(t, h) * w + wrap(s, w))]; }
};

struct MipMap {
    std::vector<Level> pyr;
    // MIPMap::triangle (mipmap.rs:283-296) with a signed floor (D60)
    void triangle(int level, double s_, double t_, double out[3]) const {
        level = std::min(std::max(level, 0), (int)pyr.size() - 1);
        const Level& l = pyr[level];
        double s = s_ * (double)l.w - 0.5, t = t_ * (double)l.h - 0.5;
        double fs = std::floor(s), ft = std::floor(t);
        int64_t s0 = (int64_t)fs, t0 = (int64_t)ft;
        double ds = s - fs, dt = t - ft;
        const double *a = l.texel(s0, t0), *b = l.texel(s0, t0 + 1), *c = l.texel(s0 + 1, t0), *d = l.texel(s0 + 1, t0 + 1);
        for (int k = 0; k < 3; ++k)
            out[k] = a[k] * ((1.0 - ds) * (1.0 - dt)) + b[k] * ((1.0 - ds) * dt) + c[k] * (ds * (1.0 - dt)) + d[k] * (ds * dt);
    }
    // MIPMap::lookup (mipmap.rs:211-227), the trilinear branch included
    void lookup(double s, double t, double width, double out[3]) const {
        const double levels = (double)pyr.size();
        double level = levels - 1.0 + std::log2(std::max(width, 1e-8));
        if (level < 0.0) {
            triangle(0, s, t, out);
        } else if (level > levels - 1.0) {
            const double* x = pyr.back().texel(0, 0);
            for (int k = 0; k < 3; ++k) out[k] = x[k];
        } else {
            double il = std::floor(level), delta = level - il;
            double a[3], b[3];
            triangle((int)il, s, t, a);
            triangle((int)il + 1, s, t, b);
            for (int k = 0; k < 3; ++k) out[k] = (1.0 - delta) * a[k] + delta * b[k];
        }
    }
};

double y_value(const double c[3]) { return 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2]; }  // spectrum.rs:679-682

// Distribution1D::new (sampling.rs:69-95; D40 intended), accumulated in double
double make_distribution(const float* f, int64_t n, float* cdf) {
    std::vector<double> c(n + 1);
    c[0] = 0.0;
    for (int64_t i = 1; i <= n; ++i) c[i] = c[i - 1] + (double)f[i - 1] / (double)n;
    double func_int = c[n];
    for (int64_t i = 0; i <= n; ++i) cdf[i] = (float)(func_int == 0.0 ? (double)i / (double)n : c[i] / func_int);
    return func_int;
}

const char* check_texels(const float* rgb, int32_t width, int32_t height, const float L[3]) {
    if (!rgb || !L) return "null pointer";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(L[k]) || L[k] < 0.0f) return "L must be finite and >= 0";
    const size_t n = (size_t)width * (size_t)height * 3;
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(rgb[i]) || rgb[i] < 0.0f) return "texels must be finite and >= 0";
        if (!std::isfinite(rgb[i] * L[i % 3])) return "a texel x L overflows float";
    }
    return nullptr;
}

// MIPMap::new (mipmap.rs:76-183) over width x height texels, each multiplied by `scale` in float (null: as they are): level 0
// as float (what the device reads, and what the pyramid is built from) and the box pyramid over it
void mipmap_build(const float* rgb, int32_t width, int32_t height, const float* scale, int rw, int rh, MipMap* out,
                  std::vector<float>* level0_out) {
    const int64_t W = width, H = height;
    std::vector<double> img((size_t)(W * H * 3));
    for (size_t i = 0; i < img.size(); ++i) img[i] = scale ? (double)(rgb[i] * scale[i % 3]) : (double)rgb[i];
    MipMap& mm = *out;
    Level l0{rw, rh, {}};
    if (rw == W && rh == H) {
        l0.v = std::move(img);  // D59: level 0 is the image itself
    } else {
        // MIPMap::new's separable Lanczos resampling (mipmap.rs:99-150): s over the original rows, then t, clamp >= 0
        std::vector<ResampleWeight> sw = resample_weights(W, rw), tw = resample_weights(H, rh);
        std::vector<double> r1((size_t)(rw * H * 3), 0.0);
        for (int64_t t = 0; t < H; ++t)
            for (int64_t s = 0; s < rw; ++s)
                for (int j = 0; j < 4; ++j) {
                    int64_t os = wrap(sw[s].first_texel + j, W);
                    for (int k = 0; k < 3; ++k) r1[3 * (t * rw + s) + k] += img[3 * (t * W + os) + k] * sw[s].weight[j];
                }
        l0.v.assign((size_t)(rw * rh * 3), 0.0);
        for (int64_t s = 0; s < rw; ++s)
            for (int64_t t = 0; t < rh; ++t) {
                double acc[3] = {0.0, 0.0, 0.0};
                for (int j = 0; j < 4; ++j) {
                    int64_t ot = wrap(tw[t].first_texel + j, H);
                    for (int k = 0; k < 3; ++k) acc[k] += r1[3 * (ot * rw + s) + k] * tw[t].weight[j];
                }
                for (int k = 0; k < 3; ++k) l0.v[3 * (t * rw + s) + k] = std::max(acc[k], 0.0);
            }
    }
    // level 0 as float: the device's texels, and what the pyramid and the tables are built from
    std::vector<float> level0(l0.v.size());
    for (size_t i = 0; i < level0.size(); ++i) {
        level0[i] = (float)l0.v[i];
        l0.v[i] = (double)level0[i];
    }
    mm.pyr.push_back(std::move(l0));
    // the 2x2 box pyramid (mipmap.rs:152-170)
    int n_levels = 1;
    for (int64_t m = std::max<int64_t>(rw, rh); m > 1; m >>= 1) ++n_levels;
    for (int i = 1; i < n_levels; ++i) {
        const Level& p = mm.pyr[i - 1];
        Level l{std::max<int64_t>(1, p.w / 2), std::max<int64_t>(1, p.h / 2), {}};
        l.v.resize((size_t)(l.w * l.h * 3));
        for (int64_t t = 0; t < l.h; ++t)
            for (int64_t s = 0; s < l.w; ++s) {
                const double *a = p.texel(2 * s, 2 * t), *b = p.texel(2 * s + 1, 2 * t), *c = p.texel(2 * s, 2 * t + 1),
                             *d = p.texel(2 * s + 1, 2 * t + 1);
                for (int k = 0; k < 3; ++k) l.v[3 * (t * l.w + s) + k] = (a[k] + b[k] + c[k] + d[k]) * 0.25;
            }
        mm.pyr.push_back(std::move(l));
    }
    *level0_out = std::move(level0);
}

}  // namespace

const char* envmap_resolution(int32_t width, int32_t height, int* res_w, int* res_h) {
    if (width < 1 || height < 1) return "width and height must be >= 1";
    int64_t rw = round_up_pow2(width), rh = round_up_pow2(height);
    if (4 * rw * rh > kMaxTableTexels) return "the map's sampling table would pass 2^28 texels";
    *res_w = (int)rw;
    *res_h = (int)rh;
    return nullptr;
}

const char* envmap_build(const float* rgb, int32_t width, int32_t height, const float L[3], EnvTables* out) {
    int rw, rh;
    if (const char* why = envmap_resolution(width, height, &rw, &rh)) return why;
    if (const char* why = check_texels(rgb, width, height, L)) return why;
    // texels x L (infinite.rs:51-53), in float as the reference multiplies them
    MipMap mm;
    std::vector<float> level0;
    mipmap_build(rgb, width, height, L, rw, rh, &mm, &level0);
    // the sin-weighted luminance image and its Distribution2D (infinite.rs:59-73; D40 intended: rows sliced by v * nu)
    EnvTables e;
    e.w = rw;
    e.h = rh;
    e.nu = 2 * rw;
    e.nv = 2 * rh;
    const int64_t nu = e.nu, nv = e.nv;
    const double fwidth = 0.5 / (double)std::min(nu, nv);
    e.func.resize((size_t)(nu * nv));
    e.cdf.resize((size_t)(nv * (nu + 1)));
    e.row_int.resize((size_t)nv);
    for (int64_t v = 0; v < nv; ++v) {
        double vp = ((double)v + 0.5) / (double)nv;
        double sin_theta = std::sin(kPiD * vp);
        for (int64_t u = 0; u < nu; ++u) {
            double up = ((double)u + 0.5) / (double)nu, c[3];
            mm.lookup(up, vp, fwidth, c);
            e.func[(size_t)(v * nu + u)] = (float)(y_value(c) * sin_theta);
        }
        e.row_int[(size_t)v] = (float)make_distribution(&e.func[(size_t)(v * nu)], nu, &e.cdf[(size_t)(v * (nu + 1))]);
    }
    e.marg_cdf.resize((size_t)(nv + 1));
    double marg_int = make_distribution(e.row_int.data(), nv, e.marg_cdf.data());
    e.marg_int = (float)marg_int;
    if (!std::isfinite(e.marg_int)) return "the map's luminance overflows float";
    double pw[3];
    mm.lookup(0.5, 0.5, 0.5, pw);  // InfiniteAreaLight::power (infinite.rs:131-133) before the pi r^2
    for (int k = 0; k < 3; ++k) e.power_rgb[k] = (float)pw[k];
    e.level0 = std::move(level0);
    *out = std::move(e);
    return nullptr;
}

double light_map_geometry(int32_t type, float fov, int32_t width, int32_t height, float screen_bounds[4], float* inv_tan) {
    if (type != PBRT_LIGHT_PROJECTION) {
        screen_bounds[0] = screen_bounds[1] = screen_bounds[2] = screen_bounds[3] = 0.0f;
        *inv_tan = 0.0f;
        return -1.0;  // the whole sphere
    }
    // projection.rs:57-76
    const double aspect = (width > 0 && height > 0) ? (double)width / (double)height : 1.0;  // in double, rounded once
    if (aspect > 1.0) {
        screen_bounds[0] = (float)-aspect, screen_bounds[1] = -1.0f, screen_bounds[2] = (float)aspect, screen_bounds[3] = 1.0f;
    } else {
        screen_bounds[0] = -1.0f, screen_bounds[1] = (float)(-1.0 / aspect), screen_bounds[2] = 1.0f, screen_bounds[3] = (float)(1.0 / aspect);
    }
    const double it = 1.0 / std::tan((double)fov * (kPiD / 180.0) / 2.0);
    *inv_tan = (float)it;
    // the light-space direction through the screen's corner (max.x, max.y): (x / inv_tan, y / inv_tan, 1), normalised
    const double cx = (double)screen_bounds[2] / it, cy = (double)screen_bounds[3] / it;
    return 1.0 / std::sqrt(cx * cx + cy * cy + 1.0);
}

const char* light_map_build(int32_t type, float fov, const float* rgb, int32_t width, int32_t height, LightMapTables* out) {
    if (type != PBRT_LIGHT_PROJECTION && type != PBRT_LIGHT_GONIOMETRIC) return "light type is not PBRT_LIGHT_PROJECTION or PBRT_LIGHT_GONIOMETRIC";
    if (type == PBRT_LIGHT_PROJECTION && !(std::isfinite(fov) && fov > 0.0f && fov < 180.0f)) return "fov must be finite and in (0, 180)";
    LightMapTables t;
    double look[3] = {1.0, 1.0, 1.0};
    if (rgb) {
        int rw, rh;
        if (const char* why = envmap_resolution(width, height, &rw, &rh)) return why;
        const float one[3] = {1.0f, 1.0f, 1.0f};
        if (const char* why = check_texels(rgb, width, height, one)) return why;
        MipMap mm;
        mipmap_build(rgb, width, height, nullptr, rw, rh, &mm, &t.level0);  // the texels as they are: I multiplies the lookup
        t.w = rw;
        t.h = rh;
        mm.lookup(0.5, 0.5, 0.5, look);
    }
    const double cos_total_width = light_map_geometry(type, fov, rgb ? width : 0, rgb ? height : 0, t.screen_bounds, &t.inv_tan);
    t.cos_total_width = (float)cos_total_width;
    // GonioPhotometricLight::power (goniometric.rs:105-113); ProjectionLight::power as pbrt-v3 has it (D89), for I = 1
    const double cone = type == PBRT_LIGHT_PROJECTION ? 2.0 * kPiD * (1.0 - cos_total_width) : 4.0 * kPiD;
    for (int k = 0; k < 3; ++k) {
        t.lookup_rgb[k] = (float)look[k];
        t.power_rgb[k] = (float)(look[k] * cone);
        if (!std::isfinite(t.power_rgb[k])) return "the map's power overflows float";
    }
    *out = std::move(t);
    return nullptr;
}

}  // namespace pb

// Context-free tables of a ProjectionLight's or GonioPhotometricLight's map (include/pbrt_hip.h)
extern "C" int pbrt_hip_light_map_tables(int32_t type, float fov, const float* rgb, int32_t width, int32_t height, int32_t* res_w,
                                         int32_t* res_h, float* level0_rgb, float lookup_rgb[3], float screen_bounds[4],
                                         float* cos_total_width, float power_rgb[3], const char** reason) try {
    auto refuse = [&](const char* why) {
        if (reason) *reason = why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (reason) *reason = "";
    if (!res_w || !res_h) return refuse("null pointer");
    pb::LightMapTables t;
    if (const char* why = pb::light_map_build(type, fov, rgb, width, height, &t)) return refuse(why);
    *res_w = t.w;
    *res_h = t.h;
    if (level0_rgb && !t.level0.empty()) std::memcpy(level0_rgb, t.level0.data(), t.level0.size() * sizeof(float));
    if (lookup_rgb) std::memcpy(lookup_rgb, t.lookup_rgb, sizeof(t.lookup_rgb));
    if (screen_bounds) std::memcpy(screen_bounds, t.screen_bounds, sizeof(t.screen_bounds));
    if (cos_total_width) *cos_total_width = t.cos_total_width;
    if (power_rgb) std::memcpy(power_rgb, t.power_rgb, sizeof(t.power_rgb));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// Context-free tables of InfiniteAreaLight::new for a caller's map (include/pbrt_hip.h)
extern "C" int pbrt_hip_envmap_tables(const float* rgb, int32_t width, int32_t height, const float L[3], int32_t* res_w,
                                      int32_t* res_h, float* level0_rgb, float* dist_func, float power_rgb[3],
                                      const char** reason) try {
    auto refuse = [&](const char* why) {
        if (reason) *reason = why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (reason) *reason = "";
    if (!rgb || !L || !res_w || !res_h) return refuse("null pointer");
    int rw, rh;
    if (const char* why = pb::envmap_resolution(width, height, &rw, &rh)) return refuse(why);
    if (!level0_rgb && !dist_func && !power_rgb) {  // the first of two calls: the sizes only
        if (const char* why = pb::check_texels(rgb, width, height, L)) return refuse(why);
        *res_w = rw;
        *res_h = rh;
        return PBRT_HIP_OK;
    }
    pb::EnvTables e;
    if (const char* why = pb::envmap_build(rgb, width, height, L, &e)) return refuse(why);
    *res_w = e.w;
    *res_h = e.h;
    if (level0_rgb) std::memcpy(level0_rgb, e.level0.data(), e.level0.size() * sizeof(float));
    if (dist_func) std::memcpy(dist_func, e.func.data(), e.func.size() * sizeof(float));
    if (power_rgb) std::memcpy(power_rgb, e.power_rgb, sizeof(e.power_rgb));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH
