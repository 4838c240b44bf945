// A patch of fur: a few hundred bent cylinder-type Curves (include/pbrt_hip.hpp: pbrt::Curve, src/shapes/curve.rs after pbrt-v3)
// standing on a quad under a distant light, triangles and curve segments in one BVHAccel. Prints what was traced and writes the
// film's raw float values, so that a test can set the same scene up through another binding of the same C ABI and compare the
// two films (tests/test_gpu_curves.py).
//
//   g++ -std=c++17 -Wall -Iinclude examples/render_fur_patch.cpp -o fur_patch -Lpbrt-rs_amd/pbrt_hip -lpbrt_hip -Wl,-rpath,$PWD/pbrt-rs_amd/pbrt_hip
//   ./fur_patch [film.raw [width height]]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pbrt_hip.hpp"

using namespace pbrt;

static const int kSide = 16;  // kSide x kSide hairs, two segments each

// the same small generator on both sides of the comparison: a 31-bit linear congruence, values in [0, 1)
static float next_unit(unsigned& state) {
    state = (state * 1103515245u + 12345u) & 0x7fffffffu;
    return (float)(state >> 7) / 16777216.0f;
}

int main(int argc, char** argv) try {
    const char* out = argc > 1 ? argv[1] : nullptr;
    const int width = argc > 3 ? std::atoi(argv[2]) : 32, height = argc > 3 ? std::atoi(argv[3]) : 32;
    TriangleMesh mesh;  // the skin: a quad in the plane y = 0, normal +y
    const float quad[4][3] = {{-1, 0, -1}, {-1, 0, 1}, {1, 0, 1}, {1, 0, -1}};
    for (const auto& v : quad) mesh.p.insert(mesh.p.end(), v, v + 3);
    for (int k : {0, 1, 2, 0, 2, 3}) mesh.vertex_indices.push_back(k);
    mesh.material = {0, 0};
    mesh.area_light = {-1, -1};
    const float kd[2][3] = {{0.6f, 0.5f, 0.4f}, {0.35f, 0.2f, 0.1f}};
    for (const auto& k : kd) {
        PbrtMaterial m{};
        m.type = PBRT_MAT_MATTE;
        m.kd[0] = k[0], m.kd[1] = k[1], m.kd[2] = k[2];
        m.eta = 1.0f;
        mesh.materials.push_back(m);
    }
    PbrtLight sun{};  // DistantLight: pos holds the direction from the surface to the light
    sun.type = PBRT_LIGHT_DISTANT;
    sun.L[0] = sun.L[1] = sun.L[2] = 3.0f;
    sun.prim = -1;
    sun.n_samples = 1;
    const float len = std::sqrt(0.3f * 0.3f + 1.0f + 0.2f * 0.2f);
    sun.pos[0] = 0.3f / len, sun.pos[1] = 1.0f / len, sun.pos[2] = -0.2f / len;
    mesh.lights.push_back(sun);

    auto ctx = std::make_shared<Context>(0);  // throws pbrt::Error without a GPU: there is no CPU fallback
    const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<Curve> fur;
    unsigned state = 12345u;
    for (int i = 0; i < kSide; ++i)
        for (int j = 0; j < kSide; ++j) {
            const float x = -0.9f + 1.8f * ((float)i + next_unit(state)) / (float)kSide, z = -0.9f + 1.8f * ((float)j + next_unit(state)) / (float)kSide;
            const float bx = 0.3f * (next_unit(state) - 0.5f), bz = 0.3f * (next_unit(state) - 0.5f), h = 0.4f + 0.3f * next_unit(state);
            const Point3f cp[4] = {{x, 0.0f, z}, {x + 0.2f * bx, 0.4f * h, z + 0.2f * bz}, {x + bx, 0.8f * h, z + bz}, {x + 2.0f * bx, h, z + 2.0f * bz}};
            for (const Curve& seg : Curve::segments(identity, nullptr, false, cp, 0.03f, 0.005f, CurveType::Cylinder, nullptr, 1, 1)) fur.push_back(seg);
        }
    auto aggregate = std::make_shared<BVHAccel>(ctx, mesh, std::vector<Shape>{}, fur);
    Scene scene(aggregate);
    const Point3f eye{0.0f, 1.6f, -2.6f}, look{0.0f, 0.3f, 0.0f};
    const Vector3f up{0, 1, 0};
    auto film = std::make_shared<Film>(width, height);
    auto camera = std::make_shared<PerspectiveCamera>(eye, look, up, 40.0f, film);
    PathIntegrator integrator(3, camera, RandomSampler(16, 7));
    integrator.render(scene);
    double xyz = 0.0;
    for (size_t i = 0; i < film->pixels.size(); i += 4) xyz += (double)film->pixels[i] + film->pixels[i + 1] + film->pixels[i + 2];
    std::printf("fur patch: %zu curve segments, %llu camera samples, %llu closest-hit + %llu shadow rays; film xyz %.9e\n", fur.size(),
                (unsigned long long)integrator.stats.camera_samples, (unsigned long long)integrator.stats.rays_closest,
                (unsigned long long)integrator.stats.rays_shadow, xyz);
    if (out) {
        std::FILE* f = std::fopen(out, "wb");
        if (!f || std::fwrite(film->pixels.data(), sizeof(float), film->pixels.size(), f) != film->pixels.size()) {
            std::fprintf(stderr, "cannot write %s\n", out);
            return 1;
        }
        std::fclose(f);
    }
    return 0;
} catch (const Error& e) {
    std::fprintf(stderr, "pbrt::Error (%d): %s\n", e.status, e.what());
    return 3;
}
