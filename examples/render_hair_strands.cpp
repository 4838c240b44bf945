// A lock of hair: a few dozen bent cylinder-type Curves with pbrt-v3's HairMaterial (include/pbrt_hip.hpp: pbrt::hair,
// Scene::set_hair_material) under a distant light and a constant environment. Writes a PNG and, for the test that sets the same
// scene up through another binding of the same C ABI (tests/test_gpu_hair.py), the film's raw float values.
//
//   g++ -std=c++17 -Wall -Iinclude examples/render_hair_strands.cpp -o hair_strands -Lpbrt-rs_amd/pbrt_hip -lpbrt_hip -Wl,-rpath,$PWD/pbrt-rs_amd/pbrt_hip
//   ./hair_strands [hair.png [width height [film.raw]]]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pbrt_hip.hpp"

using namespace pbrt;

static const int kStrands = 48;  // two segments each

// the same small generator on both sides of the comparison: a 31-bit linear congruence, values in [0, 1)
static float next_unit(unsigned& state) {
    state = (state * 1103515245u + 12345u) & 0x7fffffffu;
    return (float)(state >> 7) / 16777216.0f;
}

int main(int argc, char** argv) try {
    const char* png = argc > 1 ? argv[1] : "hair_strands.png";
    const int width = argc > 3 ? std::atoi(argv[2]) : 64, height = argc > 3 ? std::atoi(argv[3]) : 64;
    const char* raw = argc > 4 ? argv[4] : nullptr;
    TriangleMesh mesh;  // a scene needs a triangle: a speck far from everything, on row 0
    const float speck[3][3] = {{50.0f, 50.0f, 50.0f}, {50.001f, 50.0f, 50.0f}, {50.0f, 50.001f, 50.0f}};
    for (const auto& v : speck) mesh.p.insert(mesh.p.end(), v, v + 3);
    for (int k : {0, 1, 2}) mesh.vertex_indices.push_back(k);
    mesh.material = {0};
    mesh.area_light = {-1};
    for (int k = 0; k < 2; ++k) {  // row 1 becomes the hair row below
        PbrtMaterial m{};
        m.type = PBRT_MAT_MATTE;
        m.kd[0] = m.kd[1] = m.kd[2] = 0.5f;
        m.eta = 1.0f;
        mesh.materials.push_back(m);
    }
    PbrtLight sun{};  // DistantLight: pos holds the direction from the surface to the light
    sun.type = PBRT_LIGHT_DISTANT;
    sun.L[0] = sun.L[1] = sun.L[2] = 3.0f;
    sun.prim = -1;
    sun.n_samples = 1;
    const float len = std::sqrt(0.4f * 0.4f + 0.5f * 0.5f + 1.0f);
    sun.pos[0] = 0.4f / len, sun.pos[1] = 0.5f / len, sun.pos[2] = 1.0f / len;
    mesh.lights.push_back(sun);
    PbrtLight sky{};  // InfiniteAreaLight with a constant map
    sky.type = PBRT_LIGHT_INFINITE;
    sky.L[0] = 0.35f, sky.L[1] = 0.4f, sky.L[2] = 0.5f;
    sky.prim = -1;
    sky.n_samples = 1;
    mesh.lights.push_back(sky);

    auto ctx = std::make_shared<Context>(0);  // throws pbrt::Error without a GPU: there is no CPU fallback
    const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<Curve> strands;
    unsigned state = 2024u;
    for (int i = 0; i < kStrands; ++i) {
        const float x = -0.8f + 1.6f * ((float)i + next_unit(state)) / (float)kStrands, z = 0.3f * (next_unit(state) - 0.5f);
        const float sway = 0.5f * (next_unit(state) - 0.5f), curl = 0.4f * (next_unit(state) - 0.5f);
        const Point3f cp[4] = {{x, 0.9f, z}, {x + 0.3f * sway, 0.3f, z + curl}, {x + sway, -0.3f, z - curl}, {x + 1.5f * sway, -0.9f, z + 0.5f * curl}};
        for (const Curve& seg : Curve::segments(identity, nullptr, false, cp, 0.03f, 0.012f, CurveType::Cylinder, nullptr, 1, 1)) strands.push_back(seg);
    }
    auto aggregate = std::make_shared<BVHAccel>(ctx, mesh, std::vector<Shape>{}, strands);
    Scene scene(aggregate);
    scene.set_hair_material(1, hair(nullptr, nullptr, 0.8f, 0.2f));  // light brown; eta 1.55, beta_m = beta_n = 0.3, alpha 2
    const Point3f eye{0.0f, 0.0f, 3.2f}, look{0.0f, 0.0f, 0.0f};
    const Vector3f up{0, 1, 0};
    auto film = std::make_shared<Film>(width, height);
    auto camera = std::make_shared<PerspectiveCamera>(eye, look, up, 36.0f, film);
    PathIntegrator integrator(5, camera, RandomSampler(16, 7));
    integrator.render(scene);
    film->write_image(png);
    double xyz = 0.0;
    for (size_t i = 0; i < film->pixels.size(); i += 4) xyz += (double)film->pixels[i] + film->pixels[i + 1] + film->pixels[i + 2];
    std::printf("hair strands: %zu curve segments, %llu camera samples, %llu closest-hit + %llu shadow rays; film xyz %.9e; wrote %s\n",
                strands.size(), (unsigned long long)integrator.stats.camera_samples, (unsigned long long)integrator.stats.rays_closest,
                (unsigned long long)integrator.stats.rays_shadow, xyz, png);
    if (raw) {
        std::FILE* f = std::fopen(raw, "wb");
        if (!f || std::fwrite(film->pixels.data(), sizeof(float), film->pixels.size(), f) != film->pixels.size()) {
            std::fprintf(stderr, "cannot write %s\n", raw);
            return 1;
        }
        std::fclose(f);
    }
    return 0;
} catch (const Error& e) {
    std::fprintf(stderr, "pbrt::Error (%d): %s\n", e.status, e.what());
    return 3;
}
