// A camera pan: one matte unit quad under a distant light, seen by an OrthographicCamera whose camera_to_world is an
// AnimatedTransform (src/core/camera.rs:80-115) that translates along x while the shutter is open. The quad is static, so the
// scene keeps its one-level traversal; only the ray generator sees the motion. Every column of the film is the fraction of the
// shutter during which the quad covers it: a trapezoid (tests/test_gpu_camera_motion.py renders the same job through the Python
// binding and compares the two films).
//
//   g++ -std=c++17 -Wall -Iinclude examples/render_camera_pan.cpp -o camera_pan -Lpbrt-rs_amd/pbrt_hip -lpbrt_hip -Wl,-rpath,$PWD/pbrt-rs_amd/pbrt_hip
//   ./camera_pan [film.raw [resolution spp [tile_rank tile_world]]]
#include <cstdio>
#include <cstdlib>

#include "pbrt_hip.hpp"

using namespace pbrt;

int main(int argc, char** argv) try {
    const char* out = argc > 1 ? argv[1] : nullptr;
    const int res = argc > 3 ? std::atoi(argv[2]) : 64, spp = argc > 3 ? std::atoi(argv[3]) : 64;
    const int tile_rank = argc > 5 ? std::atoi(argv[4]) : 0, tile_world = argc > 5 ? std::atoi(argv[5]) : 1;
    const float shift = 1.5f, x0 = 0.77f, y0 = 0.02f;  // the pan, and the centre of the quad

    TriangleMesh mesh;
    mesh.p = {x0 - 0.5f, y0 - 0.5f, 0, x0 + 0.5f, y0 - 0.5f, 0, x0 + 0.5f, y0 + 0.5f, 0, x0 - 0.5f, y0 + 0.5f, 0};
    mesh.vertex_indices = {0, 1, 2, 0, 2, 3};
    mesh.material = {0, 0};
    mesh.area_light = {-1, -1};
    PbrtMaterial matte{};
    matte.type = PBRT_MAT_MATTE;
    matte.kd[0] = matte.kd[1] = matte.kd[2] = 0.5f;
    matte.eta = 1.0f;
    mesh.materials.push_back(matte);
    PbrtLight sun{};  // DistantLight straight on: w_light = +z
    sun.type = PBRT_LIGHT_DISTANT;
    sun.L[0] = sun.L[1] = sun.L[2] = 3.0f;
    sun.prim = -1;
    sun.n_samples = 1;
    sun.pos[2] = 1.0f;
    mesh.lights.push_back(sun);

    auto ctx = std::make_shared<Context>(0);  // throws pbrt::Error without a GPU: there is no CPU fallback
    auto aggregate = std::make_shared<BVHAccel>(ctx, mesh);
    Scene scene(aggregate);

    auto film = std::make_shared<Film>(res, res);
    auto camera = std::make_shared<OrthographicCamera>(Point3f{0, 0, 5}, Point3f{0, 0, 0}, Vector3f{0, 1, 0}, 2.0f, film);
    // camera_to_world over the shutter [0, 1]: the look_at matrix of the constructor at time 0, the same moved by `shift` at time 1
    AnimatedTransform pan{};
    for (int k = 0; k < 16; ++k) pan.start_transform[k] = pan.end_transform[k] = camera->cam.camera_to_world[k];
    pan.end_transform[3] += shift;
    pan.start_time = 0.0f, pan.end_time = 1.0f;
    camera->set_camera_to_world(pan);

    DirectLightingIntegrator integrator(LightStrategy::UniformSampleAll, 1, camera, RandomSampler(spp, 3));
    integrator.tile_rank = tile_rank, integrator.tile_world = tile_world;
    integrator.render(scene);
    double xyz = 0.0;
    for (size_t i = 0; i < film->pixels.size(); i += 4) xyz += (double)film->pixels[i] + film->pixels[i + 1] + film->pixels[i + 2];
    std::printf("camera pan: %llu camera samples, %llu closest-hit + %llu shadow rays; film xyz %.9e\n",
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
