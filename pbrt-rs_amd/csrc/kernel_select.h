// kernel_select.h — which kernel a launch runs, decided in one place (host only; no kernel lives here).
//
// Traversal: choose_trace() reads the scene and the context once and dispatch() turns the answer into compile-time constants
// for a caller-supplied generic lambda; wavefront_render (render.hip) launches k_trace* from it, launch_batch (pbrt_hip.hip)
// k_intersect_batch*. Shading: scene_needs() states what the scene's tables ask of the shading kernels and the three lookups
// below return the instantiation from constexpr tables; they name the kernels of wavefront.h, so only a translation unit that
// has included it (and says so with PB_SELECT_SHADING_KERNELS) sees them.
#pragma once
#include <type_traits>

#include "scene.h"
#include "trace_wide.h"
#include "trace_wide_packet.h"

namespace pb {

// ---- traversal ----
// Moving: a two-level scene with moving instances (trace_persistent's MOV builds over the binary records; never wide —
// the scene carries no wide records — and never stackless, which refuses every two-level scene)
// Curves: a one-level scene with curve segments (trace_persistent's CRV builds: the shapes' with the curve test beside them)
enum class TraceKind { Stackless, Wide, Shapes, Spheres, Binary, Moving, Curves };
struct TraceChoice {
    TraceKind kind;
    int inst;    // trace_persistent.h: INST (0 single level, 1 instances of one aggregate, 2 general top level)
    bool count;  // the COUNT instantiation: count_traversal == 1 for the binary families, == 2 for the wide one
    bool ok;     // false: PBRT_TRAVERSAL_STACKLESS does not apply to this scene (last_error says why); launch nothing
};

inline TraceChoice choose_trace(const PbrtHipScene* s) {
    const PbrtHipContext* ctx = s->ctx;
    TraceChoice c{TraceKind::Binary, s->d.bvh.instanced ? (s->d.bvh.general_top ? 2 : 1) : 0, ctx->count_traversal == 1, true};
    if (ctx->traversal == PBRT_TRAVERSAL_STACKLESS) {
        c.kind = TraceKind::Stackless;  // single level, no counting: stackless_applies refuses everything else
        c.ok = stackless_applies(s);
    } else if (s->has_wide && ctx->count_traversal != 1 && ctx->traversal == PBRT_TRAVERSAL_AUTO) {
        c.kind = TraceKind::Wide;
        c.count = ctx->count_traversal == 2;
    } else if (s->d.bvh.has_spheres) {  // single-level scenes only (checked at creation); 2: general quadric shapes
        c.kind = s->d.bvh.has_spheres == 2 ? TraceKind::Shapes : TraceKind::Spheres;
        if (s->d.curves) c.kind = TraceKind::Curves;  // has_spheres == 2 there, with or without shapes
    } else if (s->moving) {
        c.kind = TraceKind::Moving;
    }
    return c;
}

// grid of the wide kernels' <COUNT, INST> instantiation (their launch bounds: trace_wide.h)
template <bool COUNT, int INST>
inline int wide_grid(const PbrtHipScene* s) {
    return persistent_grid(s, (COUNT || INST) ? PB_WIDE_INST_WAVES : PB_WIDE_WAVES, wide_stack_lds(INST), wide_world_lds_bytes(INST));
}

// The camera wavefront as one-pixel wave packets (trace_wide_packet.h: k_trace_wide_packet instead of k_trace_wide<false, 0>): the
// wide records of a one-level scene, no counting, a wave of paths = the 64 samples of one pixel (PassParams::group_shift == 6), a
// tree whose walk fits the wave's stack, and pbrt_hip_context_set_camera_packets has not turned it off. Everything else —
// later wavefronts, two-level, sphere and moving scenes, pbrt_hip_li batches, counting runs — launches what it always did.
inline bool use_camera_packets(const PbrtHipScene* s, const TraceChoice& c, int wavefront, int group_shift) {
    return wavefront == 0 && c.kind == TraceKind::Wide && c.inst == 0 && !c.count && group_shift == 6 && s->ctx->camera_packets == 0 &&
           s->wide_stack_need <= kPacketStack;
}
inline int packet_grid(const PbrtHipScene* s) { return s->ctx->n_cus * PB_PACKET_WAVES; }  // 256 bytes of LDS per wave: the registers set it

template <TraceKind K>
using TraceKindC = std::integral_constant<TraceKind, K>;

// Calls f(TraceKindC<kind>, std::bool_constant<COUNT>, std::integral_constant<int, INST>) for the choice. Only the combinations
// the kernels exist for are ever formed: shapes and spheres are single level, the stackless walk has neither COUNT nor INST,
// moving scenes have two levels (INST 1 or 2).
template <class F>
inline void dispatch(const TraceChoice& c, F&& f) {
    auto with_count = [&](auto kind, auto inst) {
        if (c.count)
            f(kind, std::true_type{}, inst);
        else
            f(kind, std::false_type{}, inst);
    };
    auto with_inst = [&](auto kind) {
        if (c.inst == 2)
            with_count(kind, std::integral_constant<int, 2>{});
        else if (c.inst == 1)
            with_count(kind, std::integral_constant<int, 1>{});
        else
            with_count(kind, std::integral_constant<int, 0>{});
    };
    switch (c.kind) {
        case TraceKind::Stackless: f(TraceKindC<TraceKind::Stackless>{}, std::false_type{}, std::integral_constant<int, 0>{}); break;
        case TraceKind::Wide: with_inst(TraceKindC<TraceKind::Wide>{}); break;
        case TraceKind::Shapes: with_count(TraceKindC<TraceKind::Shapes>{}, std::integral_constant<int, 0>{}); break;
        case TraceKind::Spheres: with_count(TraceKindC<TraceKind::Spheres>{}, std::integral_constant<int, 0>{}); break;
        case TraceKind::Binary: with_inst(TraceKindC<TraceKind::Binary>{}); break;
        case TraceKind::Moving:
            if (c.inst == 2)
                with_count(TraceKindC<TraceKind::Moving>{}, std::integral_constant<int, 2>{});
            else
                with_count(TraceKindC<TraceKind::Moving>{}, std::integral_constant<int, 1>{});
            break;
        case TraceKind::Curves: with_count(TraceKindC<TraceKind::Curves>{}, std::integral_constant<int, 0>{}); break;
    }
}

// ---- shading ----
// What the scene's tables ask of a shading kernel. Precedence, as the instantiations are built: general quadric shapes win over
// everything (their builds carry the level-3 BSDF set and the map lights), a projection or goniometric light wins over the
// material level (the map-light builds are level 3 too), and AO reads neither a BSDF nor a light.
struct SceneNeeds {
    bool shapes;      // bvh.has_spheres == 2
    bool light_maps;  // a projection or goniometric light in the table
    int level;        // 0 matte / mirror / glass, 1 plastic or metal, 2 a row of pbrt_hip_scene_set_material, 3 a Disney row
    bool lobes;       // a row of pbrt_hip_scene_set_lobe_material: the lobe-list builds (never with shapes or light_maps: the setter refuses)
    bool moving;      // moving instances: the builds that interpolate the instance at the path's time (never with shapes, light_maps
                      // or lobes: creation and the setters refuse)
    bool curves;      // curve segments (DevSceneData::curves): the builds that rebuild a curve's surface from the ray (with shapes set:
                      // they are the builds for shapes with that added)
    bool hair;        // a row of pbrt_hip_scene_set_hair_material (only in a scene with curves: the setter refuses): the hair builds
    int column() const { return shapes ? 0 : light_maps ? 1 : 5 - level; }  // of the tables below: in that precedence, most general first
};
inline SceneNeeds scene_needs(const PbrtHipScene* s) {
    return SceneNeeds{s->d.bvh.has_spheres == 2, s->light_maps, s->disney ? 3 : s->bxdfs ? 2 : s->glossy ? 1 : 0, s->lobes, s->moving, s->d.curves != nullptr, s->hair};
}

#ifdef PB_SELECT_SHADING_KERNELS
using DirectKernel = void (*)(ShadeConsts, PathState, DirectState, Queues, Queues, PassParams, TileList, uint32_t);
using PathKernel = void (*)(ShadeConsts, PathState, Queues, Queues, PassParams, TileList, uint32_t, const uint32_t*);
using SpatialKernel = void (*)(ShadeConsts, float*);
}  // namespace pb
#include "curve_kernels.h"
#include "hair_kernels.h"
namespace pb {
// The tables list every instantiation the library holds, once. Their initialisers are also where the compiler first meets each
// instantiation, and the code it generates for some of the kernels depends on that order (profiles/r11_render_driver.txt): the
// rows and columns below keep the order the kernels have always been named in.

// The lobe-list builds have tables of their own at the END of this file, so that every older instantiation is met first.
inline DirectKernel lobe_direct_kernel(bool whitted);
inline PathKernel lobe_path_kernel(bool bin);
// ... and behind them those of the builds for moving instances
inline DirectKernel moving_direct_kernel(int integrator);
inline PathKernel moving_path_kernel(bool bin);
// ... and the builds for curves — k_shade_direct<MODE, 3 + kDirectCurves>, the AO build, k_shade_curves<BIN> and k_trace_curves<COUNT> —
// are instantiated in a translation unit of their own (curve_kernels.hip). That goes one step further than a table at the end of
// this file: the unit that holds every older kernel meets none of them, so it compiles, and its code object is laid out, as before
// curves existed (profiles/curve_resource_usage.txt, profiles/curve_bench.txt). (The SpatialLightDistribution tables sample lights
// only, and a curve carries none: the build for shapes serves.)
// curve_direct_kernel, curve_path_kernel, launch_trace_curves: curve_kernels.h
// ... and so are the builds for a curve scene whose table holds a hair row, k_shade_direct<MODE, 3 + kDirectCurves + kDirectHair> and
// k_shade_hair<BIN>, in hair_kernels.hip (profiles/hair_resource_usage.txt). AO reads no BSDF and traversal reads no material: the
// curve builds serve. hair_direct_kernel, hair_path_kernel: hair_kernels.h

// the build of the SpatialLightDistribution tables (wf_lights.h)
inline SpatialKernel spatial_tables_kernel(const SceneNeeds& n) {
    static constexpr SpatialKernel table[3] = {k_spatial_light_tables_shapes, k_spatial_light_tables_maps, k_spatial_light_tables};
    return table[n.shapes ? 0 : n.light_maps ? 1 : 2];
}

// k_shade_direct<MODE, LEVEL_SHP> (wf_direct.h) for DirectLighting, Whitted or AO
inline DirectKernel direct_kernel(const SceneNeeds& n, int integrator) {
    constexpr int D = PBRT_INTEGRATOR_DIRECT, W = PBRT_INTEGRATOR_WHITTED, AO = PBRT_INTEGRATOR_AO;
    static constexpr DirectKernel lit[6][2] = {{k_shade_direct<D, 3 + kDirectShapes>, k_shade_direct<W, 3 + kDirectShapes>},
                                               {k_shade_direct<D, 3 + kDirectMapLights>, k_shade_direct<W, 3 + kDirectMapLights>},
                                               {k_shade_direct<D, 3>, k_shade_direct<W, 3>},
                                               {k_shade_direct<D, 2>, k_shade_direct<W, 2>},
                                               {k_shade_direct<D, 1>, k_shade_direct<W, 1>},
                                               {k_shade_direct<D, 0>, k_shade_direct<W, 0>}};
    static constexpr DirectKernel ao[2] = {k_shade_direct<AO, kDirectShapes>, k_shade_direct<AO, 0>};
    if (n.curves && n.hair && (integrator == D || integrator == W)) return hair_direct_kernel(integrator == W);
    if (n.curves) return curve_direct_kernel(integrator);
    if (n.moving) return moving_direct_kernel(integrator);
    if (n.lobes && (integrator == D || integrator == W)) return lobe_direct_kernel(integrator == W);
    if (integrator == D || integrator == W) return lit[n.column()][integrator == W];
    return ao[n.shapes ? 0 : 1];
}

// k_shade_shapes<BIN> / k_shade_maps<BIN> / k_shade<BIN, LEVEL> (wf_path.h) for the path integrator
inline PathKernel path_kernel(const SceneNeeds& n, bool bin) {
    static constexpr PathKernel table[2][6] = {
        {k_shade_shapes<true>, k_shade_maps<true>, k_shade<true, 3>, k_shade<true, 2>, k_shade<true, 1>, k_shade<true, 0>},
        {k_shade_shapes<false>, k_shade_maps<false>, k_shade<false, 3>, k_shade<false, 2>, k_shade<false, 1>, k_shade<false, 0>}};
    if (n.curves && n.hair) return hair_path_kernel(bin);
    if (n.curves) return curve_path_kernel(bin);
    if (n.moving) return moving_path_kernel(bin);
    if (n.lobes) return lobe_path_kernel(bin);
    return table[bin ? 0 : 1][n.column()];
}

// k_shade_direct<MODE, 3 + kDirectLobes> and k_shade_lobes<BIN>: scenes that hold a lobe row
inline DirectKernel lobe_direct_kernel(bool whitted) {
    static constexpr DirectKernel table[2] = {k_shade_direct<PBRT_INTEGRATOR_DIRECT, 3 + kDirectLobes>,
                                              k_shade_direct<PBRT_INTEGRATOR_WHITTED, 3 + kDirectLobes>};
    return table[whitted ? 1 : 0];
}
inline PathKernel lobe_path_kernel(bool bin) {
    static constexpr PathKernel table[2] = {k_shade_lobes<true>, k_shade_lobes<false>};
    return table[bin ? 0 : 1];
}

// k_shade_direct<MODE, 3 + kDirectMoving>, the AO build and k_shade_moving<BIN>: scenes with moving instances
inline DirectKernel moving_direct_kernel(int integrator) {
    static constexpr DirectKernel table[3] = {k_shade_direct<PBRT_INTEGRATOR_DIRECT, 3 + kDirectMoving>,
                                              k_shade_direct<PBRT_INTEGRATOR_WHITTED, 3 + kDirectMoving>,
                                              k_shade_direct<PBRT_INTEGRATOR_AO, kDirectMoving>};
    return table[integrator == PBRT_INTEGRATOR_DIRECT ? 0 : integrator == PBRT_INTEGRATOR_WHITTED ? 1 : 2];
}
inline PathKernel moving_path_kernel(bool bin) {
    static constexpr PathKernel table[2] = {k_shade_moving<true>, k_shade_moving<false>};
    return table[bin ? 0 : 1];
}

// ---- camera rays ----
// The generator by a two-bit key: bit 0 the scene has moving instances, bit 1 camera_to_world is animated. With a static camera
// the kernels are k_generate / k_generate_moving with the arguments they always had; an animated camera has one build for both
// kinds of scene, which also takes the camera's DevMotion row (wf_camera_motion.h). Behind every older table, as above.
using GenerateKernel = void (*)(PathState, Queues, PassParams, DevCamera, TileList);
using GenerateCameraKernel = void (*)(PathState, Queues, PassParams, DevCamera, DevMotion, TileList);
constexpr int kGenerateCameraAnimated = 2;
inline int generate_key(bool scene_moving, bool camera_animated) { return (scene_moving ? 1 : 0) | (camera_animated ? kGenerateCameraAnimated : 0); }
inline GenerateKernel generate_kernel(int key) {
    static constexpr GenerateKernel table[2] = {k_generate, k_generate_moving};
    return table[key & 1];
}
inline GenerateCameraKernel generate_camera_kernel(int key) {
    static constexpr GenerateCameraKernel table[2] = {k_generate_moving_camera, k_generate_moving_camera};
    return table[key & 1];
}

#endif  // PB_SELECT_SHADING_KERNELS

}  // namespace pb
