// abi_guard.h — nothing is thrown across the C ABI ("int status returns, no exceptions or panics across the
// boundary"; the reference's own error channel is panic!, which a C caller cannot catch either). Every status-returning entry
// point is a function-try-block ending in PB_ABI_CATCH: a host allocation that fails (std::vector / std::string growing while a
// tree is built or a scene re-laid out) becomes PBRT_HIP_ERR_OOM, anything else PBRT_HIP_ERR_INVALID. Locks and device buffers
// are RAII objects: unwinding releases them.
#pragma once
#include <cstddef>
#include <new>

#include "../../include/pbrt_hip.h"

// the layouts of the hair row's structs, as every binding restates them (tests/test_hair_model.py)
static_assert(sizeof(PbrtHairDesc) == 52 && offsetof(PbrtHairDesc, absorption) == 0 && offsetof(PbrtHairDesc, sigma_a) == 4 &&
                  offsetof(PbrtHairDesc, color) == 16 && offsetof(PbrtHairDesc, eumelanin) == 28 && offsetof(PbrtHairDesc, pheomelanin) == 32 &&
                  offsetof(PbrtHairDesc, eta) == 36 && offsetof(PbrtHairDesc, beta_m) == 40 && offsetof(PbrtHairDesc, beta_n) == 44 &&
                  offsetof(PbrtHairDesc, alpha) == 48,
              "PbrtHairDesc layout");
static_assert(sizeof(PbrtHairTables) == 60 && offsetof(PbrtHairTables, sigma_a) == 0 && offsetof(PbrtHairTables, eta) == 12 &&
                  offsetof(PbrtHairTables, v) == 16 && offsetof(PbrtHairTables, s) == 32 && offsetof(PbrtHairTables, sin2k) == 36 &&
                  offsetof(PbrtHairTables, cos2k) == 48,
              "PbrtHairTables layout");

#define PB_ABI_CATCH                                  \
    catch (const std::bad_alloc&) {                   \
        return PBRT_HIP_ERR_OOM;                      \
    }                                                 \
    catch (...) {                                     \
        return PBRT_HIP_ERR_INVALID;                  \
    }
