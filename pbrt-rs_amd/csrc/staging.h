// staging.h — device scratch of an entry point that takes host pointers in and hands host pointers out: allocate, copy in, run, copy
// out, free. Failures leave their reason in the context's last_error (hip_ok); which return code a failure maps to is the entry
// point's own business. The blocks are freed on scope exit unless the context is lost: after a deadline an abandoned kernel may
// still touch them and hipFree would wait for the device, so they stay.
#pragma once
#include <vector>

#include "scene.h"

namespace pb {

struct Staging {
    PbrtHipContext* ctx;
    std::vector<void*> blocks;
    bool failed = false;  // an allocation failed: the ones after it are not tried
    explicit Staging(PbrtHipContext* c) : ctx(c) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() {
        if (ctx->lost) return;
        for (void* p : blocks) (void)hipFree(p);
    }
    template <class T>
    T* alloc(size_t n) {  // null (and `failed`): no memory, or a device error; last_error says which
        void* p = nullptr;
        if (failed || !hip_ok(ctx, hipMalloc(&p, n * sizeof(T)), "hipMalloc")) {
            failed = true;
            return nullptr;
        }
        blocks.push_back(p);
        return (T*)p;
    }
    void adopt(void* p) {  // a block somebody else allocated
        if (p) blocks.push_back(p);
    }
    // blocking copies, or (async) copies queued on the context's stream
    bool upload(void* dst, const void* src, size_t bytes, bool async = false) const {
        return hip_ok(ctx, async ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice),
                      "H2D");
    }
    bool download(void* dst, const void* src, size_t bytes, bool async = false, const char* what = "D2H") const {
        return hip_ok(ctx, async ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost),
                      what);
    }
};

}  // namespace pb
