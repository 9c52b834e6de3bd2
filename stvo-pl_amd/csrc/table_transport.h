// table_transport.h — how a front-end object's small per-image table reaches the device (stvo_lsd_set_image_sizes,
// stvo_lbd_set_image_sizes): formed on the host in a pinned block and copied on the context's stream, so it arrives behind the calls
// already enqueued (which read the previous contents) and in front of the next one; nothing waits for it.  Two pinned blocks are used
// alternately, and one is written again only after the copy that last read it (two calls ago) has completed — long since, unless
// nothing has synchronised in between.  Nothing exists until the first call; the device table is an allocation of its own.
#pragma once
#include "ctx_internal.h"

namespace stvo_detail {

struct TableTransport {
    char* dev = nullptr;
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int next = 0;

    // the pinned block to form the next table in (`capacity` bytes: the largest table of the object, the same at every call), or
    // nullptr with the error in ctx
    char* begin(stvo_ctx* ctx, size_t capacity) {
        const size_t span = (capacity + 255) & ~size_t(255);
        if (!dev && !hip_ok(ctx, hipMalloc((void**)&dev, span), "hipMalloc size table")) return nullptr;
        if (!stage[0]) {
            if (!hip_ok(ctx, hipHostMalloc((void**)&stage[0], 2 * span, hipHostMallocDefault), "hipHostMalloc size table")) return nullptr;
            stage[1] = stage[0] + span;
        }
        for (auto& e : ev)
            if (!e && !hip_ok(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate size table")) return nullptr;
        if (busy[next]) {
            if (!hip_ok(ctx, hipEventSynchronize(ev[next]), "hipEventSynchronize size table")) return nullptr;
            busy[next] = false;
        }
        return stage[next];
    }
    // the first `bytes` of the block begin() returned, to the device table
    int send(stvo_ctx* ctx, size_t bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(dev, stage[next], bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[next], ctx->stream));
        busy[next] = true;
        next ^= 1;
        return STVO_OK;
    }
    void destroy() {
        if (dev) (void)hipFree(dev);
        if (stage[0]) (void)hipHostFree(stage[0]);  // (one allocation for both blocks)
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace stvo_detail
