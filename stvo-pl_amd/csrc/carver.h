// carver.h — the carver every device allocation of the project is cut with (seq_layout.h: the pipeline, frontend_layout.h: the
// front-end objects), and the one vector type their layouts name.  Host-pure: g++ alone compiles it; under hipcc float4 is HIP's.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>
#else
struct alignas(16) float4 { float x, y, z, w; };
#endif

namespace stvo {

// Cuts one allocation into buffers of 256-byte-aligned sizes.  take<T>(count) is where a buffer is named: it returns the pointer to store.
// A layout function runs twice — on a null base, where only `off` (the bytes the allocation needs) matters and the pointers it stores
// are bare offsets, and on the allocation.  A conditional buffer is `cond ? c.take<T>(n) : nullptr`: nothing is cut for it.
struct Carver {
    uintptr_t base = 0;
    size_t off = 0;  // bytes cut so far: what the next take returns, and at the end the size of the allocation
    explicit Carver(const void* b = nullptr) : base(reinterpret_cast<uintptr_t>(b)) {}
    template <typename T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

}  // namespace stvo
