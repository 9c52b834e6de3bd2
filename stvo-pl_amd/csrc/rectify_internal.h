// rectify_internal.h — the rectifier object shared by rectify_kernels.hip (8-bit grey images) and color_kernels.hip (colour images).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx_internal.h"
#include "frontend_layout.h"

struct stvo_rectify {
    stvo_ctx* ctx = nullptr;
    int B = 0, cols = 0, rows = 0, nquads = 0;
    stvo_rect_camera cam{};
    char* dev = nullptr;  // [side][nquads] int4 map1, then [side][nquads] uint2 map2 (dist = 1 only)
    stvo_detail::Staging io;  // staging of the host-buffer entry point: 2 B source images, 2 B destinations (lazy)
    int4* map1q(int side) const { return reinterpret_cast<int4*>(dev) + (size_t)side * nquads; }
    uint2* map2q(int side) const { return reinterpret_cast<uint2*>(dev + (size_t)2 * nquads * sizeof(int4)) + (size_t)side * nquads; }
};

namespace stvo_detail {

// [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
inline bool overlaps(const void* a, const void* b, size_t bytes) { return overlaps(a, bytes, b, bytes); }

}  // namespace stvo_detail
