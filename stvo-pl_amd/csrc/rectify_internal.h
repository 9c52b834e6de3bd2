// rectify_internal.h — the rectifier object and the host-side decisions shared by rectify_kernels.hip (the object, 8-bit grey images),
// color_kernels.hip (the uniform remap kernel, colour images) and rectify_bank.hip (mixed cameras): the argument checks on byte ranges
// and the grey weight sets.  The pixel arithmetic is in rectify_px.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx_internal.h"
#include "frontend_layout.h"
#include "rectify_px.h"

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

// Four ranges of `bytes` each: neither destination shares a byte with a source or with the other destination.
inline bool stereo_ranges_ok(const void* dst_l, const void* dst_r, const void* src_l, const void* src_r, size_t bytes) {
    return !(overlaps(dst_l, src_l, bytes) || overlaps(dst_l, src_r, bytes) || overlaps(dst_r, src_l, bytes) || overlaps(dst_r, src_r, bytes) ||
             overlaps(dst_l, dst_r, bytes));
}

// np grey planes of px bytes each: none shares a byte with a source (sb bytes each) or with another plane.
inline bool gray_planes_ok(const uint8_t* const* planes, int np, size_t px, const void* src_l, const void* src_r, size_t sb) {
    for (int a = 0; a < np; ++a) {
        if (overlaps(planes[a], px, src_l, sb) || overlaps(planes[a], px, src_r, sb)) return false;
        for (int b = a + 1; b < np; ++b)
            if (overlaps(planes[a], planes[b], px)) return false;
    }
    return true;
}

// The weights of plane A for a channel order and a weight set (rectify_px.h); false for any other order or set.
inline bool gray_weights(int order, int weights, GrayWeights* w) {
    uint32_t blue, green, red;
    if (weights == STVO_GRAY_Q14) {
        blue = 1868u; green = 9617u; red = 4899u; w->shift = 14u;
    } else if (weights == STVO_GRAY_Q15) {
        blue = 3735u; green = 19235u; red = 9798u; w->shift = 15u;
    } else
        return false;
    if (order != STVO_ORDER_BGR && order != STVO_ORDER_RGB) return false;
    w->w0 = order == STVO_ORDER_BGR ? blue : red;
    w->w1 = green;
    w->w2 = order == STVO_ORDER_BGR ? red : blue;
    w->rnd = 1u << (w->shift - 1u);
    return true;
}

// The arguments of a stereo image call on n pairs of ch-channel images of the rectifier's size.
inline int check_images(const stvo_rectify* r, int n, int ch, const uint8_t* src_l, const uint8_t* src_r, const uint8_t* dst_l,
                        const uint8_t* dst_r) {
    if (!r || !src_l || !src_r || !dst_l || !dst_r || n <= 0 || n > r->B) return STVO_ERR_INVALID_ARG;
    if (!stereo_ranges_ok(dst_l, dst_r, src_l, src_r, (size_t)n * r->cols * r->rows * ch)) return STVO_ERR_INVALID_ARG;
    return STVO_OK;
}

// The uniform remap (color_kernels.hip) of n pairs of ch = 1, 3 or 4 channels on the rectifier's context; dist = 0 copies, as the
// reference does.
int launch_remap(stvo_rectify* r, int n, int ch, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r);

}  // namespace stvo_detail
