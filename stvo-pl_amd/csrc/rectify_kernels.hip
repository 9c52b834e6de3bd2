// rectify_kernels.hip — stereo rectification of raw 8-bit images (stvo_rectify_*): the cv::remap(INTER_LINEAR, BORDER_CONSTANT 0)
// that PinholeStereoCamera::rectifyImagesLR applies to every pair (src/pinholeStereoCamera.cpp:196-208), bit for bit.
//
//   rectify_remap_kernel  one thread = 4 consecutive output pixels of one side (the pixel index runs over rows * cols, so a quad may
//                         straddle two rows): one 16-B load of map1 (4 x (int16 x, int16 y)) and one 8-B load of map2 (4 x uint16),
//                         then a loop over the images of that side in this block's chunk with the map held in registers; per image
//                         4 taps per pixel and one 4-B store (byte stores where the quad is not dword-aligned in the image or runs
//                         past its end).  blockIdx.y = image chunk, blockIdx.z = side (0 left, 1 right).
//
// Arithmetic (OpenCV's fixed-point bilinear: initInterTab2D(INTER_LINEAR, fixpt = true) gives, for fractions ax, ay in 1/32 px, the
// weights (32-ax)(32-ay)*32, ax(32-ay)*32, (32-ax)ay*32, ax*ay*32 — they sum to 32768, so the table needs no correction — and
// remapBilinear rounds (sum S*w + 2^14) >> 15).  Since every weight is 32 times an integer, that equals (X + 512) >> 10 with
// X = (32-ay)((32-ax)S00 + ax S01) + ay((32-ax)S10 + ax S11) < 2^18: 24-bit multiplies, no table.  A tap outside the source
// reads 0 (BORDER_CONSTANT: borderInterpolate -> -1 -> cval; a pixel whose taps are all outside gets cval, which is the same 0).
//
// The device copy of map2 carries bit 15 = "all four taps inside the source" (the host sets it once, when the maps are uploaded),
// so the common path has no per-tap tests.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "ctx_internal.h"
#include "rectify_internal.h"

namespace {

constexpr int RECT_BLOCK = 256;
constexpr uint32_t INSIDE = 0x8000u;

__device__ __forceinline__ uint32_t tap(const uint8_t* __restrict__ S, int x, int y, int cols, int rows) {
    return ((unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows) ? (uint32_t)S[(size_t)y * cols + x] : 0u;
}

__device__ __forceinline__ uint32_t blend(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, uint32_t m2) {
    const uint32_t ax = m2 & 31u, ay = (m2 >> 5) & 31u;
    const uint32_t top = __umul24(32u - ax, s00) + __umul24(ax, s01);
    const uint32_t bot = __umul24(32u - ax, s10) + __umul24(ax, s11);
    return (__umul24(32u - ay, top) + __umul24(ay, bot) + 512u) >> 10;
}

// map1q / map2q: one side's maps padded to whole quads.  src / dst: this side's first image; images npx bytes apart.
__global__ void __launch_bounds__(RECT_BLOCK) rectify_remap_kernel(const int4* __restrict__ map1q_l, const uint2* __restrict__ map2q_l,
                                                                  const int4* __restrict__ map1q_r, const uint2* __restrict__ map2q_r,
                                                                  const uint8_t* __restrict__ src_l, const uint8_t* __restrict__ src_r,
                                                                  uint8_t* __restrict__ dst_l, uint8_t* __restrict__ dst_r, int n,
                                                                  int per_chunk, int cols, int rows, int nquads) {
    const int q = blockIdx.x * RECT_BLOCK + threadIdx.x;
    if (q >= nquads) return;
    const bool right = blockIdx.z != 0;
    const int i0 = blockIdx.y * per_chunk;
    const int i1 = min(n, i0 + per_chunk);
    if (i0 >= i1) return;
    const int4 m1 = (right ? map1q_r : map1q_l)[q];
    const uint2 m2v = (right ? map2q_r : map2q_l)[q];
    const uint8_t* src = right ? src_r : src_l;
    uint8_t* dst = right ? dst_r : dst_l;
    const size_t npx = (size_t)cols * rows;
    const size_t p0 = (size_t)q * 4;
    const int m1s[4] = {m1.x, m1.y, m1.z, m1.w};
    const uint32_t m2s[4] = {m2v.x & 0xffffu, m2v.x >> 16, m2v.y & 0xffffu, m2v.y >> 16};
    int off[4];  // source offset of the top-left tap (valid where the pixel is inside)
    bool all_inside = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = (int)(int16_t)(m1s[k] & 0xffff), y = m1s[k] >> 16;
        off[k] = y * cols + x;
        all_inside = all_inside && (m2s[k] & INSIDE);
    }
    const bool full = p0 + 4 <= npx;
    for (int i = i0; i < i1; ++i) {
        const uint8_t* S = src + (size_t)i * npx;
        uint8_t* D = dst + (size_t)i * npx + p0;
        uint32_t v[4];
        if (all_inside) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* s = S + off[k];
                v[k] = blend(s[0], s[1], s[cols], s[cols + 1], m2s[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (int)(int16_t)(m1s[k] & 0xffff), y = m1s[k] >> 16;
                v[k] = blend(tap(S, x, y, cols, rows), tap(S, x + 1, y, cols, rows), tap(S, x, y + 1, cols, rows),
                             tap(S, x + 1, y + 1, cols, rows), m2s[k]);
            }
        }
        if (full && ((reinterpret_cast<uintptr_t>(D) & 3) == 0)) {
            *reinterpret_cast<uint32_t*>(D) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < npx) D[k] = (uint8_t)v[k];
        }
    }
}

}  // namespace

namespace {

int rectify_make(stvo_ctx* ctx, int B, int cols, int rows, const stvo_rect_camera& cam, const int16_t* map1, const uint16_t* map2,
                 stvo_rectify** out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_rectify* r = new (std::nothrow) stvo_rectify();
    if (!r) return STVO_ERR_HIP;
    r->ctx = ctx;
    r->B = B; r->cols = cols; r->rows = rows;
    r->cam = cam;
    const size_t npx = (size_t)cols * rows;
    r->nquads = (int)((npx + 3) / 4);
    if (cam.dist) {
        // device layout: map1 as one int32 per pixel (x in the low half, y in the high half), map2 with the inside flag; padded with
        // (0, 0) entries to whole quads (never stored: the kernel writes only pixels < rows * cols)
        const size_t nq = (size_t)r->nquads, bytes = 2 * nq * (sizeof(int4) + sizeof(uint2));
        std::vector<char> host(bytes, 0);
        int32_t* h1 = reinterpret_cast<int32_t*>(host.data());
        uint16_t* h2 = reinterpret_cast<uint16_t*>(host.data() + 2 * nq * sizeof(int4));
        for (int side = 0; side < 2; ++side)
            for (size_t p = 0; p < npx; ++p) {
                const int x = map1[(side * npx + p) * 2], y = map1[(side * npx + p) * 2 + 1];
                const uint16_t f = (uint16_t)(map2[side * npx + p] & 1023u);
                h1[side * nq * 4 + p] = (int32_t)(((uint32_t)(uint16_t)x) | ((uint32_t)y << 16));
                const bool inside = x >= 0 && y >= 0 && x + 1 < cols && y + 1 < rows;
                h2[side * nq * 4 + p] = (uint16_t)(f | (inside ? INSIDE : 0u));
            }
        if (!hip_ok(ctx, hipMalloc((void**)&r->dev, bytes), "hipMalloc rectify maps") ||
            !upload_now(ctx, r->dev, host.data(), bytes, "hipMemcpy rectify maps")) {
            if (r->dev) (void)hipFree(r->dev);
            delete r;
            return STVO_ERR_HIP;
        }
    }
    *out = r;
    return STVO_OK;
}

int launch_remap(stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r) {
    stvo_ctx* ctx = r->ctx;
    const size_t bytes = (size_t)n * r->cols * r->rows;
    if (!r->cam.dist) {  // the reference copies (copyTo): a device-to-device copy on the context's stream
        HIP_TRY(ctx, hipMemcpyAsync(dst_l, src_l, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst_r, src_r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return STVO_OK;
    }
    // image chunks: enough blocks to fill 256 CUs a few times over, at least 4 images per thread where n allows
    const int bx = (r->nquads + RECT_BLOCK - 1) / RECT_BLOCK;
    const int want = std::max(1, (256 * 8 + 2 * bx - 1) / (2 * bx));
    const int chunks = std::max(1, std::min(want, (n + 3) / 4));
    const int per_chunk = (n + chunks - 1) / chunks;
    const int gy = (n + per_chunk - 1) / per_chunk;
    hipLaunchKernelGGL(rectify_remap_kernel, dim3(bx, gy, 2), dim3(RECT_BLOCK), 0, ctx->stream, r->map1q(0), r->map2q(0), r->map1q(1),
                       r->map2q(1), src_l, src_r, dst_l, dst_r, n, per_chunk, r->cols, r->rows, r->nquads);
    return check_launch(ctx);
}

int check_images(const stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, const uint8_t* dst_l, const uint8_t* dst_r) {
    if (!r || !src_l || !src_r || !dst_l || !dst_r || n <= 0 || n > r->B) return STVO_ERR_INVALID_ARG;
    const size_t bytes = (size_t)n * r->cols * r->rows;
    if (overlaps(dst_l, src_l, bytes) || overlaps(dst_l, src_r, bytes) || overlaps(dst_r, src_l, bytes) || overlaps(dst_r, src_r, bytes) ||
        overlaps(dst_l, dst_r, bytes))
        return STVO_ERR_INVALID_ARG;
    return STVO_OK;
}

}  // namespace

extern "C" {

int stvo_rectify_create(stvo_ctx* ctx, int B, const stvo_rect_calib* calib, stvo_rectify** out) {
    if (!ctx || !calib || !out || B <= 0) return STVO_ERR_INVALID_ARG;
    const size_t npx = (size_t)std::max(calib->width, 0) * std::max(calib->height, 0);
    stvo_rect_camera cam;
    std::vector<int16_t> m1(2 * 2 * npx);
    std::vector<uint16_t> m2(2 * npx);
    TRY(stvo_rectify_compute(calib, &cam, m1.data(), m2.data()));
    return rectify_make(ctx, B, calib->width, calib->height, cam, m1.data(), m2.data(), out);
}

int stvo_rectify_create_from_maps(stvo_ctx* ctx, int B, int cols, int rows, const int16_t* map1, const uint16_t* map2, stvo_rectify** out) {
    if (!ctx || !map1 || !map2 || !out || B <= 0 || cols <= 0 || rows <= 0 || cols > 32767 || rows > 32767) return STVO_ERR_INVALID_ARG;
    stvo_rect_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.dist = 1;
    cam.width = cols;
    cam.height = rows;
    return rectify_make(ctx, B, cols, rows, cam, map1, map2, out);
}

int stvo_rectify_destroy(stvo_rectify* r) {
    if (!r) return STVO_OK;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    if (r->dev) (void)hipFree(r->dev);
    if (r->io.p) (void)hipFree(r->io.p);
    delete r;
    return STVO_OK;
}

int stvo_rectify_camera(const stvo_rectify* r, stvo_rect_camera* out) {
    if (!r || !out) return STVO_ERR_INVALID_ARG;
    *out = r->cam;
    return STVO_OK;
}

int stvo_rectify_images_dev(stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r) {
    TRY(check_images(r, n, src_l, src_r, dst_l, dst_r));
    HIP_TRY(r->ctx, hipSetDevice(r->ctx->device));
    return launch_remap(r, n, src_l, src_r, dst_l, dst_r);
}

int stvo_rectify_images(stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r) {
    TRY(check_images(r, n, src_l, src_r, dst_l, dst_r));
    stvo_ctx* ctx = r->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * r->cols * r->rows;
    stvo::Carver size;
    stvo::carve_rectify_staging(size, r->B, r->cols, r->rows);
    TRY(staging_reserve(ctx, r->io, size.off));
    stvo::Carver c(r->io.p);
    const stvo::StereoStaging S = stvo::carve_rectify_staging(c, r->B, r->cols, r->rows);
    HIP_TRY(ctx, hipMemcpyAsync(S.src_l, src_l, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(S.src_r, src_r, bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch_remap(r, n, S.src_l, S.src_r, S.dst_l, S.dst_r));
    HIP_TRY(ctx, hipMemcpyAsync(dst_l, S.dst_l, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dst_r, S.dst_r, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

}  // extern "C"
