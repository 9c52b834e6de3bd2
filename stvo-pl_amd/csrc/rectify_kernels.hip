// rectify_kernels.hip — stereo rectification of raw 8-bit images (stvo_rectify_*): the cv::remap(INTER_LINEAR, BORDER_CONSTANT 0)
// that PinholeStereoCamera::rectifyImagesLR applies to every pair (src/pinholeStereoCamera.cpp:196-208), bit for bit.  This file holds
// the rectifier object (the maps as the kernels read them: rectify_px.h states the layout and the arithmetic) and the entry points of
// grey images; the kernel is the one-channel instance of the uniform remap kernel (color_kernels.hip, launch_remap).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "ctx_internal.h"
#include "rectify_internal.h"

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
        // device layout (rectify_px.h): map1 as one int32 per pixel, map2 with the inside flag; padded with (0, 0) entries to whole
        // quads (never stored: the kernel writes only pixels < rows * cols)
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
    TRY(check_images(r, n, 1, src_l, src_r, dst_l, dst_r));
    HIP_TRY(r->ctx, hipSetDevice(r->ctx->device));
    return launch_remap(r, n, 1, src_l, src_r, dst_l, dst_r);
}

int stvo_rectify_images(stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r) {
    TRY(check_images(r, n, 1, src_l, src_r, dst_l, dst_r));
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
    TRY(launch_remap(r, n, 1, S.src_l, S.src_r, S.dst_l, S.dst_r));
    HIP_TRY(ctx, hipMemcpyAsync(dst_l, S.dst_l, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dst_r, S.dst_r, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

}  // extern "C"
