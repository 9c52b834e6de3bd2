// color_kernels.hip — 8-bit interleaved colour images (B, G, R or B, G, R, A) in: the grey planes the detectors read, and the
// rectification of colour pairs (stvo_color_to_gray*, stvo_rectify_color_*).
//
// The reference reads its images unchanged and rectifies them with all their channels (src/dataset.cpp:147-157,
// src/pinholeStereoCamera.cpp:196-208); every consumer then makes its own grey image: cv::ORB, LSDDetectorC::detect and
// BinaryDescriptor::compute with COLOR_BGR2GRAY, the FLD branch with CV_RGB2GRAY on the same bytes (src/stereoFrame.cpp:249-258),
// which swaps the weights of channels 0 and 2.  So one pass may write two planes: A with the requested order, B with the other one.
//
//   color_to_gray_kernel   the batch [n, rows, cols, ch] is one pixel stream.  One thread = 16 pixels: ch 16-byte loads, one 16-byte
//                          store per plane; the thread after the last whole group does the tail (< 16 pixels) by bytes.  Needs the
//                          source and the planes 16-byte aligned.
//   color_to_gray_bytes    one thread = one pixel, byte loads and stores: bases that are not 16-byte aligned.
//   rectify_color_kernel   the uniform remap (one rectifier for every pair of the launch) of CH = 1, 3 or 4 channels.  One thread =
//                          4 consecutive output pixels of one side (the pixel index runs over rows * cols, so a quad may straddle
//                          two rows): one 16-B load of map1 and one 8-B load of map2, then a loop over the images of that side in
//                          this block's chunk with the maps held in registers; per image 4 taps per pixel and CH aligned dword
//                          stores (byte stores where the quad is not dword-aligned in the image or runs past its end).
//                          blockIdx.y = image chunk, blockIdx.z = side (0 left, 1 right).  GRAY = false writes the rectified image,
//                          which is rectifyImagesLR on a Mat of CH channels; GRAY = true rounds every colour channel to 8 bits as
//                          remap does, weights them and writes the plane(s) only: the rectified colour image never reaches memory.
//                          The loop over the quad's 4 pixels has one of two shapes, chosen per instance (HOISTED): with one channel
//                          the inside / border branch stands outside it and the tap offsets are 32-bit, which issues the 16 byte
//                          loads together (69 VGPRs); with 3 or 4 channels the branch stands inside it and the offsets are 64-bit
//                          (98 / 124 / 88 / 90 VGPRs for <3, false>, <4, false>, <3, true>, <4, true>: 4 - 5 waves per SIMD), since
//                          the hoisted shape costs those instances 125 - 135 VGPRs and a wave.
//
// rectify_px.h states the arithmetic: the remap's (X + 512) >> 10 per channel, a tap outside the source reads 0, the inside flag of
// map2, and cvtColor's integer grey weights.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ctx_internal.h"
#include "rectify_bank_plan.h"
#include "rectify_internal.h"

namespace {

constexpr int COLOR_BLOCK = 256;
constexpr int GROUP = 16;  // pixels per thread of the stream kernel

template <int CH, bool TWO>
__global__ void __launch_bounds__(COLOR_BLOCK) color_to_gray_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ pa,
                                                                    uint8_t* __restrict__ pb, size_t npix, size_t ngroups,
                                                                    GrayWeights w) {
    const size_t g = (size_t)blockIdx.x * COLOR_BLOCK + threadIdx.x;
    if (g < ngroups) {
        const uint4* s = reinterpret_cast<const uint4*>(src) + g * CH;
        uint32_t d[4 * CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const uint4 v = s[k];
            d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
        }
        uint32_t a[4] = {0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const int j = k * CH;
            const uint32_t c0 = (d[j >> 2] >> ((j & 3) * 8)) & 0xffu;
            const uint32_t c1 = (d[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xffu;
            const uint32_t c2 = (d[(j + 2) >> 2] >> (((j + 2) & 3) * 8)) & 0xffu;
            a[k >> 2] |= weigh(c0, c1, c2, w.w0, w.w1, w.w2, w) << ((k & 3) * 8);
            if (TWO) b[k >> 2] |= weigh(c0, c1, c2, w.w2, w.w1, w.w0, w) << ((k & 3) * 8);
        }
        reinterpret_cast<uint4*>(pa)[g] = make_uint4(a[0], a[1], a[2], a[3]);
        if (TWO) reinterpret_cast<uint4*>(pb)[g] = make_uint4(b[0], b[1], b[2], b[3]);
    } else if (g == ngroups) {  // the tail
        for (size_t p = ngroups * GROUP; p < npix; ++p) {
            const uint8_t* s = src + p * CH;
            pa[p] = (uint8_t)weigh(s[0], s[1], s[2], w.w0, w.w1, w.w2, w);
            if (TWO) pb[p] = (uint8_t)weigh(s[0], s[1], s[2], w.w2, w.w1, w.w0, w);
        }
    }
}

template <int CH, bool TWO>
__global__ void __launch_bounds__(COLOR_BLOCK) color_to_gray_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ pa,
                                                                   uint8_t* __restrict__ pb, size_t npix, GrayWeights w) {
    const size_t p = (size_t)blockIdx.x * COLOR_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const uint8_t* s = src + p * CH;
    const uint32_t c0 = s[0], c1 = s[1], c2 = s[2];
    pa[p] = (uint8_t)weigh(c0, c1, c2, w.w0, w.w1, w.w2, w);
    if (TWO) pb[p] = (uint8_t)weigh(c0, c1, c2, w.w2, w.w1, w.w0, w);
}

// map1q / map2q: one side's maps padded to whole quads.  src / dst: this side's first image; source images npx * CH bytes apart.
// GRAY = false: dst holds CH-channel images (npx * CH bytes apart), dstb and w unused.  GRAY = true: dst is plane A, dstb plane B or
// NULL (both sides), images npx bytes apart.
template <int CH, bool GRAY>
__global__ void __launch_bounds__(COLOR_BLOCK) rectify_color_kernel(const int4* __restrict__ map1q_l, const uint2* __restrict__ map2q_l,
                                                                    const int4* __restrict__ map1q_r, const uint2* __restrict__ map2q_r,
                                                                    const uint8_t* __restrict__ src_l, const uint8_t* __restrict__ src_r,
                                                                    uint8_t* __restrict__ dst_l, uint8_t* __restrict__ dst_r,
                                                                    uint8_t* __restrict__ dstb_l, uint8_t* __restrict__ dstb_r, int n,
                                                                    int per_chunk, int cols, int rows, int nquads, GrayWeights w) {
    constexpr int NC = GRAY ? 3 : CH;  // channels computed: the grey planes never read alpha
    constexpr bool HOISTED = CH == 1;  // the shape of the loop over the quad's pixels (see the top of the file)
    const int q = blockIdx.x * COLOR_BLOCK + threadIdx.x;
    if (q >= nquads) return;
    const bool right = blockIdx.z != 0;
    const int i0 = blockIdx.y * per_chunk;
    const int i1 = min(n, i0 + per_chunk);
    if (i0 >= i1) return;
    const int4 m1 = (right ? map1q_r : map1q_l)[q];
    const uint2 m2v = (right ? map2q_r : map2q_l)[q];
    const uint8_t* src = right ? src_r : src_l;
    uint8_t* dst = right ? dst_r : dst_l;
    uint8_t* dstb = right ? dstb_r : dstb_l;
    const size_t npx = (size_t)cols * rows;
    const size_t p0 = (size_t)q * 4;
    const size_t row_b = (size_t)cols * CH;
    const int m1s[4] = {m1.x, m1.y, m1.z, m1.w};
    const uint32_t m2s[4] = {m2v.x & 0xffffu, m2v.x >> 16, m2v.y & 0xffffu, m2v.y >> 16};
    bool all_inside = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) all_inside = all_inside && (m2s[k] & INSIDE);
    const bool full = p0 + 4 <= npx;
    auto at = [&](int x, int y) { return ((size_t)y * cols + x) * CH; };  // a pixel's offset in its image
    int off[4];  // HOISTED: the offset of the top-left tap (one channel: an image is below 2^31 bytes), valid where the pixel is inside
    if constexpr (HOISTED) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int x, y;
            map_tap(m1s[k], x, y);
            off[k] = y * cols + x;
        }
    }
    for (int i = i0; i < i1; ++i) {
        const uint8_t* S = src + (size_t)i * npx * CH;
        uint32_t v[4][NC];
        if constexpr (HOISTED) {
            if (all_inside) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t t00[NC], t01[NC], t10[NC], t11[NC];
                    const uint8_t* s = S + off[k];
                    load_px<CH, NC>(s, t00);
                    load_px<CH, NC>(s + CH, t01);
                    load_px<CH, NC>(s + cols, t10);
                    load_px<CH, NC>(s + cols + CH, t11);
#pragma unroll
                    for (int c = 0; c < NC; ++c) v[k][c] = blend(t00[c], t01[c], t10[c], t11[c], m2s[k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int x, y;
                    map_tap(m1s[k], x, y);
                    uint32_t t00[NC], t01[NC], t10[NC], t11[NC];
                    tap_px<CH, NC>(S, x, y, cols, rows, at, t00);
                    tap_px<CH, NC>(S, x + 1, y, cols, rows, at, t01);
                    tap_px<CH, NC>(S, x, y + 1, cols, rows, at, t10);
                    tap_px<CH, NC>(S, x + 1, y + 1, cols, rows, at, t11);
#pragma unroll
                    for (int c = 0; c < NC; ++c) v[k][c] = blend(t00[c], t01[c], t10[c], t11[c], m2s[k]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int x, y;
                map_tap(m1s[k], x, y);
                uint32_t t00[NC], t01[NC], t10[NC], t11[NC];
                if (all_inside) {
                    const uint8_t* s = S + ((size_t)y * cols + x) * CH;
                    load_px<CH, NC>(s, t00);
                    load_px<CH, NC>(s + CH, t01);
                    load_px<CH, NC>(s + row_b, t10);
                    load_px<CH, NC>(s + row_b + CH, t11);
                } else {
                    tap_px<CH, NC>(S, x, y, cols, rows, at, t00);
                    tap_px<CH, NC>(S, x + 1, y, cols, rows, at, t01);
                    tap_px<CH, NC>(S, x, y + 1, cols, rows, at, t10);
                    tap_px<CH, NC>(S, x + 1, y + 1, cols, rows, at, t11);
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) v[k][c] = blend(t00[c], t01[c], t10[c], t11[c], m2s[k]);
            }
        }
        if (GRAY) {
            uint8_t* D = dst + (size_t)i * npx + p0;
            uint32_t ga[4][1], gao[1];
#pragma unroll
            for (int k = 0; k < 4; ++k) ga[k][0] = weigh(v[k][0], v[k][1], v[k][2], w.w0, w.w1, w.w2, w);
            if (full && ((reinterpret_cast<uintptr_t>(D) & 3) == 0)) {
                pack_quad<1>(ga, gao);
                *reinterpret_cast<uint32_t*>(D) = gao[0];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p0 + k < npx) D[k] = (uint8_t)ga[k][0];
            }
            if (dstb) {
                uint8_t* E = dstb + (size_t)i * npx + p0;
                uint32_t gb[4][1], gbo[1];
#pragma unroll
                for (int k = 0; k < 4; ++k) gb[k][0] = weigh(v[k][0], v[k][1], v[k][2], w.w2, w.w1, w.w0, w);
                if (full && ((reinterpret_cast<uintptr_t>(E) & 3) == 0)) {
                    pack_quad<1>(gb, gbo);
                    *reinterpret_cast<uint32_t*>(E) = gbo[0];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (p0 + k < npx) E[k] = (uint8_t)gb[k][0];
                }
            }
        } else {
            uint8_t* D = dst + ((size_t)i * npx + p0) * CH;
            if (full && ((reinterpret_cast<uintptr_t>(D) & 3) == 0)) {
                uint32_t o[CH];
                if constexpr (!GRAY) pack_quad<CH>(v, o);
#pragma unroll
                for (int c = 0; c < CH; ++c) reinterpret_cast<uint32_t*>(D)[c] = o[c];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p0 + k < npx) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) D[k * CH + c] = (uint8_t)v[k][c];
                    }
            }
        }
    }
}

template <int CH>
void launch_gray_ch(hipStream_t st, const uint8_t* src, uint8_t* pa, uint8_t* pb, size_t npix, const GrayWeights& w) {
    const bool aligned = (((uintptr_t)src | (uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
    if (aligned) {
        const size_t ngroups = npix / GROUP;
        const unsigned blocks = (unsigned)((ngroups + 1 + COLOR_BLOCK - 1) / COLOR_BLOCK);
        if (pb)
            hipLaunchKernelGGL((color_to_gray_kernel<CH, true>), dim3(blocks), dim3(COLOR_BLOCK), 0, st, src, pa, pb, npix, ngroups, w);
        else
            hipLaunchKernelGGL((color_to_gray_kernel<CH, false>), dim3(blocks), dim3(COLOR_BLOCK), 0, st, src, pa, pb, npix, ngroups, w);
    } else {
        const unsigned blocks = (unsigned)((npix + COLOR_BLOCK - 1) / COLOR_BLOCK);
        if (pb)
            hipLaunchKernelGGL((color_to_gray_bytes<CH, true>), dim3(blocks), dim3(COLOR_BLOCK), 0, st, src, pa, pb, npix, w);
        else
            hipLaunchKernelGGL((color_to_gray_bytes<CH, false>), dim3(blocks), dim3(COLOR_BLOCK), 0, st, src, pa, pb, npix, w);
    }
}

// pixel counts the one-dimensional grids hold: the byte kernel has one thread per pixel
constexpr size_t MAX_STREAM_PIXELS = (size_t)0x7fffffffu * COLOR_BLOCK;

int launch_gray(stvo_ctx* ctx, int ch, const uint8_t* src, uint8_t* pa, uint8_t* pb, size_t npix, const GrayWeights& w) {
    if (ch == 3)
        launch_gray_ch<3>(ctx->stream, src, pa, pb, npix, w);
    else
        launch_gray_ch<4>(ctx->stream, src, pa, pb, npix, w);
    return check_launch(ctx);
}

int check_gray(int n, int rows, int cols, int ch, const uint8_t* src, const uint8_t* pa, const uint8_t* pb, size_t* npix) {
    if (n <= 0 || rows <= 0 || cols <= 0 || (ch != 3 && ch != 4) || !src || !pa) return STVO_ERR_INVALID_ARG;
    const size_t px = (size_t)n * rows * cols;
    if (px > MAX_STREAM_PIXELS) return STVO_ERR_CAPACITY;
    if (overlaps(src, px * ch, pa, px) || (pb && (overlaps(src, px * ch, pb, px) || overlaps(pa, px, pb, px)))) return STVO_ERR_INVALID_ARG;
    *npix = px;
    return STVO_OK;
}

// The device block of ONE host-buffer call.  Whichever way the call ends, copies and kernels may still be using the block: the
// context's stream is synchronised before it is freed.
struct CallBlock {
    stvo_ctx* ctx;
    uint8_t* p = nullptr;
    ~CallBlock() {
        if (!p) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
    }
};

template <int CH, bool GRAY>
void launch_rect_ch(stvo_rectify* r, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r, uint8_t* dstb_l,
                    uint8_t* dstb_r, const GrayWeights& w) {
    // image chunks by the bank's rule with every pair on this calibration (rectify_bank_plan.h)
    const int bx = (r->nquads + COLOR_BLOCK - 1) / COLOR_BLOCK;
    int per_chunk = 0;
    const int gy = stvo::rbank_chunks(bx, n, &per_chunk);
    hipLaunchKernelGGL((rectify_color_kernel<CH, GRAY>), dim3(bx, gy, 2), dim3(COLOR_BLOCK), 0, r->ctx->stream, r->map1q(0), r->map2q(0),
                       r->map1q(1), r->map2q(1), src_l, src_r, dst_l, dst_r, dstb_l, dstb_r, n, per_chunk, r->cols, r->rows, r->nquads, w);
}

}  // namespace

int stvo_detail::launch_remap(stvo_rectify* r, int n, int ch, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r) {
    stvo_ctx* ctx = r->ctx;
    if (!r->cam.dist) {  // the reference copies (copyTo): a device-to-device copy on the context's stream
        const size_t bytes = (size_t)n * r->cols * r->rows * ch;
        HIP_TRY(ctx, hipMemcpyAsync(dst_l, src_l, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst_r, src_r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return STVO_OK;
    }
    const GrayWeights none{};
    if (ch == 1)
        launch_rect_ch<1, false>(r, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    else if (ch == 3)
        launch_rect_ch<3, false>(r, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    else
        launch_rect_ch<4, false>(r, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    return check_launch(ctx);
}

extern "C" {

int stvo_color_to_gray_dev(stvo_ctx* ctx, int n, int rows, int cols, int channels, int order, int weights, const uint8_t* src,
                           uint8_t* gray, uint8_t* gray_swapped) {
    GrayWeights w;
    size_t npix = 0;
    if (!ctx || !gray_weights(order, weights, &w)) return STVO_ERR_INVALID_ARG;
    TRY(check_gray(n, rows, cols, channels, src, gray, gray_swapped, &npix));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_gray(ctx, channels, src, gray, gray_swapped, npix, w);
}

int stvo_color_to_gray(stvo_ctx* ctx, int n, int rows, int cols, int channels, int order, int weights, const uint8_t* src, uint8_t* gray,
                       uint8_t* gray_swapped) {
    GrayWeights w;
    size_t npix = 0;
    if (!ctx || !gray_weights(order, weights, &w)) return STVO_ERR_INVALID_ARG;
    TRY(check_gray(n, rows, cols, channels, src, gray, gray_swapped, &npix));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::Carver size;
    stvo::carve_gray_staging(size, npix, channels);
    CallBlock io{ctx};
    HIP_TRY(ctx, hipMalloc((void**)&io.p, size.off));
    stvo::Carver c(io.p);
    const stvo::GrayStaging S = stvo::carve_gray_staging(c, npix, channels);
    uint8_t* db = gray_swapped ? S.swapped : nullptr;
    HIP_TRY(ctx, hipMemcpyAsync(S.src, src, npix * channels, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch_gray(ctx, channels, S.src, S.gray, db, npix, w));
    HIP_TRY(ctx, hipMemcpyAsync(gray, S.gray, npix, hipMemcpyDeviceToHost, ctx->stream));
    if (db) HIP_TRY(ctx, hipMemcpyAsync(gray_swapped, db, npix, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_rectify_color_images_dev(stvo_rectify* r, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                                  uint8_t* dst_r) {
    if (channels != 3 && channels != 4) return STVO_ERR_INVALID_ARG;
    TRY(check_images(r, n, channels, src_l, src_r, dst_l, dst_r));
    HIP_TRY(r->ctx, hipSetDevice(r->ctx->device));
    return launch_remap(r, n, channels, src_l, src_r, dst_l, dst_r);
}

int stvo_rectify_color_images(stvo_rectify* r, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                              uint8_t* dst_r) {
    if (channels != 3 && channels != 4) return STVO_ERR_INVALID_ARG;
    TRY(check_images(r, n, channels, src_l, src_r, dst_l, dst_r));
    stvo_ctx* ctx = r->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * r->cols * r->rows * channels;
    stvo::Carver size;
    stvo::carve_color_rectify_staging(size, n, r->cols, r->rows, channels);
    CallBlock io{ctx};
    HIP_TRY(ctx, hipMalloc((void**)&io.p, size.off));
    stvo::Carver c(io.p);
    const stvo::StereoStaging S = stvo::carve_color_rectify_staging(c, n, r->cols, r->rows, channels);
    HIP_TRY(ctx, hipMemcpyAsync(S.src_l, src_l, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(S.src_r, src_r, bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch_remap(r, n, channels, S.src_l, S.src_r, S.dst_l, S.dst_r));
    HIP_TRY(ctx, hipMemcpyAsync(dst_l, S.dst_l, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dst_r, S.dst_r, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_rectify_color_to_gray_dev(stvo_rectify* r, int n, int channels, int order, int weights, const uint8_t* src_l, const uint8_t* src_r,
                                   uint8_t* gray_l, uint8_t* gray_r, uint8_t* swapped_l, uint8_t* swapped_r) {
    GrayWeights w;
    if (!r || !src_l || !src_r || !gray_l || !gray_r || n <= 0 || n > r->B || (channels != 3 && channels != 4) ||
        (swapped_l == nullptr) != (swapped_r == nullptr) || !gray_weights(order, weights, &w))
        return STVO_ERR_INVALID_ARG;
    const size_t px = (size_t)n * r->cols * r->rows, sb = px * channels;
    const uint8_t* planes[4] = {gray_l, gray_r, swapped_l, swapped_r};
    if (!gray_planes_ok(planes, swapped_l ? 4 : 2, px, src_l, src_r, sb)) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = r->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!r->cam.dist) {  // the reference's copy, then the consumers' conversion: the plain conversion of each side
        TRY(launch_gray(ctx, channels, src_l, gray_l, swapped_l, px, w));
        return launch_gray(ctx, channels, src_r, gray_r, swapped_r, px, w);
    }
    if (channels == 3)
        launch_rect_ch<3, true>(r, n, src_l, src_r, gray_l, gray_r, swapped_l, swapped_r, w);
    else
        launch_rect_ch<4, true>(r, n, src_l, src_r, gray_l, gray_r, swapped_l, swapped_r, w);
    return check_launch(ctx);
}

}  // extern "C"
