// rectify_px.h — the pixel arithmetic of the input stage, stated ONCE: the fixed-point bilinear of cv::remap, cvtColor's integer grey
// weights, how a map word gives a tap and how 4 pixels become dwords.  color_kernels.hip (the uniform remap of 1, 3 and 4 channels,
// its fused colour -> grey form and the plain conversion) and rectify_bank.hip (the same per pair, for mixed cameras) draw every
// primitive from here; each kernel keeps its own addressing (tap_px takes it as `at`) and its own store rule.  The part above the
// device section is host-pure (g++ alone compiles it).
//
// What a kernel still writes itself, and why: the split of a quad's int4 / uint2 into words with the test of INSIDE over them, and the
// run "four load_px, then blend per channel" of a pixel.  Either one moved into a function here compiles to other code in kernels that
// this header must leave as they are (the bank's prologue is re-ordered; the colour kernels of color_kernels.hip go from 98 / 124 /
// 88 / 90 to 84 / 102 / 77 / 72 VGPRs with another load schedule): they use only the primitives below, in place.
//
// Remap (OpenCV's fixed-point bilinear: initInterTab2D(INTER_LINEAR, fixpt = true) gives, for fractions ax, ay in 1/32 px, the weights
// (32-ax)(32-ay)*32, ax(32-ay)*32, (32-ax)ay*32, ax*ay*32 — they sum to 32768, so the table needs no correction — and remapBilinear
// rounds (sum S*w + 2^14) >> 15).  Since every weight is 32 times an integer, that equals (X + 512) >> 10 with
// X = (32-ay)((32-ax)S00 + ax S01) + ay((32-ax)S10 + ax S11) < 2^18: 24-bit multiplies, no table; per channel for colour images.  A tap
// outside the source reads 0 (BORDER_CONSTANT: borderInterpolate -> -1 -> cval; a pixel whose taps are all outside gets cval, which is
// the same 0).
//
// Maps on the device: map1 as one int32 per pixel (x in the low half, y in the high half), map2 as one uint16 (ax in bits 0-4, ay in
// bits 5-9) whose bit 15 says "all four taps inside the source" (the host sets it once, when the maps are uploaded), so the common path
// has no per-tap tests.  A quad is 4 consecutive pixels: one int4 of map1 and one uint2 of map2.
//
// Grey (cvtColor's 8-bit integer form): (w0 c0 + w1 c1 + w2 c2 + 2^(shift-1)) >> shift with (blue, green, red) weights
// (1868, 9617, 4899) and shift 14, the table form of OpenCV 3.0 - 3.4.1, or (3735, 19235, 9798) and shift 15 of the later releases.
// The sum stays below 2^23 + 2^14, so 32-bit arithmetic is exact.
#pragma once

#include <cstddef>
#include <cstdint>

namespace stvo_detail {

constexpr uint32_t INSIDE = 0x8000u;  // of a map2 word: all four taps of the pixel lie inside the source

struct GrayWeights {
    uint32_t w0, w1, w2, rnd, shift;  // plane A; plane B swaps w0 and w2
};

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t weigh(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t w0, uint32_t w1, uint32_t w2,
                                          const GrayWeights& w) {
    return (w0 * c0 + w1 * c1 + w2 * c2 + w.rnd) >> w.shift;
}

__device__ __forceinline__ uint32_t blend(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, uint32_t m2) {
    const uint32_t ax = m2 & 31u, ay = (m2 >> 5) & 31u;
    const uint32_t top = __umul24(32u - ax, s00) + __umul24(ax, s01);
    const uint32_t bot = __umul24(32u - ax, s10) + __umul24(ax, s11);
    return (__umul24(32u - ay, top) + __umul24(ay, bot) + 512u) >> 10;
}

// The first NC channels of the pixel at p.  A 4-channel pixel is one (unaligned) 32-bit load: three byte loads per tap made the fused
// kernel slower on B, G, R, A than remap-then-convert; a 1- or 3-channel pixel is read by bytes (a word would run past the last pixel).
template <int CH, int NC>
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ p, uint32_t (&c)[NC]) {
    if (CH == 4) {
        uint32_t w;
        __builtin_memcpy(&w, p, 4);
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = (w >> (8 * k)) & 0xffu;
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = p[k];
    }
}

// The pixel (x, y) of a cols x rows image at S; 0 outside the image.  at(x, y) is the pixel's byte offset: the addressing is the
// kernel's own (the uniform kernels' rows are cols * CH bytes apart, the bank's a slot's pitch), asked for only where the pixel exists.
template <int CH, int NC, typename At>
__device__ __forceinline__ void tap_px(const uint8_t* __restrict__ S, int x, int y, int cols, int rows, const At& at, uint32_t (&c)[NC]) {
    if ((unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows) {
        load_px<CH, NC>(S + at(x, y), c);
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = 0u;
    }
}

// One pixel's word of map1: its top-left tap.
__device__ __forceinline__ void map_tap(int m1, int& x, int& y) {
    x = (int)(int16_t)(m1 & 0xffff);
    y = m1 >> 16;
}

// 4 pixels x CH values (each < 256) as the CH dwords that hold them in memory
template <int CH>
__device__ __forceinline__ void pack_quad(const uint32_t (&v)[4][CH], uint32_t (&o)[CH]) {
#pragma unroll
    for (int c = 0; c < CH; ++c) o[c] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int j = k * CH + c;
            o[j >> 2] |= v[k][c] << ((j & 3) * 8);
        }
}

#endif  // __HIPCC__

}  // namespace stvo_detail
