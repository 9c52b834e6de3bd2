// lsd_scale_kernels.hip — the scaled image of the LSD detector for every blur radius but 3 (lsd_kernels.hip keeps the 7 x 7 route:
// launch_blur7_u8 + launch_resize_linear_u8):  cv::GaussianBlur(img, (1 + 2h) x (1 + 2h), sigma)  +  cv::resize(…, Size(), scale, scale)
// on 8-bit data, as oracle/stvo_lsd_oracle.c:82-109 states the blur for h = 3 (OpenCV 3's separable fixed point: integer weights x 2^8
// per pass, BORDER_REFLECT_101 repeated while the index is outside, ONE rounding shift by 16, bytes BEFORE the resize reads them) and
// orb_kernels.hip's orb_resize_kernel the resize; bit-exact against that statement for h = 0 .. 15 (tests/test_gpu_lsd_scale.py).
//
// lsd_blur_resize_kernel: one workgroup per tile of the SCALED image, everything between the source bytes and the scaled bytes in LDS.
//   1. the source columns / rows the tile's bilinear taps read (two per output column / row): when they span no more than 2 x the
//      tile they are taken as one contiguous run, otherwise (scale < 0.5) as the list of pairs — at 0.25 half of the columns and rows
//   2. the source window those need, widened by the radius, staged as bytes (word loads, four in flight per thread; the images are
//      at least 4 bytes wide); the reflection is resolved HERE, once per byte
//   3. horizontal sums (32 bit: a weight can be 256 and the weights can add up to 259, so a sum needs 17 bits) for every staged row,
//      only in the columns of 1.; a thread makes 4 adjacent sums of a run (2 of a pair) from the bytes they share
//   4. vertical sums + rounding + clamp, only in the rows of 1.: the blurred bytes; again 4 (2) per thread down a column
//   5. orb_resize_kernel's arithmetic on those bytes -> the tile of the scaled image
// A down-scale neither writes nor reads a full-size blurred image.  The radius is a template argument (one instance per radius: the
// tap loops unroll, the weights — 32-bit values from the kernel-argument segment — sit in scalar registers and the LDS reads carry
// immediate offsets; with the radius as a launch argument every tap waited for a scalar load of its weight), the tile a launch
// argument chosen by the host so that the LDS fits (lsd_scale_plan.h).
//
// One image size per image (stvo_lsd_set_image_sizes on a detector created with STVO_LSD_SIZES_ANY_RADIUS): the MIXED instance, in the
// form of lsd_kernels.hip — the table (LsdTable<MIXED>, lsd_sizes.h) an argument of its own, empty for the uniform instance, one body.  A workgroup takes its image
// from blockIdx.z and that image's row of the table with scalar loads; the row replaces the BOUNDS only (the source size for the taps,
// the reflection and the word-load clamp; the scaled size for the tile's extent and the store), the pitches and the strides per image
// stay the slot's, source and scaled.  The launch is the slot's — its grid, its tile, its LDS, which bounds the need of every tile of
// every image that fits the slot (lsd_scale_plan.h) — and a workgroup whose tile lies outside its image's scaled size leaves as a
// whole before the first barrier.  Nothing is read outside the image's crop and nothing written outside the top-left w_i x h_i of its
// slot of the scaled buffer.  The uniform instances are the code they were (profiles/mixed_lsd_scale_kernel_resources.txt).
#include "kernels.h"
#include "lsd_sizes.h"

#pragma clang fp contract(off)

namespace stvo {
namespace {

constexpr int BR_T = 256;                 // threads of a workgroup

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;  // a word at any byte address (gfx950 global memory allows it)

__device__ __forceinline__ int reflect101(int p, int n) {  // BORDER_REFLECT_101, repeated: the radius may exceed the image
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        if (p >= n) p = 2 * n - 2 - p;
    }
    return p;
}

// The two source indices and 11-bit weights of destination index d (orb_resize_kernel / orc_resize_linear_fxy): along x a position
// outside the image is moved to the border WITH its weights (fx = 0), along y only the indices are clamped.
template <bool X>
__device__ __forceinline__ void resize_taps(int d, double step, int n, int& i0, int& i1, int& w0, int& w1) {
    float f = (float)(((double)d + 0.5) * step - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (X) {
        if (s < 0) {
            f = 0.f;
            s = 0;
        }
        if (s >= n - 1) {
            f = 0.f;
            s = n - 1;
        }
    }
    w0 = (short)__float2int_rn((1.f - f) * 2048.f);
    w1 = (short)__float2int_rn(f * 2048.f);
    i0 = min(max(s, 0), n - 1);
    i1 = min(max(s + 1, 0), n - 1);
}

struct BlurResizeArgs {
    int B, scols, srows, dcols, drows;
    int tw_log, th_log;       // tile of the scaled image: (1 << tw_log) x (1 << th_log)
    int lds_bytes;            // what the launch provides
    double step_x, step_y;    // 1 / scale (cv::resize keeps inv_scale = fx, fy as given)
    const uint8_t* src;       // [B][srows][scols]
    uint8_t* dst;             // [B][drows][dcols]
    int k[STVO_LSD_MAX_TAPS]; // the integer weights
};

// R sums of 1 + 2 HK taps each over R + 2 HK consecutive values: sum u covers v[u .. u + 2 HK].  Weights <= 2^8, bytes < 2^8, row
// sums < 2^24: the 24-bit multiplies are exact; the sums are integers, so their order is free.
template <int HK, int R>
__device__ __forceinline__ void tap_sums(const uint32_t (&v)[R + 2 * HK], const int* k, uint32_t (&acc)[R]) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
        for (int i = 0; i <= 2 * HK; ++i) acc[u] += __umul24((uint32_t)k[i], v[u + i]);
    }
}

template <int HK, bool MIXED>  // radius: 1 + 2 HK taps; MIXED: the bounds of every image from its row of the table
__global__ __launch_bounds__(BR_T) void lsd_blur_resize_kernel(BlurResizeArgs a, LsdTable<MIXED> tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char br_lds[];
    const int tid = threadIdx.x;
    const int tw = 1 << a.tw_log, th = 1 << a.th_log;
    const int dx0 = blockIdx.x << a.tw_log, dy0 = blockIdx.y << a.th_log, b = blockIdx.z;
    // the slot's pitches and strides per image, before the image's own bounds take the place of a.scols .. a.drows in the kernel's copy
    // of its argument (so the text below is one for both instances; the uniform instance does none of this)
    const int spitch = a.scols, sheight = a.srows, dpitch = a.dcols, dheight = a.drows;
    if constexpr (MIXED) {  // the row is uniform over the workgroup; it is clamped into the slot, which the host has validated it to fit
        const LsdSizeRow* e = tab.sz + (b % tab.n_sz);
        a.scols = __builtin_amdgcn_readfirstlane(min(max(e->cols, 8), a.scols));
        a.srows = __builtin_amdgcn_readfirstlane(min(max(e->rows, 1), a.srows));
        a.dcols = __builtin_amdgcn_readfirstlane(min(max(e->w, 1), a.dcols));
        a.drows = __builtin_amdgcn_readfirstlane(min(max(e->h, 1), a.drows));
        if (dx0 >= a.dcols || dy0 >= a.drows) return;  // a tile of the slot's grid outside this image: block-uniform, before any barrier
    }
    const int ntw = min(tw, a.dcols - dx0), nth = min(th, a.drows - dy0);
    constexpr int hk = HK;
    int cmin, cmax, rmin, rmax, t0, t1, t2;  // (the taps are monotonic in d: the first and the last output bound the window)
    resize_taps<true>(dx0, a.step_x, a.scols, cmin, t0, t1, t2);
    resize_taps<true>(dx0 + ntw - 1, a.step_x, a.scols, t0, cmax, t1, t2);
    resize_taps<false>(dy0, a.step_y, a.srows, rmin, t0, t1, t2);
    resize_taps<false>(dy0 + nth - 1, a.step_y, a.srows, t0, rmax, t1, t2);
    // (lsd_scale_plan.h: br_tile_layout states these four lines for the host, and says why they stay here; tests/test_lsd_scale_plan_host.py
    // holds the two texts together)
    const int nx = cmax - cmin + 1, ny = rmax - rmin + 1;
    const bool xlist = nx > 2 * ntw, ylist = ny > 2 * nth;  // the taps as pairs per output (scale < 0.5), not as one contiguous run
    const int nr = ylist ? 2 * nth : ny;
    const BrLayout l = br_layout(nx, ny, 4 * (((xlist ? 2 * ntw : nx) + 3) / 4), nr, hk, tw, th);
    if (l.bytes > a.lds_bytes) return;  // never: the host sizes the launch by an upper bound of this
    const int sr = l.sr, scp = l.scp, ncp = l.ncp;
    uint32_t* s_h = reinterpret_cast<uint32_t*>(br_lds);                  // [sr][ncp] horizontal sums
    int4* s_xt = reinterpret_cast<int4*>(s_h + sr * ncp);                 // [ntw] the taps of an output column: (first tap's column of the window = source
                                                                          //   column - cmin, second tap 0 / 1 columns further, the two weights)
    int4* s_yt = s_xt + tw;                                               // [nth] the same for the output rows
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_yt + th);               // [sr][scp] source bytes from (rmin - hk, cmin - hk), reflected; 0 beyond nx + 2 hk
    uint8_t* s_bl = s_src + sr * scp;                                     // [nr][ncp] blurred bytes

    for (int d = tid; d < ntw + nth; d += BR_T) {  // (the coordinate arithmetic is in double: once per column and row, not per pixel)
        int i0, i1, w0, w1;
        if (d < ntw) {
            resize_taps<true>(dx0 + d, a.step_x, a.scols, i0, i1, w0, w1);
            s_xt[d] = make_int4(i0 - cmin, i1 - i0, w0, w1);
        } else {
            resize_taps<false>(dy0 + d - ntw, a.step_y, a.srows, i0, i1, w0, w1);
            s_yt[d - ntw] = make_int4(i0 - rmin, i1 - i0, w0, w1);
        }
    }
    const uint8_t* img = a.src + (size_t)b * sheight * spitch;
    // staging, a word of the window per thread and four of them in flight: away from the image border a word of the window is a word
    // of the image (at any byte address); at the border, and in the padding of a row, it is put together byte by byte
    {
        uint32_t* src32 = reinterpret_cast<uint32_t*>(s_src);
        const int scp4 = scp >> 2, nwords = sr * scp4, wn = nx + 2 * hk;
        for (int t0 = tid; t0 < nwords; t0 += 4 * BR_T) {
            uint32_t w[4];
            int gx[4];
            const uint8_t* row[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = min(t0 + m * BR_T, nwords - 1), r = t / scp4;
                gx[m] = cmin - hk + 4 * (t - r * scp4);
                row[m] = img + (size_t)reflect101(rmin - hk + r, a.srows) * spitch;
                w[m] = *reinterpret_cast<const u32_unaligned*>(row[m] + min(max(gx[m], 0), a.scols - 4));
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = t0 + m * BR_T, c = gx[m] - (cmin - hk);
                if (t >= nwords) break;
                if (gx[m] < 0 || gx[m] + 3 >= a.scols || c + 3 >= wn) {
                    w[m] = 0u;
                    for (int q = 0; q < 4; ++q)
                        if (c + q < wn) w[m] |= (uint32_t)row[m][reflect101(gx[m] + q, a.scols)] << (8 * q);
                }
                src32[t] = w[m];
            }
        }
    }
    __syncthreads();
    // horizontal sums for every staged row.  A contiguous run: a thread makes 4 adjacent sums from the 4 + 2 hk bytes they share, read
    // as aligned words.  Pairs: the two sums of an output column from the 2 + 2 hk bytes at its first tap (its second tap is the same
    // column at the image's right edge, the next one elsewhere).
    if (!xlist) {
        constexpr int NW = 1 + (2 * HK + 3) / 4;  // words that hold 4 + 2 HK bytes
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(s_src);
        const int ng = ncp >> 2, scp4 = scp >> 2;
        for (int t = tid; t < sr * ng; t += BR_T) {
            const int r = t / ng, g = t - r * ng;
            uint32_t w[NW], v[4 + 2 * HK], acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int m = 0; m < NW; ++m) w[m] = src32[r * scp4 + g + m];
#pragma unroll
            for (int i = 0; i < 4 + 2 * HK; ++i) v[i] = (w[i >> 2] >> (8 * (i & 3))) & 255u;
            tap_sums<HK, 4>(v, a.k, acc);
            *reinterpret_cast<uint4*>(s_h + r * ncp + 4 * g) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        }
    } else {
        for (int t = tid; t < sr * ntw; t += BR_T) {
            const int r = t / ntw, d = t - r * ntw;
            const int c0 = s_xt[d].x, second = s_xt[d].y;
            const uint8_t* p = s_src + r * scp + c0;
            uint32_t v[2 + 2 * HK], acc[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 2 + 2 * HK; ++i) v[i] = p[i];
            tap_sums<HK, 2>(v, a.k, acc);
            s_h[r * ncp + 2 * d] = acc[0];
            s_h[r * ncp + 2 * d + 1] = second ? acc[1] : acc[0];
        }
    }
    __syncthreads();
    // vertical sums + rounding + clamp in the rows the resize reads: a thread walks down one column — 4 adjacent rows of a contiguous
    // run from the 4 + 2 hk sums they share, or the two rows of an output row (rows past the staged ones belong to no output)
    if (!ylist) {
        const int ngr = (nr + 3) >> 2;
        for (int t = tid; t < ngr * ncp; t += BR_T) {
            const int g = t / ncp, j = t - g * ncp;
            uint32_t v[4 + 2 * HK], acc[4] = {1u << 15, 1u << 15, 1u << 15, 1u << 15};
#pragma unroll
            for (int i = 0; i < 4 + 2 * HK; ++i) v[i] = s_h[min(4 * g + i, sr - 1) * ncp + j];
            tap_sums<HK, 4>(v, a.k, acc);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (4 * g + u < nr) s_bl[(4 * g + u) * ncp + j] = (uint8_t)min(acc[u] >> 16, 255u);
        }
    } else {
        for (int t = tid; t < nth * ncp; t += BR_T) {
            const int e = t / ncp, j = t - e * ncp;
            const int r0 = s_yt[e].x, second = s_yt[e].y;
            uint32_t v[2 + 2 * HK], acc[2] = {1u << 15, 1u << 15};
#pragma unroll
            for (int i = 0; i < 2 + 2 * HK; ++i) v[i] = s_h[min(r0 + i, sr - 1) * ncp + j];
            tap_sums<HK, 2>(v, a.k, acc);
            s_bl[2 * e * ncp + j] = (uint8_t)min(acc[0] >> 16, 255u);
            s_bl[(2 * e + 1) * ncp + j] = (uint8_t)min((second ? acc[1] : acc[0]) >> 16, 255u);
        }
    }
    __syncthreads();
    uint8_t* out = a.dst + (size_t)b * dheight * dpitch;
    for (int t = tid; t < (th << a.tw_log); t += BR_T) {
        const int lx = t & (tw - 1), ly = t >> a.tw_log;
        if (lx >= ntw || ly >= nth) continue;
        const int4 xt = s_xt[lx], yt = s_yt[ly];
        const int a0 = xt.z, a1 = xt.w, b0 = yt.z, b1 = yt.w;
        const int jx0 = xlist ? 2 * lx : xt.x, jx1 = xlist ? 2 * lx + 1 : xt.x + xt.y;
        const int qy0 = ylist ? 2 * ly : yt.x, qy1 = ylist ? 2 * ly + 1 : yt.x + yt.y;
        const int S0 = (int)s_bl[qy0 * ncp + jx0] * a0 + (int)s_bl[qy0 * ncp + jx1] * a1;
        const int S1 = (int)s_bl[qy1 * ncp + jx0] * a0 + (int)s_bl[qy1 * ncp + jx1] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        out[(size_t)(dy0 + ly) * dpitch + dx0 + lx] = (uint8_t)min(max(v, 0), 255);
    }
}

}  // namespace

void launch_blur_resize_u8(hipStream_t s, int B, int scols, int srows, int dcols, int drows, const uint8_t* src, uint8_t* dst, double scale,
                           int radius, const int* weights, const BlurResizePlan& p, const LsdSizeRow* sz, int n_sz) {
    BlurResizeArgs a{};
    a.B = B; a.scols = scols; a.srows = srows; a.dcols = dcols; a.drows = drows;
    a.tw_log = p.tw_log; a.th_log = p.th_log; a.lds_bytes = p.lds_bytes;
    a.step_x = a.step_y = 1.0 / scale;
    a.src = src; a.dst = dst;
    for (int i = 0; i < 1 + 2 * radius; ++i) a.k[i] = weights[i];
    const int tw = 1 << p.tw_log, th = 1 << p.th_log;
    const dim3 grid((dcols + tw - 1) / tw, (drows + th - 1) / th, B);
#define BR_KERNELS(M)                                                                                                             \
    {lsd_blur_resize_kernel<0, M>,  lsd_blur_resize_kernel<1, M>,  lsd_blur_resize_kernel<2, M>,  lsd_blur_resize_kernel<3, M>,   \
     lsd_blur_resize_kernel<4, M>,  lsd_blur_resize_kernel<5, M>,  lsd_blur_resize_kernel<6, M>,  lsd_blur_resize_kernel<7, M>,   \
     lsd_blur_resize_kernel<8, M>,  lsd_blur_resize_kernel<9, M>,  lsd_blur_resize_kernel<10, M>, lsd_blur_resize_kernel<11, M>,  \
     lsd_blur_resize_kernel<12, M>, lsd_blur_resize_kernel<13, M>, lsd_blur_resize_kernel<14, M>, lsd_blur_resize_kernel<15, M>}
    if (sz && n_sz > 0) {  // one size per image: the slot's grid, tile and LDS
        typedef void (*kernel_t)(BlurResizeArgs, LsdTable<true>);
        static const kernel_t kernels[STVO_LSD_MAX_RADIUS + 1] = BR_KERNELS(true);
        hipLaunchKernelGGL(kernels[radius], grid, dim3(BR_T), (size_t)p.lds_bytes, s, a, LsdTable<true>{sz, n_sz});
        return;
    }
    typedef void (*kernel_t)(BlurResizeArgs, LsdTable<false>);
    static const kernel_t kernels[STVO_LSD_MAX_RADIUS + 1] = BR_KERNELS(false);
    hipLaunchKernelGGL(kernels[radius], grid, dim3(BR_T), (size_t)p.lds_bytes, s, a, LsdTable<false>{});
#undef BR_KERNELS
}

}  // namespace stvo
