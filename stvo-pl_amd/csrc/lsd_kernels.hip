// lsd_kernels.hip — the LSD key-line detector on gfx950: what the reference obtains from
//     lsd->detect(img, lines, Config::lsdScale(), 1, opts)  + the top-N cut by response   (/root/reference/src/stereoFrame.cpp:219-240)
// through LSDDetectorC::detectImpl (3rdparty/line_descriptor/src/LSDDetector_custom.cpp:227-325) and cv::LineSegmentDetector.
// The detector core is third-party code that is not under /root/reference: the semantics are those of oracle/stvo_lsd_oracle.c
// (restated from the published algorithm, parity unpinned), against which these kernels are bit-exact (tests/test_gpu_lsd.py).
//
//   blur + resize        the scaled image (cv::GaussianBlur (1 + 2h) x (1 + 2h) + cv::resize on 8-bit data): for h = 3 (every shipped
//                        yaml) orb_kernels.hip's two kernels, for every other radius 0 .. 15 lsd_scale_kernels.hip's fused one
//   lsd_gradient_kernel  ll_angle: 2 x 2 gradient, norm, level-line angle (fastAtan2, degrees), the float cos / sin a pixel
//                        contributes to a region angle, the largest squared gradient of the image (integer atomic max)
//   lsd_hist / lsd_scan / lsd_scatter_kernel   the pseudo-ordering: the defined pixels by bin of the gradient norm, highest bin first,
//                        row-major inside a bin (oracle note (1)) — a stable counting sort written here (until round 5: rocPRIM's radix sort)
//   the search           region_grow + region2rect for every unused seed in that order.  Inherently sequential per image — whether a
//                        pixel joins depends on the running region angle, which changes with every pixel added, and on what all
//                        earlier regions took.  Inside a wave the work of one step is spread over the lanes: the 9 neighbours of
//                        7 consecutive region points are fetched by 63 lanes at once (one memory round trip per 7 points) and
//                        then resolved in the oracle's order; the sums of region2rect are accumulated strictly in region order
//                        (lane-parallel products, serial additions), so every rounding is the oracle's.  Each job is ONE routine:
//                          lsd_angle_dist    isAligned's distance of two angles
//                          lsd_grow_plain    region_grow, candidates one after the other (the oracle's loop as it stands)
//                          lsd_grow_fast     region_grow, a sub-group's candidates by guess + verification (same regions)
//                          lsd_region2rect   the rectangle; its ordered sums through LDS chains (add_ordered) or v_readlane
//                          lsd_segment       rectangle -> end points in the input image
//                        and three kernels say who calls them:
//   lsd_grow_kernel      ONE wavefront walks an image, the batch supplies the parallelism: lsd_grow_fast + LDS chains
//   lsd_grow_xcd_kernel  the same search for batches of <= 128 images as an exact speculate / commit protocol over the CUs of one XCD per
//                        image: a committing wave (LDS bitmap), a dispatcher, a feeder, speculating workgroups (9 ms instead of 63 per
//                        image); the committer and the speculating waves grow with lsd_grow_fast
//   lsd_grow_refine_kernel  one wave per image on lsd_grow_plain + v_readlane sums, for every batch size.  <REFINE = true>: lsd_refine = 1
//                        (LSD_REFINE_STD) — a sparse region gives its pixels back, is grown again under a tolerance from the angles near
//                        its seed, then cut back by radius (flags that turn off break the strike-off and the speculation of the other
//                        forms).  <REFINE = false>: STVO_LSD_GROW=0, the in-library cross-check of the fast routines
//                        The three take a bool PROF: the <PROF = true> instances carry the developer's cycle counters and debug rows
//                        (LsdProbe) and run only while stvo_lsd_debug has them switched on; the shipped instances hold none of it
//   lsd_keylines_kernel  the wrapper: checkLineExtremes, length, min_length, KeyLine fields (numOfPixels = the CLIPPED cv::LineIterator
//                        count), top-N by response (stable)
// Every kernel is a template on MIXED: the MIXED instances read their image's row of a size table (one image size and minimum length
// per image, stvo_lsd_set_image_sizes, csrc/lsd_sizes.h), the others are the kernels as they were.  Which search kernel a detection
// launches is decided in ONE place, csrc/lsd_route.h: under a table ONE wave per image at every batch size by default (lsd_grow_kernel /
// lsd_grow_refine_kernel), or — stvo_lsd_set_table_route(STVO_LSD_TABLE_BY_BATCH) — the no-table rule, lsd_grow_xcd_kernel<false, true>
// for a detector that holds the small-batch arena.
// The scaled image under a table: ORB's MIXED blur and resize at radius 3, the MIXED instance of lsd_blur_resize_kernel at every other
// radius — for a detector created with STVO_LSD_SIZES_ANY_RADIUS (lsd_scale_kernels.hip, lsd_scale_plan.h).
// Byte / integer work except where the source computes in floating point; no fused multiply-adds outside the two of the sine /
// cosine reduction, which the oracle has too.
#include <cmath>
#include <new>
#include <vector>

#include "ctx_internal.h"
#include "fast_atan2.h"
#include "frontend_layout.h"
#include "gaussian_q8.h"
#include "line_common.h"
#include "lsd_route.h"
#include "lsd_sizes.h"
#include "table_transport.h"

#pragma clang fp contract(off)

namespace stvo {
namespace {

constexpr double LSD_PI = 3.14159265358979323846;
constexpr double LSD_DEG2RAD = LSD_PI / 180;
constexpr double LSD_3_2_PI = (3 * LSD_PI) / 2;
constexpr double LSD_2_PI = 2 * LSD_PI;
constexpr uint32_t LSD_NOKEY = 0xFFFFFFFFu;
constexpr int LSD_IDX_BITS = 20;  // pixel index inside a sort key: scaled images up to 2^20 pixels
constexpr int LSD_ROWS = 16;      // image rows per workgroup of the per-pixel kernels

typedef float lsd_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ LsdPx px_ld(const LsdPx* p) {  // one 16-byte load
    const lsd_f4 v = *reinterpret_cast<const lsd_f4*>(p);
    LsdPx r;
    r.ang = v.x; r.c = v.y; r.s = v.z; r.used = __float_as_int(v.w);
    return r;
}

struct LsdDev {
    int B, w, h;               // the scaled image
    int cols, rows;            // the input image
    int n_bins, min_reg_size, seg_cap, K, nfeatures;
    double rho, prec, scale, min_length;
    const uint8_t* scaled;     // [B][h][w]
    LsdPx* px;                 // [B][w h] what the search reads of a pixel, ONE 16-byte record (one gather per neighbour instead of three)
    int32_t* k32;              // [B][w h] gx^2 + gy^2 of the defined pixels (the gradient norm is sqrt(k / 4): recomputed where it is used), -1: undefined
    uint32_t* cnt;             // [B][units][n_bins] the pseudo-ordering's counters: pixels per bin and unit, then the first rank of every bin in every unit
    uint32_t* order;           // [B][w h] (highest bin first) << 20 | pixel index of the defined pixels in the pseudo-ordering, LSD_NOKEY behind them
    int32_t* reg;              // [B][w h] the region being grown: x | y << 16
    int32_t* kmax;             // [B] largest gx^2 + gy^2 among the defined pixels, -1: none
    float4* seg;               // [B][seg_cap] (x1, y1, x2, y2) in detection order
    int32_t* n_seg;            // [B]
    int32_t* n_pass;           // [B] segments longer than min_length, before the top-N / capacity cut (stvo_lsd_counts)
    double* dbg;               // developer aid (stvo_lsd_debug), touched by the PROF instances of the search kernels only: [B][seg_cap][8] cx, cy, Ixx, Iyy, Ixy, theta, l_min, l_max, or nullptr
    // outputs of the wrapper
    stvo_keyline* lines;       // [B][K]
    float* response;           // [B][K] or nullptr
    int32_t* n_lines;          // [B]
};

// One image size per image (stvo_lsd_set_image_sizes): LsdTable<MIXED> (lsd_sizes.h), an argument of its own behind LsdDev and empty for
// the uniform instances — they take the arguments they always took.

// The image a workgroup works on.  MIXED = false: the slot itself — the kernel as it was, reading its argument.  MIXED = true: the
// kernel's own copy of its argument takes the image's sizes, smallest region and minimum length from the image's row of the table in
// place of the slot's, so the code below the call is one text for both.  Every kernel takes its image from a block index: the row is
// uniform over the workgroup and is read with scalar loads; it is clamped into the slot, which the host has validated it to fit.
// The uniform instances do not make the call (if constexpr): their code is the code they had, the argument's address never taken
// (profiles/mixed_lines_kernel_resources.txt).  LsdSlot: the slot's scaled size, taken before the call.  The per-image stride of the
// search arrays (px, k32, order, reg: the slot's w h; cnt: the slot's units) stays the slot's; INSIDE its block an image indexes them
// compactly with its own w, so the search routines keep one w for pitch and bound (std::rint is monotone: an image's scaled size, and
// with it its pixels and units, never exceed the slot's — lsd_sizes.h).  Only the gradient kernel reads the scaled image, at the
// slot's pitch.
struct LsdSlot {
    int w, h;
};
__device__ __forceinline__ void lsd_take_image(LsdDev& d, const LsdTable<true>& tab, int b) {
    const LsdSizeRow* e = tab.sz + (b % tab.n_sz);
    d.w = __builtin_amdgcn_readfirstlane(min(max(e->w, 1), d.w));
    d.h = __builtin_amdgcn_readfirstlane(min(max(e->h, 1), d.h));
    d.cols = __builtin_amdgcn_readfirstlane(min(max(e->cols, 1), d.cols));
    d.rows = __builtin_amdgcn_readfirstlane(min(max(e->rows, 1), d.rows));
    d.min_reg_size = __builtin_amdgcn_readfirstlane(e->min_reg_size);
    d.min_length = e->min_length;
}

// ll_angle: one thread per pixel of the scaled image
template <bool MIXED>
__global__ __launch_bounds__(256) void lsd_gradient_kernel(LsdDev d, LsdTable<MIXED> tab) {
    const int x = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    // a workgroup wholly outside its image has no pixel and no gradient to report: it leaves as a whole, before the reduction
    if constexpr (MIXED)
        if ((int)blockIdx.x * 256 >= d.w || (int)blockIdx.y * LSD_ROWS >= d.h) return;
    const bool in_row = x < d.w;  // (no early return: the whole wave takes part in the reduction below)
    const size_t base = (size_t)b * slot.w * slot.h;
    int kw = -1;
    // LSD_ROWS rows per workgroup: one row each made 2.8 M workgroups per 1024 images and the launch dispatch-bound (25 ms)
    for (int y = blockIdx.y * LSD_ROWS; y < min((int)(blockIdx.y + 1) * LSD_ROWS, d.h); ++y) {
    const size_t q = base + (size_t)y * d.w + (in_row ? x : 0);
    float ang = -1.f;
    float2 cs = make_float2(0.f, 0.f);
    double norm = 0.0;
    int kdef = -1;
    if (x < d.w - 1 && y < d.h - 1) {
        const uint8_t* r0 = d.scaled + base + (size_t)y * slot.w + x;  // (the scaled image keeps the slot's pitch)
        const uint8_t* r1 = r0 + slot.w;
        const int DA = (int)r1[1] - (int)r0[0], BC = (int)r0[1] - (int)r1[0];
        const int gx = DA + BC, gy = DA - BC;
        const int k = gx * gx + gy * gy;
        norm = sqrt((double)k / 4.0);
        if (!(norm <= d.rho)) {
            ang = fast_atan2_deg((float)gx, (float)-gy);
            const double a = (double)ang * LSD_DEG2RAD;
            double s, c;
            sincos_det((double)(float)a, s, c);
            cs = make_float2((float)c, (float)s);
            kdef = k;
        }
    }
    kw = max(kw, kdef);
    if (in_row) {
        lsd_f4 rec;
        rec.x = ang; rec.y = cs.x; rec.z = cs.y; rec.w = 0.f;  // (used = 0)
        *reinterpret_cast<lsd_f4*>(d.px + q) = rec;
        d.k32[q] = kdef;
    }
    }
    // the image's largest squared gradient: one atomic per wave, and only when it can raise the value
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kw = max(kw, __shfl_xor(kw, off, 64));
    if ((threadIdx.x & 63) == 0 && kw >= 0 && kw > __hip_atomic_load(&d.kmax[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&d.kmax[b], kw);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The pseudo-ordering — pixels by bin of their gradient norm, highest bin first, row-major inside a bin, undefined pixels not at all
// (src of the semantics: oracle/stvo_lsd_oracle.c note (1)) — as a stable counting sort of our own (round 6; until then a key array +
// rocPRIM's segmented radix sort: 36 of the 188 ms of 4096 images).  A wave owns a UNIT of 64 rows of 64 consecutive pixels:
//   lsd_hist_kernel     the pixels of every bin in the unit (LDS counters, wave-private);
//   lsd_scan_kernel     per image: first rank of every (bin, unit) = pixels of higher bins + pixels of the bin in earlier units; LSD_NOKEY
//                       behind the last defined pixel (the searches stop at the first batch that begins with it);
//   lsd_scatter_kernel  the unit again, row by row: a pixel's rank = the bin's running position + the lower lanes of its row with the same
//                       bin (the lanes with equal bins matched bit by bit with ballots) — stable by construction, no atomics on the way.
// The bin is (int)(norm (n_bins - 1) / max norm), norm = sqrt(k / 4) in double precision from the integer k both times.
constexpr int LSD_MAX_BINS = 2048;
__device__ __forceinline__ double lsd_bin_coef(const LsdDev& d, int b) {
    const int km = d.kmax[b];
    const double max_grad = km >= 0 ? sqrt((double)km / 4.0) : -1.0;
    return max_grad > 0 ? (double)(d.n_bins - 1) / max_grad : 0.0;
}
__device__ __forceinline__ int lsd_keybin(int k, double bin_coef, int n_bins) {
    int bin = (int)(sqrt((double)k / 4.0) * bin_coef);
    bin = bin < 0 ? 0 : (bin >= n_bins ? n_bins - 1 : bin);
    return n_bins - 1 - bin;
}

template <bool MIXED>
__global__ __launch_bounds__(256) void lsd_hist_kernel(LsdDev d, LsdTable<MIXED> tab) {
    extern __shared__ unsigned s_h[];  // [4][n_bins]
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int slot_px = slot.w * slot.h, slot_units = (slot_px + LSD_UNIT - 1) / LSD_UNIT;  // the strides of an image's blocks
    const int npx = d.w * d.h, nunits = (npx + LSD_UNIT - 1) / LSD_UNIT, unit = blockIdx.x * 4 + wv;
    if (unit >= nunits) return;  // (wave-private LDS, no workgroup barrier below)
    unsigned* h = s_h + wv * d.n_bins;
    for (int t = lane; t < d.n_bins; t += 64) h[t] = 0u;
    const double bin_coef = lsd_bin_coef(d, b);
    const int32_t* k32 = d.k32 + (size_t)b * slot_px;
#pragma unroll 8
    for (int r = 0; r < LSD_UNIT_ROWS; ++r) {
        const int i = unit * LSD_UNIT + r * 64 + lane;
        const int k = i < npx ? k32[i] : -1;
        if (k >= 0) atomicAdd(&h[lsd_keybin(k, bin_coef, d.n_bins)], 1u);
    }
    unsigned* out = d.cnt + ((size_t)b * slot_units + unit) * d.n_bins;
    for (int t = lane; t < d.n_bins; t += 64) out[t] = h[t];
}

template <bool MIXED>
__global__ __launch_bounds__(1024) void lsd_scan_kernel(LsdDev d, LsdTable<MIXED> tab) {
    __shared__ unsigned s_w[16];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int slot_px = slot.w * slot.h, slot_units = (slot_px + LSD_UNIT - 1) / LSD_UNIT;
    const int npx = d.w * d.h, nunits = (npx + LSD_UNIT - 1) / LSD_UNIT, nb = d.n_bins;
    unsigned* cnt = d.cnt + (size_t)b * slot_units * nb;
    unsigned carry = 0u;  // pixels of all the bins in front
    for (int t0 = 0; t0 < nb; t0 += 1024) {  // (n_bins <= 2048: one or two turns)
        const int bin = t0 + t;
        unsigned tot = 0u;
        if (bin < nb)
            for (int u = 0; u < nunits; ++u) tot += cnt[(size_t)u * nb + bin];
        // exclusive scan over the 1024 threads
        unsigned inc = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned v = __shfl_up(inc, off, 64);
            if (lane >= off) inc += v;
        }
        __syncthreads();  // (s_w of the previous turn has been read)
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        unsigned before = 0u, all = 0u;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const unsigned x = s_w[v];
            before += v < wv ? x : 0u;
            all += x;
        }
        unsigned run = carry + before + inc - tot;
        if (bin < nb)
            for (int u = 0; u < nunits; ++u) {
                const unsigned c = cnt[(size_t)u * nb + bin];
                cnt[(size_t)u * nb + bin] = run;
                run += c;
            }
        carry += all;
    }
    // the end mark: every reader walks the ranks in batches of 64 and stops at the first batch whose first rank holds LSD_NOKEY
    if (t < 128 && carry + (unsigned)t < (unsigned)npx) d.order[(size_t)b * slot_px + carry + t] = LSD_NOKEY;
}

template <bool MIXED>
__global__ __launch_bounds__(256) void lsd_scatter_kernel(LsdDev d, LsdTable<MIXED> tab) {
    extern __shared__ unsigned s_h[];  // [4][n_bins] the next rank of every bin, for this wave's unit
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int slot_px = slot.w * slot.h, slot_units = (slot_px + LSD_UNIT - 1) / LSD_UNIT;
    const int npx = d.w * d.h, nunits = (npx + LSD_UNIT - 1) / LSD_UNIT, unit = blockIdx.x * 4 + wv;
    if (unit >= nunits) return;  // (wave-private LDS, no workgroup barrier below)
    unsigned* h = s_h + wv * d.n_bins;
    const unsigned* first = d.cnt + ((size_t)b * slot_units + unit) * d.n_bins;
    for (int t = lane; t < d.n_bins; t += 64) h[t] = first[t];
    const double bin_coef = lsd_bin_coef(d, b);
    const int32_t* k32 = d.k32 + (size_t)b * slot_px;
    uint32_t* order = d.order + (size_t)b * slot_px;
    const unsigned long long lt = lane == 0 ? 0ull : ~0ull >> (64 - lane);
#pragma unroll 4
    for (int r = 0; r < LSD_UNIT_ROWS; ++r) {
        const int i = unit * LSD_UNIT + r * 64 + lane;
        const int k = i < npx ? k32[i] : -1;
        const bool valid = k >= 0;
        const int kb = valid ? lsd_keybin(k, bin_coef, d.n_bins) : 0;
        unsigned long long m = __ballot(valid);  // ... the lanes of the row with this lane's bin
        if (!m) continue;  // uniform
#pragma unroll
        for (int bit = 0; bit < 11; ++bit) {
            const bool one = (kb >> bit) & 1;
            const unsigned long long bb = __ballot(one);
            m &= one ? bb : ~bb;
        }
        if (valid) {
            const int rank = __builtin_popcountll(m & lt);
            const unsigned pos = h[kb] + (unsigned)rank;
            order[pos] = ((uint32_t)kb << LSD_IDX_BITS) | (uint32_t)i;
            if (rank == 0) h[kb] = pos + (unsigned)__builtin_popcountll(m);  // (the lowest lane of every bin; the read above comes first: one wave, LDS in order)
        }
    }
}

constexpr int LSD_RING = 1024;  // the most recent region points, in LDS (4 KB: the LDS must not limit the images in flight per CU)
constexpr int LSD_WRING = 256;  // the same per wave of lsd_grow_xcd_kernel
constexpr int LSD_GR = 2;       // sub-groups of 7 region points (63 lanes) fetched per round of the region growing

// The flags / the region list are written by lane 0 and read by all lanes of the SAME wave later: workgroup-scope ordering is
// what is needed — the vector L1 is write-through and shared by the CU, so such accesses are ordinary loads / stores with a wait
// for the stores in between.  (Device-scope atomics were the first version: on this part they bypass the XCD's L2, ~2 us each,
// and 512 images took 0.5 s.)
__device__ __forceinline__ int ld_coherent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_coherent(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ float readlane_f32(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
// stores of this wave are complete / later loads of this wave see them
__device__ __forceinline__ void wave_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// LDS of this wave: the writes so far before the reads that follow
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the committer of lsd_grow_xcd_kernel keeps the flags it decides on as a bitmap in LDS
__device__ __forceinline__ unsigned bit_ld(const unsigned* bits, int q) { return (__hip_atomic_load(bits + (q >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (q & 31)) & 1u; }
__device__ __forceinline__ void bit_set(unsigned* bits, int q) { (void)__hip_atomic_fetch_or(bits + (q >> 5), 1u << (q & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The developer's cycle counters and event counts (stvo_lsd_debug, tools/lsd_probe.py).  Only the PROF instances of the search
// kernels, which lsd_enqueue launches while stvo_lsd_debug has them enabled, hold any of it: for the shipped instances the type is
// empty and every call on it compiles to nothing.
template <bool PROF>
struct LsdProbe {
    long long v[16] = {};
    bool on;  // this wave measures
    __device__ explicit LsdProbe(bool on_) : on(on_) {}
    __device__ long long now() const { return on ? (long long)__builtin_readcyclecounter() : 0ll; }
    __device__ void add(int i, long long x) { v[i] += x; }
    __device__ void settle() const {  // everything in flight has arrived: what follows is timed alone (this changes what it measures)
        if (on) __builtin_amdgcn_s_waitcnt(0);
    }
};
template <>
struct LsdProbe<false> {
    __device__ explicit LsdProbe(bool) {}
    __device__ long long now() const { return 0ll; }
    __device__ void add(int, long long) {}
    __device__ void settle() const {}
};
// what a one-wave kernel counts, in the order of its two counter rows (behind the total)
enum { OW_GROW, OW_RES, OW_RECT, OW_ROUNDS, OW_ADD, OW_REGIONS, OW_BATCHES, OW_PUB, OW_ISSUE, OW_WAIT, OW_SEED, OW_N };

// isAligned: the distance of two level-line angles, folded at 3 pi / 2
__device__ __forceinline__ double lsd_angle_dist(double theta, double a) {
    double n_theta = theta - a;
    if (n_theta < 0) n_theta = -n_theta;
    if (n_theta > LSD_3_2_PI) {
        n_theta -= LSD_2_PI;
        if (n_theta < 0) n_theta = -n_theta;
    }
    return n_theta;
}

// The batch of 64 seeds a one-wave kernel is working through: lane l holds the seed of rank o0 + l.  A seed of the batch that a region
// grown from an earlier seed of the batch takes is struck off as it is taken (one compare + ballot per pixel added) — re-reading the
// flags after every region cost a memory round trip per region
struct LsdSeeds {
    int q_l;                  // the seed's pixel
    bool key_ok;              // (the last batch of an image is not full)
    unsigned long long todo;  // the seeds still to be looked at, a lane mask
};

// One round of the region growing: the next (up to) 7 LSD_GR region points — sub-group r holds points i + 7 r .. i + 7 r + 6, lane =
// 9 x point + neighbour — fetched together, then resolved sub-group after sub-group, lane after lane: the oracle's order.
//
// PLAIN region_grow from `seed` (angle ang_deg) under the tolerance tol — the direct statement of the oracle's loop: the candidates of
// a sub-group are taken one after the other.  The list goes to reg (and the ring), the size is returned.  STVO_LSD_GROW=0 and
// lsd_refine = 1 run it; the former as the in-library cross-check of the fast form below (tests/test_gpu_lsd.py runs both).
template <bool PROF>
__device__ __forceinline__ int lsd_grow_plain(LsdPx* px, int32_t* reg, int* ring, int seed, float ang_deg, int w, int h, double tol, LsdSeeds& sd,
                                              double& reg_angle, LsdProbe<PROF>& pr) {
    const int lane = threadIdx.x & 63, npx = w * h;
    const long long tg0 = pr.now();
    pr.add(OW_REGIONS, 1);
    const int sx0 = seed % w, sy0 = seed / w;
    reg_angle = (double)ang_deg * LSD_DEG2RAD;
    double sn0, cs0;
    sincos_det(reg_angle, sn0, cs0);
    float sumdx = (float)cs0, sumdy = (float)sn0;
    int n_reg = 1;
    if (lane == 0) {
        st_coherent(&px[seed].used, 1);
        st_coherent(reg, sx0 | (sy0 << 16));
        ring[0] = sx0 | (sy0 << 16);
    }
    pr.add(OW_SEED, pr.now() - tg0);
    for (int i = 0; i < n_reg;) {
        const long long tp0 = pr.now();
        wave_publish();  // lane 0's stores of the earlier rounds before the flag / list loads below
        pr.settle();
        const long long tp1 = pr.now();
        pr.add(OW_PUB, tp1 - tp0);
        const int cnt = n_reg - i < 7 * LSD_GR ? n_reg - i : 7 * LSD_GR;  // uniform
        const int slot0 = lane / 9, nb = lane - slot0 * 9;
        int qq[LSD_GR], xy[LSD_GR];
        float2 cs[LSD_GR];
        double ad[LSD_GR];
        bool cand[LSD_GR];
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            const int slot = 7 * r + slot0;
            bool valid = lane < 63 && slot < cnt && nb != 4;  // (the centre is the region point itself)
            int pxy = 0;
            if (valid) pxy = (n_reg - (i + slot) <= LSD_RING) ? ring[(i + slot) & (LSD_RING - 1)] : ld_coherent(reg + i + slot);
            const int xx = (pxy & 0xFFFF) + (nb % 3) - 1, yy = (pxy >> 16) + nb / 3 - 1;  // neighbours row by row
            valid = valid && xx >= 0 && xx < w && yy >= 0 && yy < h;
            qq[r] = valid ? yy * w + xx : 0;
            xy[r] = xx | (yy << 16);
            int u = 1;
            float a = -1.f;
            cs[r] = make_float2(0.f, 0.f);
            if (valid) {
                const LsdPx t = px_ld(px + qq[r]);
                u = t.used;
                a = t.ang;
                cs[r] = make_float2(t.c, t.s);
            }
            cand[r] = valid && u == 0 && a >= 0.f;
            ad[r] = (double)a * LSD_DEG2RAD;
        }
        const long long ti1 = pr.now();  // the loads are issued ...
        pr.settle();
        const long long tr0 = pr.now();  // ... and have arrived
        pr.add(OW_ISSUE, ti1 - tp1);
        pr.add(OW_WAIT, tr0 - ti1);
        pr.add(OW_ROUNDS, 1);
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            if (7 * r >= cnt) break;  // uniform
            int next = 0;  // lanes below `next` have had their turn
            for (;;) {
                const unsigned long long m = __ballot(cand[r] && lane >= next && lsd_angle_dist(reg_angle, ad[r]) <= tol);
                if (!m || n_reg >= npx) break;  // (the bound can only bind if a flag were lost: never write past the list)
                const int L = __builtin_ctzll(m);
                const int qL = __builtin_amdgcn_readlane(qq[r], L), xyL = __builtin_amdgcn_readlane(xy[r], L);
                const float cL = readlane_f32(cs[r].x, L), sL = readlane_f32(cs[r].y, L);
                if (lane == 0) {
                    st_coherent(&px[qL].used, 1);
                    st_coherent(reg + n_reg, xyL);
                    ring[n_reg & (LSD_RING - 1)] = xyL;
                }
                ++n_reg;
#pragma unroll
                for (int r2 = 0; r2 < LSD_GR; ++r2) cand[r2] = cand[r2] && qq[r2] != qL;  // the same pixel seen from another point of the round
                sd.todo &= ~__ballot(sd.key_ok && sd.q_l == qL);
                sumdx += cL;
                sumdy += sL;
                reg_angle = (double)fast_atan2_deg(sumdy, sumdx) * LSD_DEG2RAD;
                next = L + 1;
            }
        }
        pr.add(OW_RES, pr.now() - tr0);
        i += cnt;
        wave_lds_sync();  // the ring: lane 0's writes before the next round's reads
    }
    pr.add(OW_GROW, pr.now() - tg0);
    pr.add(OW_ADD, n_reg);
    return n_reg;
}

// FAST region_grow from `seed` (the default of every route without refinement): a sub-group's candidates are resolved by guess +
// verification instead of one after the other, and the loads of all sub-groups of a round are issued before the first is used.  Same
// results as the plain form.  Round 4, one KITTI-size image: 233 M cycles plain, 155 M fast (NOTES.md has the table of the steps in
// between).
//   MARK     (a one-wave kernel, the committer): a pixel is taken by setting its flag.  !MARK (a speculating wave): the flags are only
//            read; the wave's own pixels carry `id` in `stamp`.
//   FAR      the flag in a pixel's record is stored by ANOTHER CU: the load bypasses the vector L1.
//   BITS     (with MARK) the flags this wave decides on are a bitmap in LDS (`bits`); `used` is only written — for the waves of other CUs.
//   RING     points of the ring in LDS.
//   STRIKE   the pixels taken strike the later seeds of the batch `sd` off (else sd is not looked at).
//   SKIP_AT_CAP  what happens where a sub-group might not fit the list of `cap` entries: the sub-group is passed over, or (else) the
//            growth ends and -1 is returned.  With cap = w h the bound can only bind if a flag were lost or in an image of w + h <= 64
//            (the gradient leaves the last row and column undefined: a region has at most (w - 1)(h - 1) pixels); each caller keeps
//            the behaviour it always had.
// The list goes to `list`, the final region angle to `angle_out`, the size is returned.
template <bool MARK, bool FAR, bool BITS, int RING, bool STRIKE, bool SKIP_AT_CAP, bool PROF>
__device__ __forceinline__ int lsd_grow_fast(LsdPx* px, int32_t* stamp, int id, unsigned* bits, int32_t* list, int cap, int* ring, int seed,
                                             float seed_ang, int w, int h, double prec, LsdSeeds* sd, double& angle_out, LsdProbe<PROF>& pr) {
    const int lane = threadIdx.x & 63;
    const long long tg0 = pr.now();
    pr.add(OW_REGIONS, 1);
    const int sx0 = seed % w, sy0 = seed / w;
    double reg_angle = (double)seed_ang * LSD_DEG2RAD;
    double sn0, cs0;
    sincos_det(reg_angle, sn0, cs0);
    float sumdx = (float)cs0, sumdy = (float)sn0;
    int n_reg = 1;
    if (lane == 0) {
        if (MARK) st_coherent(&px[seed].used, 1);
        else st_coherent(stamp + seed, id);
        if (BITS) bit_set(bits, seed);
        st_coherent(list, sx0 | (sy0 << 16));
        ring[0] = sx0 | (sy0 << 16);
    }
    pr.add(OW_SEED, pr.now() - tg0);
    for (int i = 0; i < n_reg;) {
        const int cnt = n_reg - i < 7 * LSD_GR ? n_reg - i : 7 * LSD_GR;  // uniform
        const int slot0 = lane / 9, nb = lane - slot0 * 9;
        int qq[LSD_GR], xy[LSD_GR], pxyv[LSD_GR], u[LSD_GR], own[LSD_GR];
        float2 cs[LSD_GR];
        float a[LSD_GR];
        double ad[LSD_GR];
        bool val[LSD_GR];
        const long long tp0 = pr.now();
        wave_publish();  // the stores of the earlier rounds before the flag / list loads below
        pr.settle();
        const long long tp1 = pr.now();
        pr.add(OW_PUB, tp1 - tp0);
        // every sub-group's region point first, then every load, then the uses: the flag / angle / (cos, sin) loads of the sub-groups
        // overlap (one after the other they were two memory round trips per round).  Lanes without a neighbour load pixel 0 and drop
        // the values
        const bool in_ring = n_reg - i <= RING;  // uniform: the round's oldest point is still in the LDS ring
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            const int slot = 7 * r + slot0;
            val[r] = lane < 63 && slot < cnt && nb != 4;  // (the centre is the region point itself)
            const int at = val[r] ? i + slot : i;
            pxyv[r] = in_ring ? ring[at & (RING - 1)] : ld_coherent(list + at);
        }
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            const int xx = (pxyv[r] & 0xFFFF) + (nb % 3) - 1, yy = (pxyv[r] >> 16) + nb / 3 - 1;  // neighbours row by row
            val[r] = val[r] && xx >= 0 && xx < w && yy >= 0 && yy < h;
            qq[r] = val[r] ? yy * w + xx : 0;
            xy[r] = xx | (yy << 16);
            own[r] = MARK ? 0 : ld_coherent(stamp + qq[r]);
        }
        {   // the records: one 16-byte gather per sub-group
            LsdPx t[LSD_GR];
            if constexpr (FAR) {
                static_assert(LSD_GR == 2, "two loads in one statement");
                lsd_f4 v0, v1;
                asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                             : "=&v"(v0), "=&v"(v1)
                             : "v"(px + qq[0]), "v"(px + qq[1])
                             : "memory");
                t[0].ang = v0.x; t[0].c = v0.y; t[0].s = v0.z; t[0].used = __float_as_int(v0.w);
                t[1].ang = v1.x; t[1].c = v1.y; t[1].s = v1.z; t[1].used = __float_as_int(v1.w);
            } else {
#pragma unroll
                for (int r = 0; r < LSD_GR; ++r) t[r] = px_ld(px + qq[r]);
            }
#pragma unroll
            for (int r = 0; r < LSD_GR; ++r) {
                u[r] = BITS ? (int)bit_ld(bits, qq[r]) : t[r].used;
                a[r] = t[r].ang;
                cs[r] = make_float2(t[r].c, t[r].s);
            }
        }
        // Every per-lane flag is kept as a 64-bit lane mask in scalar registers (they are compare results to begin with).
        unsigned long long cand_m[LSD_GR];
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            cand_m[r] = __ballot(val[r] && u[r] == 0 && (MARK || own[r] != id) && a[r] >= 0.f);
            ad[r] = (double)a[r] * LSD_DEG2RAD;
        }
        const long long ti1 = pr.now();  // the loads are issued ...
        pr.settle();
        const long long tr0 = pr.now();  // ... and have arrived
        pr.add(OW_ISSUE, ti1 - tp1);
        pr.add(OW_WAIT, tr0 - ti1);
        pr.add(OW_ROUNDS, 1);
        // Guess + verification (tools/experiments/lsd_resolve_model.c has the CPU model and the argument).  Only the two float
        // additions per pixel depend on the order; the ~30 operations of the angle update run for all lanes at once:
        //   A   = the lanes aligned with the angle at the start of the sub-group
        //   A'  = A walked from the lowest lane: a lane taken removes the later lanes that hold the same pixel
        //   lane k: sums_k = start sums + (cos, sin) of A's lanes below k, added in lane order; angle_k = fastAtan2(sums_k), or
        //           the start angle if A' has no lane below k;  dup_k = a lane of A' below k holds the same pixel
        //   D   = the lanes aligned with their angle_k and not dup.  D == A': A' is what the sequential loop accepts
        //         (induction over the lanes); else the lanes below the first difference m are final, lane m's decision is
        //         D[m]: again with A = A' below m | D from m on (2 % of the sub-groups of a KITTI-size scene).
        unsigned long long key_m = 0ull;
        if constexpr (STRIKE) key_m = __ballot(sd->key_ok);
#pragma unroll
        for (int r = 0; r < LSD_GR; ++r) {
            if (7 * r >= cnt) break;  // uniform
            unsigned long long A = __ballot(lsd_angle_dist(reg_angle, ad[r]) <= prec) & cand_m[r];
            if (!A) continue;
            if (n_reg + 64 > cap) {  // uniform
                if constexpr (SKIP_AT_CAP) continue;
                else return -1;
            }
            unsigned long long acc, kill, hit_m[LSD_GR];
            float sx, sy;
            double th;
            for (;;) {
                unsigned long long rem = A, dup_m = 0ull;
                acc = 0ull;
                kill = 0ull;
#pragma unroll
                for (int r2 = 0; r2 < LSD_GR; ++r2) hit_m[r2] = 0ull;
                sx = sumdx;
                sy = sumdy;
                while (rem) {  // uniform: the lanes of the guess, lowest first
                    const int j = __builtin_ctzll(rem);
                    const int qj = __builtin_amdgcn_readlane(qq[r], j);
                    const float cj = readlane_f32(cs[r].x, j), sj = readlane_f32(cs[r].y, j);
                    const unsigned long long later = j == 63 ? 0ull : ~0ull << (j + 1);
                    const unsigned long long same = __ballot(qq[r] == qj);
                    acc |= 1ull << j;
                    rem &= ~same;  // lane j itself and the later lanes that hold the same pixel
                    dup_m |= same & later;
                    const float nx = sx + cj, ny = sy + sj;  // (a select, not a masked addition of zero: x + 0 is not x for x = -0)
                    const bool is_later = lane > j;
                    sx = is_later ? nx : sx;
                    sy = is_later ? ny : sy;
                    if constexpr (STRIKE) kill |= __ballot(sd->q_l == qj);
#pragma unroll
                    for (int r2 = 0; r2 < LSD_GR; ++r2)
                        if (r2 > r) hit_m[r2] |= __ballot(qq[r2] == qj);
                }
                const bool any = lane > __builtin_ctzll(acc);
                th = any ? (double)fast_atan2_deg(sy, sx) * LSD_DEG2RAD : reg_angle;
                const unsigned long long D = __ballot(lsd_angle_dist(th, ad[r]) <= prec) & cand_m[r] & ~dup_m;
                if (D == acc) break;
                const unsigned long long below = (1ull << __builtin_ctzll(D ^ acc)) - 1ull;
                A = (acc & below) | (D & ~below);  // (never empty: the lowest lane of a guess sees the start angle, as the guess did)
            }
            // acc is the sequential result: every accepted lane stores its own pixel, in lane order
            if ((acc >> lane) & 1ull) {
                const int idx = n_reg + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(acc >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)acc, 0u));
                if (MARK) st_coherent(&px[qq[r]].used, 1);
                else st_coherent(stamp + qq[r], id);
                if (BITS) bit_set(bits, qq[r]);
                st_coherent(list + idx, xy[r]);
                ring[idx & (RING - 1)] = xy[r];
            }
            n_reg += __builtin_popcountll(acc);
            sumdx = readlane_f32(sx, 63);  // lane 63 is never a candidate: its sums are the sums over all of acc
            sumdy = readlane_f32(sy, 63);
            reg_angle = readlane_f64(th, 63);
            if constexpr (STRIKE) sd->todo &= ~(kill & key_m);
#pragma unroll
            for (int r2 = 0; r2 < LSD_GR; ++r2)
                if (r2 > r) cand_m[r2] &= ~hit_m[r2];
        }
        pr.add(OW_RES, pr.now() - tr0);
        i += cnt;
        wave_lds_sync();  // the ring: this round's writes before the next round's reads
    }
    pr.add(OW_GROW, pr.now() - tg0);
    pr.add(OW_ADD, n_reg);
    angle_out = reg_angle;
    return n_reg;
}

// region2rect: what the rectangle of a region is made of
struct LsdRect {
    double cx, cy;         // the centre of mass
    double Ixx, Iyy, Ixy;  // the inertia sums
    double theta, dx, dy;  // the direction and its cos / sin
    double l_min, l_max;   // the region's extent along it
    double width;          // and across it, at least 1 (lsd_refine = 1 asks for it)
};

// The three ordered sums of a pass of region2rect as three independent chains: lane l < 3 adds row l of `term` ([3][64] doubles of
// LDS) term by term into its `chain` (one LDS read + one addition per region point instead of six v_readlane + three additions)
__device__ __forceinline__ void add_ordered(double (*term)[64], double t0, double t1, double t2, int cn, double& chain) {
    const int lane = threadIdx.x & 63;
    term[0][lane] = t0;
    term[1][lane] = t1;
    term[2][lane] = t2;
    wave_lds_sync();
    if (lane < 3) {
        const double* row = term[lane];
#pragma unroll 8
        for (int k = 0; k < cn; ++k) chain += row[k];
    }
    wave_lds_sync();  // the reads before the next chunk's writes
}

// region2rect of list[0 .. n_reg): every sum strictly in region order, so that every addition rounds as the oracle's.  The lanes form
// the products; the additions are serial — CHAINS (the fast form): through add_ordered, else through v_readlane.
template <bool CHAINS>
__device__ __forceinline__ LsdRect lsd_region2rect(const int32_t* list, int n_reg, const int32_t* __restrict__ k32, int w, double reg_angle, double prec,
                                                   double (*term)[64]) {
    const int lane = threadIdx.x & 63;
    wave_publish();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;  // the running sums (CHAINS: s0 is the lane's chain)
    auto add3 = [&](double t0, double t1, double t2, int cn) {
        if constexpr (CHAINS) {
            add_ordered(term, t0, t1, t2, cn, s0);
        } else {
            for (int k = 0; k < cn; ++k) {
                s0 += readlane_f64(t0, k);
                s1 += readlane_f64(t1, k);
                s2 += readlane_f64(t2, k);
            }
        }
    };
    auto take3 = [&](double& a, double& b, double& c) {
        a = CHAINS ? readlane_f64(s0, 0) : s0;
        b = CHAINS ? readlane_f64(s0, 1) : s1;
        c = CHAINS ? readlane_f64(s0, 2) : s2;
        s0 = s1 = s2 = 0.0;
    };
    LsdRect rc;
    for (int c0 = 0; c0 < n_reg; c0 += 64) {
        const int t = c0 + lane, cn = n_reg - c0 < 64 ? n_reg - c0 : 64;
        int pxy = 0;
        double wgt = 0.0;
        if (t < n_reg) {
            pxy = ld_coherent(list + t);
            wgt = sqrt((double)k32[(pxy >> 16) * w + (pxy & 0xFFFF)] / 4.0);  // the gradient norm (ll_angle's expression)
        }
        add3((double)(pxy & 0xFFFF) * wgt, (double)(pxy >> 16) * wgt, wgt, cn);
    }
    double X, Y, S;
    take3(X, Y, S);
    const double cx = X / S, cy = Y / S;
    for (int c0 = 0; c0 < n_reg; c0 += 64) {
        const int t = c0 + lane, cn = n_reg - c0 < 64 ? n_reg - c0 : 64;
        double t_xx = 0.0, t_yy = 0.0, t_xy = 0.0;
        if (t < n_reg) {
            const int pxy = ld_coherent(list + t);
            const double wgt = sqrt((double)k32[(pxy >> 16) * w + (pxy & 0xFFFF)] / 4.0);
            const double ddx = (double)(pxy & 0xFFFF) - cx, ddy = (double)(pxy >> 16) - cy;
            t_xx = ddy * ddy * wgt;
            t_yy = ddx * ddx * wgt;
            t_xy = ddx * ddy * wgt;
        }
        add3(t_xx, t_yy, -t_xy, cn);  // (a - b and a + (-b) round alike)
    }
    double Ixx, Iyy, Ixy;
    take3(Ixx, Iyy, Ixy);
    const double lambda = 0.5 * (Ixx + Iyy - sqrt((Ixx - Iyy) * (Ixx - Iyy) + 4.0 * Ixy * Ixy));
    double theta = (fabs(Ixx) > fabs(Iyy)) ? (double)fast_atan2_deg((float)(lambda - Ixx), (float)Ixy)
                                           : (double)fast_atan2_deg((float)Ixy, (float)(lambda - Iyy));
    theta *= LSD_DEG2RAD;
    {
        double diff = theta - reg_angle;  // angle_diff
        while (diff <= -LSD_PI) diff += LSD_2_PI;
        while (diff > LSD_PI) diff -= LSD_2_PI;
        if (fabs(diff) > prec) theta += LSD_PI;
    }
    double dx, dy;
    sincos_det(theta, dy, dx);
    double l_min = 0.0, l_max = 0.0, w_min = 0.0, w_max = 0.0;
    for (int t = lane; t < n_reg; t += 64) {
        const int pxy = ld_coherent(list + t);
        const double rdx = (double)(pxy & 0xFFFF) - cx, rdy = (double)(pxy >> 16) - cy;
        const double l = rdx * dx + rdy * dy, ww = -rdx * dy + rdy * dx;
        l_max = l > l_max ? l : l_max;
        l_min = l < l_min ? l : l_min;
        w_max = ww > w_max ? ww : w_max;
        w_min = ww < w_min ? ww : w_min;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // maxima / minima: any order
        const double a0 = __shfl_xor(l_max, off, 64), a1 = __shfl_xor(l_min, off, 64), a2 = __shfl_xor(w_max, off, 64), a3 = __shfl_xor(w_min, off, 64);
        l_max = a0 > l_max ? a0 : l_max;
        l_min = a1 < l_min ? a1 : l_min;
        w_max = a2 > w_max ? a2 : w_max;
        w_min = a3 < w_min ? a3 : w_min;
    }
    rc.cx = cx; rc.cy = cy; rc.Ixx = Ixx; rc.Iyy = Iyy; rc.Ixy = Ixy; rc.theta = theta; rc.dx = dx; rc.dy = dy;
    rc.l_min = l_min; rc.l_max = l_max;
    rc.width = w_max - w_min < 1.0 ? 1.0 : w_max - w_min;  // (where only the segment is wanted, none of the width survives in the code)
    return rc;
}

// the end points of a rectangle's axis, in the scaled image
__device__ __forceinline__ void lsd_rect_ends(const LsdRect& rc, double& x1, double& y1, double& x2, double& y2) {
    x1 = rc.cx + rc.l_min * rc.dx; y1 = rc.cy + rc.l_min * rc.dy; x2 = rc.cx + rc.l_max * rc.dx; y2 = rc.cy + rc.l_max * rc.dy;
}
// rect -> the segment in the input image: pixel centres, 1 / scale
__device__ __forceinline__ float4 lsd_segment(const LsdRect& rc, double scale) {
    double x1, y1, x2, y2;
    lsd_rect_ends(rc, x1, y1, x2, y2);
    x1 += 0.5; y1 += 0.5; x2 += 0.5; y2 += 0.5;
    if (scale != 1) {
        x1 /= scale; y1 /= scale; x2 /= scale; y2 /= scale;
    }
    return make_float4((float)x1, (float)y1, (float)x2, (float)y2);
}

// what a one-wave kernel does with a rectangle: segment n_seg of image b — and, PROF, the rectangle's row for stvo_lsd_debug
template <bool PROF>
__device__ __forceinline__ void lsd_store_segment(const LsdDev& d, int b, int n_seg, const LsdRect& rc) {
    const float4 sg = lsd_segment(rc, d.scale);
    if ((threadIdx.x & 63) != 0 || n_seg >= d.seg_cap) return;
    d.seg[(size_t)b * d.seg_cap + n_seg] = sg;
    if constexpr (PROF) {
        double* q = d.dbg + ((size_t)b * d.seg_cap + n_seg) * 8;
        q[0] = rc.cx; q[1] = rc.cy; q[2] = rc.Ixx; q[3] = rc.Iyy; q[4] = rc.Ixy; q[5] = rc.theta; q[6] = rc.l_min; q[7] = rc.l_max;
    }
}
// tools/lsd_probe.py: the counters of image 0's wave in the last 16 doubles of image 0's block
__device__ __forceinline__ void lsd_store_counters(const LsdDev& d, int b, const LsdProbe<true>& pr, long long t_begin) {
    if ((threadIdx.x & 63) != 0 || b != 0) return;
    double* q = d.dbg + ((size_t)d.seg_cap - 2) * 8;
    q[0] = (double)(pr.now() - t_begin);
    for (int i = 0; i < OW_N; ++i) q[1 + i] = (double)pr.v[i];
}

// The search, ONE wave per image: the batch loop over the seeds in their pseudo-order, the fast growth, region2rect with its sums from
// LDS.  The default where lsd_grow_xcd_kernel does not run (batches above LSD_WAVES_MAX_B images, STVO_LSD_WAVES=0).
template <bool PROF, bool MIXED>
__global__ __launch_bounds__(64) void lsd_grow_kernel(LsdDev d, LsdTable<MIXED> tab) {
    __shared__ int s_ring[LSD_RING];
    __shared__ double s_term[3][64];  // region2rect: the terms of one chunk
    const int b = blockIdx.x, lane = threadIdx.x;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int w = d.w, h = d.h, npx = w * h;
    const size_t base = (size_t)b * (slot.w * slot.h);
    LsdPx* px = d.px + base;
    const int32_t* __restrict__ k32 = d.k32 + base;
    const uint32_t* __restrict__ order = d.order + base;
    int32_t* reg = d.reg + base;
    int n_seg = 0;
    LsdProbe<PROF> pr(true);
    const long long t_begin = pr.now();
    for (int o0 = 0; o0 < npx; o0 += 64) {
        pr.add(OW_BATCHES, 1);
        const uint32_t key = o0 + lane < npx ? order[o0 + lane] : LSD_NOKEY;
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)key) == LSD_NOKEY) break;  // sorted: only undefined pixels from here on
        LsdSeeds sd;
        sd.q_l = (int)(key & ((1u << LSD_IDX_BITS) - 1u));
        sd.key_ok = key != LSD_NOKEY;
        const LsdPx seed_l = px_ld(px + (sd.key_ok ? sd.q_l : 0));  // the seeds' angles, fetched with the batch
        const float ang_l = sd.key_ok ? seed_l.ang : -1.f;
        sd.todo = __ballot(sd.key_ok && seed_l.used == 0);
        while (sd.todo) {
            const int j = __builtin_ctzll(sd.todo);
            sd.todo &= sd.todo - 1ull;
            const int seed = __builtin_amdgcn_readlane(sd.q_l, j);
            double reg_angle;
            const int n_reg = lsd_grow_fast<true, false, false, LSD_RING, true, true>(px, nullptr, 0, nullptr, reg, npx, s_ring, seed, readlane_f32(ang_l, j),
                                                                                      w, h, d.prec, &sd, reg_angle, pr);
            if (n_reg < d.min_reg_size) continue;
            const long long tq0 = pr.now();
            lsd_store_segment<PROF>(d, b, n_seg, lsd_region2rect<true>(reg, n_reg, k32, w, reg_angle, d.prec, s_term));
            ++n_seg;
            pr.add(OW_RECT, pr.now() - tq0);
        }
    }
    if (lane == 0) d.n_seg[b] = n_seg;
    if constexpr (PROF) lsd_store_counters(d, b, pr, t_begin);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The plain search, one wave per image for every batch size: the direct statement of the oracle's loops.
//   !REFINE  STVO_LSD_GROW=0: the cross-check of the fast forms.
//   REFINE   lsd_refine = 1 (LSD_REFINE_STD; oracle/stvo_lsd_oracle.c: refine_region / reduce_region_radius): a region too sparse for
//            its rectangle is given back (its pixels are FREE again), grown once more from the same seed under a tolerance of twice
//            the standard deviation of the angles near the seed and, if still too sparse, cut back to 75 % of its radius until it is
//            dense enough or gone.  Flags that turn OFF break what the other forms of the search rely on (a batch's seeds struck off
//            for good, speculation against flags that only ever turn on), so the mode runs here whatever the batch.  No shipped
//            configuration uses it (config/*.yaml: lsd_refine : 0); it is there so that a caller who sets it gets the detector it
//            asked for rather than an error.
template <bool REFINE, bool PROF, bool MIXED>
__global__ __launch_bounds__(64) void lsd_grow_refine_kernel(LsdDev d, const double density_th, LsdTable<MIXED> tab) {
    __shared__ int s_ring[LSD_RING];
    const int b = blockIdx.x, lane = threadIdx.x;
    const LsdSlot slot{d.w, d.h};
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int w = d.w, h = d.h, npx = w * h;
    const size_t base = (size_t)b * (slot.w * slot.h);
    LsdPx* px = d.px + base;
    const int32_t* __restrict__ k32 = d.k32 + base;
    const uint32_t* __restrict__ order = d.order + base;
    int32_t* reg = d.reg + base;
    const double prec = d.prec;
    int n_seg = 0;
    LsdProbe<PROF> pr(true);
    const long long t_begin = pr.now();
    auto dist_sq = [](double x1, double y1, double x2, double y2) { return (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1); };
    auto density_of = [&](const LsdRect& rc, int n_reg) {
        double x1, y1, x2, y2;
        lsd_rect_ends(rc, x1, y1, x2, y2);
        return (double)n_reg / (sqrt(dist_sq(x1, y1, x2, y2)) * rc.width);
    };
    for (int o0 = 0; o0 < npx; o0 += 64) {
        pr.add(OW_BATCHES, 1);
        const uint32_t key = o0 + lane < npx ? order[o0 + lane] : LSD_NOKEY;
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)key) == LSD_NOKEY) break;  // sorted: only undefined pixels from here on
        LsdSeeds sd;
        sd.q_l = (int)(key & ((1u << LSD_IDX_BITS) - 1u));
        sd.key_ok = key != LSD_NOKEY;
        if constexpr (REFINE) wave_publish();  // (flags the last batch turned off)
        const LsdPx seed_l = px_ld(px + (sd.key_ok ? sd.q_l : 0));  // the seeds' angles, fetched with the batch
        const float ang_l = sd.key_ok ? seed_l.ang : -1.f;
        sd.todo = __ballot(sd.key_ok && seed_l.used == 0);
        while (sd.todo) {
            const int j = __builtin_ctzll(sd.todo);
            sd.todo &= sd.todo - 1ull;
            const int seed = __builtin_amdgcn_readlane(sd.q_l, j);
            const float seed_ang = readlane_f32(ang_l, j);
            double reg_angle;
            int n_reg = lsd_grow_plain(px, reg, s_ring, seed, seed_ang, w, h, prec, sd, reg_angle, pr);
            if (n_reg < d.min_reg_size) continue;
            const long long tq0 = pr.now();
            LsdRect rc = lsd_region2rect<false>(reg, n_reg, k32, w, reg_angle, prec, nullptr);
            if constexpr (REFINE) {
                double density = density_of(rc, n_reg);
                if (!(density >= density_th)) {
                    // ---- refine: the angles near the seed (within the rectangle's width), every pixel of the region free again ----
                    const int xy0 = ld_coherent(reg);
                    const double xc = (double)(xy0 & 0xFFFF), yc = (double)(xy0 >> 16);
                    const double ang_c = (double)seed_ang * LSD_DEG2RAD;
                    double sum = 0.0, s_sum = 0.0;
                    int n = 0;
                    for (int c0 = 0; c0 < n_reg; c0 += 64) {
                        const int t = c0 + lane, cn = n_reg - c0 < 64 ? n_reg - c0 : 64;
                        bool in = false;
                        double ang_d = 0.0;
                        if (t < n_reg) {
                            const int pxy = ld_coherent(reg + t);
                            const int q = (pxy >> 16) * w + (pxy & 0xFFFF);
                            const LsdPx tq = px_ld(px + q);
                            st_coherent(&px[q].used, 0);
                            in = sqrt(dist_sq(xc, yc, (double)(pxy & 0xFFFF), (double)(pxy >> 16))) < rc.width;
                            double diff = (double)tq.ang * LSD_DEG2RAD - ang_c;  // angle_diff_signed
                            while (diff <= -LSD_PI) diff += LSD_2_PI;
                            while (diff > LSD_PI) diff -= LSD_2_PI;
                            ang_d = diff;
                        }
                        const double sq = ang_d * ang_d;
                        const unsigned long long in_m = __ballot(in);
                        for (int k = 0; k < cn; ++k)
                            if ((in_m >> k) & 1ull) {  // uniform
                                sum += readlane_f64(ang_d, k);
                                s_sum += readlane_f64(sq, k);
                                ++n;
                            }
                    }
                    const double mean_angle = sum / (double)n;
                    const double tau = 2.0 * sqrt((s_sum - 2.0 * mean_angle * sum) / (double)n + mean_angle * mean_angle);
                    n_reg = lsd_grow_plain(px, reg, s_ring, seed, seed_ang, w, h, tau, sd, reg_angle, pr);
                    bool gone = n_reg < 2;
                    if (!gone) {
                        rc = lsd_region2rect<false>(reg, n_reg, k32, w, reg_angle, prec, nullptr);
                        density = density_of(rc, n_reg);
                        if (density < density_th) {
                            // ---- reduce_region_radius: points farther than the (shrinking) radius from the seed leave, the LAST point of the
                            // list takes a leaving point's place (and is looked at next) — one point after the other, as the oracle does
                            double ex1, ey1, ex2, ey2;
                            lsd_rect_ends(rc, ex1, ey1, ex2, ey2);
                            const double r1 = dist_sq(xc, yc, ex1, ey1), r2 = dist_sq(xc, yc, ex2, ey2);
                            double rad_sq = r1 > r2 ? r1 : r2;
                            while (density < density_th) {
                                rad_sq *= 0.75 * 0.75;
                                wave_publish();
                                for (int c0 = 0; c0 < n_reg; c0 += 64) {
                                    const int t = c0 + lane;
                                    const int pxy = t < n_reg ? ld_coherent(reg + t) : 0;
                                    const bool far = t < n_reg && dist_sq(xc, yc, (double)(pxy & 0xFFFF), (double)(pxy >> 16)) > rad_sq;
                                    unsigned long long far_m = __ballot(far);
                                    while (far_m) {
                                        const int k = __builtin_ctzll(far_m);
                                        far_m &= far_m - 1ull;
                                        const int i = c0 + k;
                                        if (i >= n_reg) break;  // (the list has shrunk below this position: its point left as a LAST point)
                                        int out_xy = __builtin_amdgcn_readlane(pxy, k);
                                        for (;;) {  // the point at position i leaves; the last point moves in and is tested in turn
                                            if (lane == 0) st_coherent(&px[(out_xy >> 16) * w + (out_xy & 0xFFFF)].used, 0);
                                            --n_reg;
                                            if (i >= n_reg) break;  // (it was the last point itself)
                                            const int last_xy = __builtin_amdgcn_readfirstlane(ld_coherent(reg + n_reg));
                                            if (!(dist_sq(xc, yc, (double)(last_xy & 0xFFFF), (double)(last_xy >> 16)) > rad_sq)) {
                                                if (lane == 0) st_coherent(reg + i, last_xy);
                                                break;
                                            }
                                            out_xy = last_xy;  // the point that moved in is too far as well: it leaves from position i
                                        }
                                    }
                                    wave_publish();  // (a later chunk may hold positions this one has just filled)
                                }
                                if (n_reg < 2) {
                                    gone = true;
                                    break;
                                }
                                rc = lsd_region2rect<false>(reg, n_reg, k32, w, reg_angle, prec, nullptr);
                                density = density_of(rc, n_reg);
                            }
                        }
                    }
                    // flags have been turned off: the batch's later seeds as they stand now
                    wave_publish();
                    const int u_now = sd.key_ok ? ld_coherent(&px[sd.q_l].used) : 1;
                    sd.todo = __ballot(sd.key_ok && lane > j && u_now == 0);
                    if (gone) continue;
                }
            }
            lsd_store_segment<PROF>(d, b, n_seg, rc);
            ++n_seg;
            pr.add(OW_RECT, pr.now() - tq0);
        }
    }
    if (lane == 0) d.n_seg[b] = n_seg;
    if constexpr (PROF) lsd_store_counters(d, b, pr, t_begin);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ONE image by many waves — an EXACT asynchronous form of the search, the default for batches of <= LSD_WAVES_MAX_B images
// (STVO_LSD_WAVES=0: one wave per image there too).  The scheme is replayed on the CPU by tools/experiments/lsd_waves_sim.c.
//   the COMMITTER walks the seeds in order.  A seed with a finished PENDING region takes it if every pixel of it is still free (the
//   segment was computed by the wave that grew it), a seed another wave is growing right now is waited for (bounded), any other
//   seed — and any pending region that lost a pixel — is grown by the committer itself, flags set as it goes.
//   the SPECULATING waves grow regions of free seeds in front of the committer against the flags committed so far; a wave marks ITS
//   pixels in a stamp array of its own and leaves the flags alone.  Seeds are handed out in rank order, >= LSD_SEP px (Chebyshev)
//   from every seed in flight, at most LSD_AHEAD ranks ahead of the committer.
// Exactness: flags only turn on.  A region grown against an older state of the flags made the sequential decisions at every pixel it
// examined unless it ACCEPTED a pixel that was taken before its turn — then the validation at its turn fails and the seed is grown again.
// Output order = commit order = seed order.
// Round 5 ran this inside ONE workgroup of sixteen waves (22.8 ms per KITTI-size image: the waves share a CU's four SIMDs and a
// growth round is ~1500 cycles of dependent instructions — fifteen speculators delivered ~2.7 waves' worth of growth); round 6
// spreads it over the CUs of one XCD: lsd_grow_xcd_kernel below (9.9 ms; the oracle takes 17 ms on one host core).
constexpr int LSD_SEP = 8;            // (4 … 16 give the same ~130 failed validations per KITTI-size image, 0: 390; 24 … 32: more seeds reach the committer unclaimed)
constexpr int LSD_LOOK = 2048;       // ranks the dispatcher examines per pass, from the front
constexpr int LSD_AHEAD = 16384;     // the front's lead over the committer (ranks; ~200 seeds of a KITTI-size scene)
// Table entry of a seed: 0 = nobody's; LSD_CLAIM | wave = a speculating wave is growing it; else a finished region (lsd_entry_x)
constexpr long long LSD_CLAIM = (long long)0x8000000000000000ull;
__device__ __forceinline__ long long ld_coherent64(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_coherent64(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ long long readlane_i64(long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long readfirstlane64(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// loads that bypass the vector L1 (sc1: served by the XCD's L2) — data another CU of the same XCD stores during the launch
__device__ __forceinline__ int ld_l2(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long ld_l2_64(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---------------------------------------------------------------------------------------------------------------------------------
// The protocol above across the CUs of ONE XCD.  A workgroup is four waves, one per SIMD (84 KB of LDS at least: a CU holds one).
// Image b is served by the workgroups b, b + 8, b + 16, ... — the dispatcher of the hardware places those on one XCD:
//   workgroup b       wave 0 the COMMITTER.  One wave on its SIMD pays its issue latency for every instruction, so it executes as
//                            little as possible per region: its flags are a bitmap in LDS (the global flags are written behind, for the
//                            speculating waves), the finished regions reach it through LDS records (the feeder);
//                     wave 1 the DISPATCHER: scans the ranks in front of the committer and hands the free seeds to idle speculating
//                            waves through their mail boxes, in rank order.  The only wave that claims — with every wave scanning for
//                            itself they all find the same first candidate and beyond ~8 waves the claims serialise (measured: 33
//                            waves 38 ms, 125 waves 57 ms per image; with the dispatcher 13 ms before the two items above);
//                     wave 2 the FEEDER: for the free seeds within LSD_FEED_AHEAD ranks of the committer whose table entry shows a
//                            finished region, segment + pixel list from the L2 into a record ring in LDS, in rank order;
//   workgroups b + 8 k  four SPECULATING waves each: mail box -> lsd_grow_fast against the global flags (loads that bypass the L1) ->
//                            lsd_region2rect -> list + segment stored, waited for (vmcnt), table entry, mail box "idle".
// What the workgroups exchange lives in HBM and meets in that XCD's L2: stores are ordinary (write-through L1, the line stays in the
// L2), loads of anything another CU stores during the launch bypass the vector L1 (sc1).  The flags and the mail boxes are ADVISORY
// for a speculating wave — a stale flag costs a failed validation, never a wrong region; what the committer (or the feeder) takes on
// trust are the pixel list + segment of a finished region: stored, waited for, THEN the table entry (a workgroup-scope release does
// not wait for the stores — the first version lost a segment that way in one of two images).
// Placement is verified, never assumed: the committer publishes the id of ITS XCD (HW_REG_XCC_ID, an agent-scope store), a
// speculating workgroup that finds itself on another one leaves without announcing itself — the committer alone is the sequential
// search, so any placement gives the same segments, only later.
constexpr int LSD_XW = 4;          // waves per workgroup: one per SIMD
constexpr int LSD_X_MAXW = 125;    // waves per image at most (7 bits of a table entry; 31 speculating workgroups of an XCD's 32 CUs)
constexpr int LSD_FEED_PX = 8192;   // words of the feeder's record ring (LDS)
constexpr int LSD_FEED_Q = 256;     // records in it at most
constexpr int LSD_FEED_MAXW = 2048; // a record's pixels at most (a quarter of the ring; larger regions go through the table)
constexpr int LSD_FEED_AHEAD = 192;  // ranks the feeder runs ahead of the committer at most (further ahead most regions are still being grown: 2048: a quarter of the regions found finished, 128 - 256: 95 %)
constexpr int XC_ALIVE = 0;        // the committer's XCC id + 1 (0: it has not started)
constexpr int XC_DONE = 1;
constexpr int XC_MBOX = 64;        // [128] 64-bit mail boxes: 0 = wave v is not there, 1 = idle, else bit 62 | rank << 21 | seed pixel: grow this one
struct LsdXcd {
    int32_t* stamp;  // [B][nw][w h] (slot 0 unused)
    int32_t* wlist;  // [B][nw][w h] per wave: region after region, 4 words of segment + the pixel list
    long long* pend; // [B][w h] by rank: 0 free, LSD_CLAIM | wave, or lsd_entry_x
    int32_t* ctl;    // [B][LSD_CTL]
    int nsb;         // speculating workgroups per image; nw = 1 + nsb LSD_XW
    int feed_ahead, sep, ahead;  // LSD_FEED_AHEAD, LSD_SEP, LSD_AHEAD or their developer overrides (STVO_LSD_FEED_AHEAD / _SEP / _AHEAD)
    int multi;       // 0: the committer takes its seeds one by one (STVO_LSD_MULTI=0)
};
__device__ __forceinline__ long long lsd_entry_x(int wave, int n, int off) { return (1ll << 62) | ((long long)wave << 42) | ((long long)n << 21) | (long long)off; }

// what the committer counts (PROF), in the order of its counter rows; the dispatcher and the speculating waves have rows of their own
enum { CM_T_SELF, CM_T_WAIT, CM_T_TAKE, CM_TOOK, CM_SELF, CM_BAD, CM_WAITED, CM_FAST, CM_STALE, CM_BATCH, CM_MULTI, CM_MULTI_UNDO,
       CM_T_MULTI, CM_T_PEEK, CM_T_REFRESH, CM_MULTI_TRY };
enum { DP_ITER, DP_CHUNKS, DP_GIVEN, DP_NOIDLE, DP_BLOCKED, DP_N };
enum { SP_BUSY, SP_REGIONS };

template <bool PROF, bool MIXED>
__global__ __launch_bounds__(LSD_XW * 64) void lsd_grow_xcd_kernel(LsdDev d, LsdXcd x, LsdTable<MIXED> tab) {
    __shared__ int s_ring[LSD_XW][LSD_WRING];
    __shared__ double s_term[LSD_XW][3][64];
    __shared__ int s_scan, s_done, s_qhead, s_qtail, s_cwords;
    // image b = XCD (b mod 8), place (b div 8) there; its 1 + nsb workgroups are neighbours in the XCD's share of the grid
    const int slot = blockIdx.x >> 3, role = slot % (1 + x.nsb), b = (blockIdx.x & 7) + 8 * (slot / (1 + x.nsb));
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (b >= d.B) return;
    int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    // Under a table (MIXED) two sizes meet here.  The SLOT's pixel count spx is the STRIDE of everything cut per image at creation:
    // the blocks of px / k32 / order / pend and, per wave, of stamp / wlist.  The IMAGE's own w, h, npx (its row of the table, known
    // only now that b is) are every BOUND and every pitch inside a block, where an image lies compactly as in the one-wave kernels:
    // the walks of the ranks, the dispatcher's scan, x / y of a pixel index, the neighbour bounds, the list capacities, region2rect.
    // The uniform instances do not make the call and spx is npx: their code is the code they had.
    const int spx = d.w * d.h;
    if constexpr (MIXED) lsd_take_image(d, tab, b);
    const int w = d.w, h = d.h, npx = w * h;
    const size_t base = (size_t)b * spx;
    LsdPx* px = d.px + base;
    const int32_t* __restrict__ k32 = d.k32 + base;
    const uint32_t* __restrict__ order = d.order + base;
    long long* pend = x.pend + base;
    int32_t* ctl = x.ctl + (size_t)b * LSD_CTL;
    long long* mbox = reinterpret_cast<long long*>(ctl + XC_MBOX);
    const int nw = 1 + x.nsb * LSD_XW;
    // dynamic LDS of the committer's workgroup: its flags, one bit per pixel | the feeder's record ring | the records' descriptors
    // (MIXED: carved for the IMAGE's npx — one bit per pixel it can index, fewer words to clear; the allocation is cut for the slot
    // and npx <= spx, so the records behind the bitmap end inside it, and the three waves of the workgroup carve alike)
    extern __shared__ unsigned s_bits[];
    const int nbw = (((npx + 31) / 32) + 3) & ~3;  // (whole 16-byte units: the descriptors behind are int4)
    int* const s_px = reinterpret_cast<int*>(s_bits + nbw);  // [LSD_FEED_PX] per record: its pixel indices, the record's number (mod 256) in the top byte
    int4* const s_desc = reinterpret_cast<int4*>(s_px + LSD_FEED_PX);  // [LSD_FEED_Q] {rank, size, position in s_px, words fed up to its end}
    float4* const s_dseg = reinterpret_cast<float4*>(s_desc + LSD_FEED_Q);  // [LSD_FEED_Q] the records' segments
    if (role == 0) {
        if (threadIdx.x == 0) {
            s_scan = -1;
            s_done = 0;
            s_qhead = 0;
            s_qtail = 0;
            s_cwords = 0;
        }
        for (int i = threadIdx.x; i < nbw; i += LSD_XW * 64) s_bits[i] = 0u;
        __syncthreads();
    }
    // keys and table entries of LSD_SB batches per round trip, the next such span requested before this one is worked on (the
    // committer and the feeder walk the ranks alike).
    // The end of the ranks: lsd_scan_kernel writes LSD_NOKEY into the 128 ranks behind the image's last defined pixel (those below npx:
    // the image's own under a table), and a rank >= npx reads as LSD_NOKEY here.  Behind the mark `order` may hold the keys of an earlier
    // detection — one with more defined pixels, or under a table a LARGER image of the same slot, whose pixel indices this image does
    // not have.  No reader acts on them: the committer and the feeder take batches at multiples of 64 in rank order and stop at the
    // first batch whose first rank holds LSD_NOKEY — the batch that straddles the last defined rank has the mark in all its later
    // lanes, the next one begins inside the mark; the dispatcher's chunks begin anywhere, but no further than 64 ranks behind the last
    // defined one (front <= the end of a chunk that began at a defined rank; the committer's rank is defined), so inside the 128.  The
    // requests run up to two spans ahead into stale ranks: those keys are loaded (r < npx <= the slot's pixels) and never looked at.
    constexpr int LSD_SB = 4;
    uint32_t kn[LSD_SB], kc[LSD_SB];
    long long en[LSD_SB], ec[LSD_SB];
    auto request = [&](int s0, bool entries) {
#pragma unroll
        for (int i = 0; i < LSD_SB; ++i) {
            const int r = s0 + 64 * i + lane;
            kn[i] = r < npx ? order[r] : LSD_NOKEY;
            en[i] = entries && r < npx ? ld_l2_64(pend + r) : 0ll;
        }
    };
    auto next_span = [&](int s0, bool entries) {
#pragma unroll
        for (int i = 0; i < LSD_SB; ++i) {
            kc[i] = kn[i];
            ec[i] = en[i];
        }
        request(s0 + 64 * LSD_SB, entries);
    };
    auto batch_regs = [&](int bi, uint32_t& key, long long& ent) {
        key = kc[0];
        ent = ec[0];
#pragma unroll
        for (int i = 1; i < LSD_SB; ++i) {
            key = bi == i ? kc[i] : key;
            ent = bi == i ? ec[i] : ent;
        }
    };
    if (role == 0 && wv == 0) {
        // ---------------- the committer ----------------
        // One wave on its SIMD: every instruction costs its issue latency, so the wave executes as little as possible per region.
        // Its flags are the bitmap in LDS (the global flags are written behind, for the speculating waves, and never read here); the
        // finished regions of the seeds in front of it come through LDS too — the feeder wave (below) has read table entry, segment
        // and pixel list from the L2 and left a record in rank order.  A seed without a record (its region was not finished when the
        // feeder passed, or the feeder is behind) takes the path through the table.
        __builtin_amdgcn_s_setprio(3);
        int32_t* wlist = x.wlist + (size_t)b * nw * spx;
        if (lane == 0) __hip_atomic_store(ctl + XC_ALIVE, xcc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int n_seg = 0;
        LsdProbe<PROF> pr(b == 0);  // tools/lsd_probe.py: where the committer's time goes
        LsdProbe<false> quiet(false);
        const long long t_begin = pr.now();
        int qt = 0, qh = 0;  // records consumed / known to be there
        request(0, false);
        bool at_end = false;
        for (int s0 = 0; s0 < npx && !at_end; s0 += 64 * LSD_SB) {
        next_span(s0, false);
        for (int bi = 0; bi < LSD_SB; ++bi) {
            const int o0 = s0 + 64 * bi;
            uint32_t key;
            long long ent_unused;
            batch_regs(bi, key, ent_unused);
            if ((uint32_t)__builtin_amdgcn_readfirstlane((int)key) == LSD_NOKEY) {
                at_end = true;
                break;
            }
            pr.add(CM_BATCH, 1);
            const int q_l = (int)(key & ((1u << LSD_IDX_BITS) - 1u));
            const bool key_ok = key != LSD_NOKEY;
            unsigned long long todo = __ballot(key_ok && bit_ld(s_bits, key_ok ? q_l : 0) == 0u);
            bool one_record = false;  // after a pass whose regions shared a pixel: the next pass takes the first record alone
            while (todo) {
                // ---- the records at the front of the feeder's queue against the free seeds of the batch, up to eight at once.  A lane
                // below 8 holds a descriptor, a lane of the batch that is a free seed finds "its" descriptor by its ordinal among the
                // free seeds; the pass covers the leading seeds whose records are there, one behind the other in the ring and together
                // at most 128 pixels.  All their pixels are tested in one LDS round trip and taken together as far as the sequential
                // search would take them — up to the first region with a used pixel — unless two of them share a pixel (the returning
                // ds_or of the take shows it: then the bits are cleared again and the first record goes alone).
                const long long tm0 = pr.now();
                pr.add(CM_MULTI_TRY, 1);
                if (qh - qt < 8) qh = __hip_atomic_load(&s_qhead, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int have = qh - qt < 8 ? qh - qt : 8;
                const int4 dl = s_desc[(qt + (lane & 7)) & (LSD_FEED_Q - 1)];  // {rank, pixels, position, words fed up to its end}
                const bool is_seed = (todo >> lane) & 1ull;
                const int ord = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(todo >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)todo, 0u));
                const int first_rank = o0 + __builtin_ctzll(todo);
                int k = 0;
                {
                    const int drank = __shfl(dl.x, ord & 7, 64);  // the rank in the descriptor with this seed's ordinal
                    const unsigned long long hit = __ballot(is_seed && ord < have && drank == o0 + lane);
                    const unsigned long long miss = todo & ~hit;
                    k = __builtin_popcountll(miss ? todo & ((1ull << __builtin_ctzll(miss)) - 1ull) : todo);
                    // one behind the other in the ring (a wrap shows as a jump of the running word count), 128 pixels together
                    const int base0 = __builtin_amdgcn_readfirstlane(dl.w - dl.y), pos0c = __builtin_amdgcn_readfirstlane(dl.z);
                    const int startw = dl.w - dl.y - base0;
                    const unsigned inrow = (unsigned)__ballot(lane < 8 && dl.z == pos0c + startw && startw + dl.y <= 128) & 0xFFu;
                    const int kc = __builtin_ctz(~inrow);
                    k = k < kc ? k : kc;
                    if ((one_record || !x.multi) && k > 1) k = 1;
                    one_record = false;
                }
                bool regrow_first = false;
                if (k >= 1) {
                    const int pos0 = __builtin_amdgcn_readfirstlane(dl.z);
                    const int total = __builtin_amdgcn_readlane(dl.w, k - 1) - __builtin_amdgcn_readfirstlane(dl.w - dl.y);
                    const bool a0 = lane < total, a1 = 64 + lane < total;
                    const int w0 = a0 ? s_px[pos0 + lane] : 0, w1 = a1 ? s_px[pos0 + 64 + lane] : 0;
                    const int q0 = w0 & 0xFFFFFF, q1 = w1 & 0xFFFFFF;
                    const int r0 = (((unsigned)w0 >> 24) - (unsigned)qt) & 0xFFu, r1 = (((unsigned)w1 >> 24) - (unsigned)qt) & 0xFFu;  // the record of a word, from the front
                    const unsigned long long b0 = __ballot(a0 && bit_ld(s_bits, q0) != 0u), b1 = __ballot(a1 && bit_ld(s_bits, q1) != 0u);
                    int kk = k;  // the records in front of the first one with a used pixel
                    if (b0) kk = __builtin_amdgcn_readlane(r0, __builtin_ctzll(b0));
                    else if (b1) kk = __builtin_amdgcn_readlane(r1, __builtin_ctzll(b1));
                    if (kk == 0) {  // the first record has lost a pixel: its region is grown again below
                        regrow_first = true;
                        ++qt;
                        pr.add(CM_BAD, 1);
                        if (lane == 0) {
                            lds_st(&s_cwords, __builtin_amdgcn_readfirstlane(dl.w));
                            lds_st(&s_qtail, qt);
                        }
                    } else {
                        const bool t0 = a0 && r0 < kk, t1 = a1 && r1 < kk;
                        unsigned o0w = 0u, o1w = 0u;
                        if (t0) o0w = __hip_atomic_fetch_or(s_bits + (q0 >> 5), 1u << (q0 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (t1) o1w = __hip_atomic_fetch_or(s_bits + (q1 >> 5), 1u << (q1 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const bool c0 = t0 && ((o0w >> (q0 & 31)) & 1u), c1 = t1 && ((o1w >> (q1 & 31)) & 1u);
                        if (__ballot(c0 || c1)) {  // two of the regions share a pixel: undo (the bits were clear before), the first record alone next
                            if (t0 && !c0) (void)__hip_atomic_fetch_and(s_bits + (q0 >> 5), ~(1u << (q0 & 31)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (t1 && !c1) (void)__hip_atomic_fetch_and(s_bits + (q1 >> 5), ~(1u << (q1 & 31)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            pr.add(CM_MULTI_UNDO, 1);
                            one_record = true;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            pr.add(CM_T_MULTI, pr.now() - tm0);
                            continue;
                        }
                        if (t0) st_coherent(&px[q0].used, 1);
                        if (t1) st_coherent(&px[q1].used, 1);
                        // the segments of the regions large enough, in order: a descriptor's lane each
                        const unsigned long long big = __ballot(lane < kk && dl.y >= d.min_reg_size);
                        if ((big >> lane) & 1ull) {
                            const int idx = n_seg + __builtin_popcountll(big & ((1ull << lane) - 1ull));
                            if (idx < d.seg_cap) d.seg[(size_t)b * d.seg_cap + idx] = s_dseg[(qt + lane) & (LSD_FEED_Q - 1)];
                        }
                        n_seg += __builtin_popcountll(big);
                        todo &= ~__ballot(is_seed && ord < kk);
                        const int last_rank = __builtin_amdgcn_readlane(dl.x, kk - 1), last_end = __builtin_amdgcn_readlane(dl.w, kk - 1);
                        qt += kk;
                        pr.add(CM_TOOK, kk);
                        pr.add(CM_FAST, kk);
                        pr.add(CM_MULTI, 1);
                        if (lane == 0) {
                            lds_st(&s_scan, last_rank);
                            lds_st(&s_cwords, last_end);
                            lds_st(&s_qtail, qt);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        todo &= __ballot(key_ok && bit_ld(s_bits, key_ok ? q_l : 0) == 0u);
                        pr.add(CM_T_MULTI, pr.now() - tm0);
                        continue;
                    }
                } else if (have >= 1 && __builtin_amdgcn_readfirstlane(dl.x) == first_rank) {
                    // the first seed's record is too large for a pass (more than 128 pixels: 3 % of the regions): alone, chunk by chunk
                    const int n = __builtin_amdgcn_readfirstlane(dl.y), pos = __builtin_amdgcn_readfirstlane(dl.z);
                    bool bad = false;
                    for (int t = lane; t < n; t += 64) bad = bad || bit_ld(s_bits, s_px[pos + t] & 0xFFFFFF) != 0u;
                    const bool ok = !__ballot(bad);
                    if (ok) {
                        for (int t = lane; t < n; t += 64) {
                            const int q = s_px[pos + t] & 0xFFFFFF;
                            bit_set(s_bits, q);
                            st_coherent(&px[q].used, 1);
                        }
                        if (n >= d.min_reg_size) {
                            if (lane == 0 && n_seg < d.seg_cap) d.seg[(size_t)b * d.seg_cap + n_seg] = s_dseg[qt & (LSD_FEED_Q - 1)];
                            ++n_seg;
                        }
                        todo &= todo - 1ull;
                        pr.add(CM_TOOK, 1);
                        pr.add(CM_FAST, 1);
                    } else {
                        regrow_first = true;
                        pr.add(CM_BAD, 1);
                    }
                    ++qt;
                    if (lane == 0) {
                        if (ok) lds_st(&s_scan, first_rank);
                        lds_st(&s_cwords, __builtin_amdgcn_readfirstlane(dl.w));
                        lds_st(&s_qtail, qt);
                    }
                    if (ok) {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        todo &= __ballot(key_ok && bit_ld(s_bits, key_ok ? q_l : 0) == 0u);
                        pr.add(CM_T_MULTI, pr.now() - tm0);
                        continue;
                    }
                } else {
                    // no record for the first free seed at the front of the queue: records of seeds taken meanwhile are passed over ...
                    const unsigned stale = (unsigned)__ballot(lane < have && dl.x < first_rank) & 0xFFu;
                    const int ns = __builtin_ctz(~stale);
                    if (ns > 0) {
                        const int cend = __builtin_amdgcn_readlane(dl.w, ns - 1);
                        qt += ns;
                        pr.add(CM_STALE, ns);
                        if (lane == 0) {
                            lds_st(&s_cwords, cend);
                            lds_st(&s_qtail, qt);
                        }
                        pr.add(CM_T_MULTI, pr.now() - tm0);
                        continue;
                    }
                }
                // ---- ... and ONE seed goes through the table (its region was not finished when the feeder passed, is larger than a
                // record, or the feeder is behind), or — the record's region has lost a pixel — is grown again
                const long long tp0 = pr.now();
                pr.add(CM_T_MULTI, tp0 - tm0);
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int seed = __builtin_amdgcn_readlane(q_l, j), rank = o0 + j;
                if (lane == 0) lds_st(&s_scan, rank);
                bool took = false;
                long long p = 1;
                const long long tk = pr.now();
                pr.add(CM_T_PEEK, tk - tp0);
                if (!regrow_first) {
                    auto table = [&]() { return readfirstlane64(ld_l2_64(pend + rank)); };  // (one address: a scalar result)
                    p = table();
                    if (p < 0) {  // a speculating wave is growing this very seed: its work is the work this wave would do (bounded wait)
                        const long long tw = pr.now();
                        for (int spin = 0; spin < (1 << 20) && (p = table()) < 0; ++spin) __builtin_amdgcn_s_sleep(2);
                        if (p < 0) p = 0;  // (gave up: this wave grows the seed itself, whatever the other one publishes later is never read)
                        pr.add(CM_T_WAIT, pr.now() - tw);
                        pr.add(CM_WAITED, 1);
                    }
                    if (p) {
                        const int off = (int)(p & 0x1FFFFF), n = (int)((p >> 21) & 0x1FFFFF), pw = (int)((p >> 42) & 0x7F);
                        if (n > 0) {
                            const int32_t* pl = x.wlist + ((size_t)b * nw + pw) * spx + off;  // 4 words of segment, then the pixels
                            const int w0 = lane < n + 4 ? ld_l2(pl + lane) : 0;
                            const bool has = lane >= 4 && lane < n + 4;
                            const int q0 = (w0 >> 16) * w + (w0 & 0xFFFF);
                            bool bad = has && bit_ld(s_bits, q0) != 0u;
                            for (int t = 64 + lane; t < n + 4; t += 64) {  // (a long list: the rest in further round trips)
                                const int pxy = ld_l2(pl + t);
                                bad = bad || bit_ld(s_bits, (pxy >> 16) * w + (pxy & 0xFFFF)) != 0u;
                            }
                            if (!__ballot(bad)) {  // every pixel still free: this IS the region of the sequential search
                                if (has) {
                                    bit_set(s_bits, q0);
                                    st_coherent(&px[q0].used, 1);
                                }
                                for (int t = 64 + lane; t < n + 4; t += 64) {
                                    const int pxy = ld_l2(pl + t);
                                    const int q = (pxy >> 16) * w + (pxy & 0xFFFF);
                                    bit_set(s_bits, q);
                                    st_coherent(&px[q].used, 1);
                                }
                                took = true;
                                if (n >= d.min_reg_size) {
                                    if (lane < 4 && n_seg < d.seg_cap) reinterpret_cast<int*>(d.seg + (size_t)b * d.seg_cap + n_seg)[lane] = w0;
                                    ++n_seg;
                                }
                            }
                        }
                    }
                    if (took) pr.add(CM_TOOK, 1);
                    else if (p) pr.add(CM_BAD, 1);
                    else pr.add(CM_SELF, 1);
                }
                const long long ts = pr.now();
                pr.add(CM_T_TAKE, ts - tk);
                if (!took) {
                    double reg_angle;
                    const int n = lsd_grow_fast<true, false, true, LSD_WRING, false, false>(px, nullptr, 0, s_bits, wlist, npx, s_ring[0], seed, px[seed].ang, w, h,
                                                                                            d.prec, nullptr, reg_angle, quiet);
                    if (n >= d.min_reg_size) {
                        const float4 sg = lsd_segment(lsd_region2rect<true>(wlist, n, k32, w, reg_angle, d.prec, s_term[0]), d.scale);
                        if (lane == 0 && n_seg < d.seg_cap) d.seg[(size_t)b * d.seg_cap + n_seg] = sg;
                        ++n_seg;
                    }
                    pr.add(CM_T_SELF, pr.now() - ts);
                }
                // seeds of the batch taken meanwhile (an LDS round trip)
                const long long tr0 = pr.now();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                todo &= __ballot(key_ok && bit_ld(s_bits, key_ok ? q_l : 0) == 0u);
                pr.add(CM_T_REFRESH, pr.now() - tr0);
            }
        }
        }
        if (lane == 0) {
            d.n_seg[b] = n_seg;
            lds_st(&s_done, 1);
            st_coherent(ctl + XC_DONE, 1);
        }
        if constexpr (PROF) {  // the last 16 doubles of image 0's block (row seg_cap - 1: marker -1 = a committer's counters), and row seg_cap - 5
            if (pr.on && lane == 0) {
                double* q = d.dbg + ((size_t)d.seg_cap - 2) * 8, *q5 = d.dbg + ((size_t)d.seg_cap - 5) * 8;
                q[0] = (double)(pr.now() - t_begin);
                for (int i = CM_T_SELF; i <= CM_WAITED; ++i) q[1 + i] = (double)pr.v[i];
                q[8] = -1.0;
                for (int i = CM_FAST; i <= CM_MULTI_UNDO; ++i) q[2 + i] = (double)pr.v[i];
                for (int i = CM_T_MULTI; i <= CM_MULTI_TRY; ++i) q5[i - CM_T_MULTI] = (double)pr.v[i];
            }
        }
    } else if (role == 0 && wv == 2) {
        // ---------------- the feeder: the finished regions in front of the committer, from the L2 into LDS, in rank order ----------------
        // For every seed that is free now and whose table entry shows a finished region: segment + pixel list (as pixel INDICES) into
        // the record ring, a descriptor behind it.  Never waited for by the committer; waits itself for room in the ring and keeps
        // within LSD_FEED_AHEAD ranks of the committer (entries further ahead are mostly still being grown).
        constexpr int GRP = 4;
        int wpos = 0, qhd = 0;  // words / records fed so far
        request(0, true);
        bool at_end = false;
        auto gone = [&]() { return lds_ld(&s_done) != 0; };
        for (int s0 = 0; s0 < npx && !at_end; s0 += 64 * LSD_SB) {
        next_span(s0, true);
        for (int bi = 0; bi < LSD_SB && !at_end; ++bi) {
            const int o0 = s0 + 64 * bi;
            uint32_t key;
            long long ent;
            batch_regs(bi, key, ent);
            if ((uint32_t)__builtin_amdgcn_readfirstlane((int)key) == LSD_NOKEY) {
                at_end = true;
                break;
            }
            for (int spin = 0; o0 > lds_ld(&s_scan) + x.feed_ahead; ++spin) {
                if (gone() || spin > (1 << 22)) return;
                __builtin_amdgcn_s_sleep(8);
            }
            const bool key_ok = key != LSD_NOKEY;
            const int q_l = (int)(key & ((1u << LSD_IDX_BITS) - 1u));
            // (entries read a span ago: those of free seeds that were not finished then are read again now that their batch is near)
            if (__ballot(key_ok && (ent >> 62) != 1ll && bit_ld(s_bits, key_ok ? q_l : 0) == 0u)) {
                const long long e2 = ld_l2_64(pend + (o0 + lane < npx ? o0 + lane : 0));
                ent = o0 + lane < npx ? e2 : ent;
            }
            const int en_n = (int)((ent >> 21) & 0x1FFFFF);
            unsigned long long g = __ballot(key_ok && (ent >> 62) == 1ll && en_n != 0 && en_n <= LSD_FEED_MAXW && bit_ld(s_bits, key_ok ? q_l : 0) == 0u);
            while (g) {
                int J[GRP], W[GRP];
                const int32_t* PL[GRP];
#pragma unroll
                for (int k = 0; k < GRP; ++k) {  // the loads of a group together
                    J[k] = g ? __builtin_ctzll(g) : -1;
                    g &= g - 1ull;
                    W[k] = 0;
                    PL[k] = nullptr;
                    if (J[k] >= 0) {
                        const long long p = readlane_i64(ent, J[k]);
                        const int off = (int)(p & 0x1FFFFF), n = (int)((p >> 21) & 0x1FFFFF), pw = (int)((p >> 42) & 0x7F);
                        PL[k] = x.wlist + ((size_t)b * nw + pw) * spx + off;
                        if (lane < n + 4) W[k] = ld_l2(PL[k] + lane);
                    }
                }
#pragma unroll
                for (int k = 0; k < GRP; ++k) {
                    if (J[k] < 0) continue;
                    const long long p = readlane_i64(ent, J[k]);
                    const int n = (int)((p >> 21) & 0x1FFFFF), L = n;
                    int pos = wpos & (LSD_FEED_PX - 1);
                    if (pos + L > LSD_FEED_PX) {  // (records are contiguous: the rest of the ring's end stays unused)
                        wpos += LSD_FEED_PX - pos;
                        pos = 0;
                    }
                    for (int spin = 0; wpos + L - lds_ld(&s_cwords) > LSD_FEED_PX || qhd - lds_ld(&s_qtail) >= LSD_FEED_Q; ++spin) {
                        if (gone() || spin > (1 << 22)) return;
                        __builtin_amdgcn_s_sleep(4);
                    }
                    // the list's words: the segment (4) to the descriptor's side, the pixels as INDICES tagged with the record's number
                    const int tag = (qhd & 0xFF) << 24;
                    if (lane < 4) reinterpret_cast<int*>(s_dseg + (qhd & (LSD_FEED_Q - 1)))[lane] = W[k];
                    else if (lane < n + 4) s_px[pos + lane - 4] = ((W[k] >> 16) * w + (W[k] & 0xFFFF)) | tag;
                    for (int t = 64 + lane; t < n + 4; t += 64) {
                        const int pxy = ld_l2(PL[k] + t);
                        s_px[pos + t - 4] = ((pxy >> 16) * w + (pxy & 0xFFFF)) | tag;
                    }
                    wpos += L;
                    if (lane == 0) s_desc[qhd & (LSD_FEED_Q - 1)] = make_int4(o0 + J[k], n, pos, wpos);
                    ++qhd;
                    if (lane == 0) __hip_atomic_store(&s_qhead, qhd, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);  // (the record before its count)
                }
            }
        }
        }
    } else if (role == 0 && wv == 1) {
        // ---------------- the dispatcher: hands the free seeds in front of the committer to idle speculating waves, in rank order ----------------
        // The ONLY wave that claims: no compare-and-swap, no two waves after the same seed (with every wave scanning for itself — the
        // one-workgroup form — all of them find the same first candidate: beyond ~8 waves the claims serialise).  Lane u stands for the
        // speculating waves u + 1 and u + 65: idle or not (its mail box), where its seed in flight lies.
        const int ns = nw - 1;
        int sxy0 = -1, sxy1 = -1;  // x | y << 16 of the seed in flight, -1: none
        int front = 0;             // every rank below is used, pending or claimed — for good
        LsdProbe<PROF> pr(b == 0);
        for (int idle = 0; idle < (1 << 24); ++idle) {  // (bounded)
            if (lds_ld(&s_done)) break;
            const bool idle0 = lane < ns && ld_l2_64(mbox + lane) == 1, idle1 = lane + 64 < ns && ld_l2_64(mbox + 64 + lane) == 1;  // (1: the wave is there and idle)
            if (idle0) sxy0 = -1;
            if (idle1) sxy1 = -1;
            unsigned long long I0 = __ballot(idle0), I1 = __ballot(idle1);
            pr.add(DP_ITER, 1);
            if (!(I0 | I1)) {
                pr.add(DP_NOIDLE, 1);
                __builtin_amdgcn_s_sleep(4);
                continue;
            }
            const int scan = lds_ld(&s_scan);
            const int start = front > scan + 1 ? front : scan + 1;
            if (start - scan > x.ahead) {  // far enough ahead of the committer: regions grown beyond see flags too stale to survive
                __builtin_amdgcn_s_sleep(8);
                continue;
            }
            bool contiguous = true, end = false;
            for (int c = 0; c < LSD_LOOK && (I0 | I1) && !end; c += 64) {
                const int r = start + c + lane;
                const uint32_t key = r < npx ? order[r] : LSD_NOKEY;
                end = (uint32_t)__builtin_amdgcn_readfirstlane((int)key) == LSD_NOKEY;
                if (end) break;
                const bool ok = key != LSD_NOKEY;
                const int q = (int)(key & ((1u << LSD_IDX_BITS) - 1u));
                const bool open = ok && bit_ld(s_bits, ok ? q : 0) == 0u && ld_coherent64(pend + (ok ? r : 0)) == 0;  // (the committer's bitmap; this wave's own claims: one CU)
                const int qx = q % w, qy = q / w;
                const unsigned long long m_open = __ballot(open);
                unsigned long long mm = m_open, given = 0ull;
                pr.add(DP_CHUNKS, 1);
                while (mm && (I0 | I1)) {
                    const int L = __builtin_ctzll(mm);
                    mm &= mm - 1ull;
                    const int cx = __builtin_amdgcn_readlane(qx, L), cy = __builtin_amdgcn_readlane(qy, L);
                    auto near = [&](int sxy) {
                        const int ddx = cx - (sxy & 0xFFFF), ddy = cy - (sxy >> 16);
                        const int adx = ddx < 0 ? -ddx : ddx, ady = ddy < 0 ? -ddy : ddy;
                        return sxy >= 0 && (adx > ady ? adx : ady) < x.sep;
                    };
                    if (__ballot(near(sxy0) || near(sxy1))) {  // too close to a growth in flight: later (the front stays in front of it)
                        pr.add(DP_BLOCKED, 1);
                        continue;
                    }
                    const int u = I0 ? __builtin_ctzll(I0) : 64 + __builtin_ctzll(I1);
                    if (u < 64) I0 &= I0 - 1ull;
                    else I1 &= I1 - 1ull;
                    if (lane == (u & 63)) {
                        if (u < 64) sxy0 = cx | (cy << 16);
                        else sxy1 = cx | (cy << 16);
                    }
                    if (lane == L) {
                        st_coherent64(pend + r, LSD_CLAIM | (long long)(u + 1));
                        st_coherent64(mbox + u, (1ll << 62) | ((long long)r << 21) | (long long)q);
                    }
                    given |= 1ull << L;
                    pr.add(DP_GIVEN, 1);
                    idle = 0;
                }
                if (contiguous) {  // the ranks of this chunk in front of the first one still open join the solid part
                    const unsigned long long rem = m_open & ~given;
                    front = start + c + (rem ? __builtin_ctzll(rem) : 64);
                    contiguous = rem == 0ull;
                }
            }
        }
        if constexpr (PROF) {
            if (pr.on && lane == 0)
                for (int i = 0; i < DP_N; ++i) d.dbg[((size_t)d.seg_cap - 4) * 8 + i] = (double)pr.v[i];
        }
    } else if (role != 0) {
        // ---------------- a speculating wave ----------------
        {  // on the committer's XCD, or not at all
            int alive = 0;
            for (int spin = 0; spin < (1 << 18) && (alive = __builtin_amdgcn_readfirstlane(ld_l2(ctl + XC_ALIVE))) == 0; ++spin) __builtin_amdgcn_s_sleep(16);
            if (alive != xcc + 1) return;
        }
        const int v = 1 + (role - 1) * LSD_XW + wv;  // this wave among the image's waves
        int32_t* stamp = x.stamp + ((size_t)b * nw + v) * spx;
        int32_t* wl = x.wlist + ((size_t)b * nw + v) * spx;
        int id = 0, off = 0;
        LsdProbe<PROF> pr(b == 0);
        LsdProbe<false> quiet(false);
        const long long sp_t0 = pr.now();
        if (lane == 0) st_coherent64(mbox + (v - 1), 1ll);  // here, and idle
        for (int idle = 0; idle < (1 << 24); ++idle) {  // (bounded: a wave that is handed nothing for this long gives up)
            const long long m = readfirstlane64(ld_l2_64(mbox + (v - 1)));
            if (m <= 1) {
                if (__builtin_amdgcn_readfirstlane(ld_l2(ctl + XC_DONE))) break;
                __builtin_amdgcn_s_sleep(2);
                continue;
            }
            idle = 0;
            const long long sp_a = pr.now();
            const int pick_r = (int)((m >> 21) & 0x1FFFFF), pick_q = (int)(m & 0x1FFFFF);
            int n = 0;
            if (npx - off >= 4096) {  // (out of room: empty records from here on — the committer grows those seeds itself)
                ++id;
                double reg_angle = 0.0;
                n = lsd_grow_fast<false, true, false, LSD_WRING, false, false>(px, stamp, id, nullptr, wl + off + 4, npx - off - 4, s_ring[wv], pick_q, px[pick_q].ang, w, h,
                                                                        d.prec, nullptr, reg_angle, quiet);
                if (n >= d.min_reg_size) {
                    const float4 sg = lsd_segment(lsd_region2rect<true>(wl + off + 4, n, k32, w, reg_angle, d.prec, s_term[wv]), d.scale);
                    if (lane == 0) {
                        st_coherent(wl + off, __float_as_int(sg.x));
                        st_coherent(wl + off + 1, __float_as_int(sg.y));
                        st_coherent(wl + off + 2, __float_as_int(sg.z));
                        st_coherent(wl + off + 3, __float_as_int(sg.w));
                    }
                }
            }
            // the list and the segment have reached the L2 before the table entry leaves (a workgroup-scope release does not wait: the
            // entry is read on ANOTHER CU)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) st_coherent64(pend + pick_r, lsd_entry_x(v, n > 0 ? n : 0, off));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) st_coherent64(mbox + (v - 1), 1ll);  // idle again
            if (n > 0) off += 4 + n;
            pr.add(SP_BUSY, pr.now() - sp_a);
            pr.add(SP_REGIONS, 1);
        }
        if constexpr (PROF) {  // tools/lsd_probe.py: the speculating waves together (row seg_cap - 3 of image 0's block, as integers)
            if (pr.on && lane == 0) {
                unsigned long long* q = reinterpret_cast<unsigned long long*>(d.dbg + ((size_t)d.seg_cap - 3) * 8);
                atomicAdd(q + 0, (unsigned long long)pr.v[SP_BUSY]);
                atomicAdd(q + 1, (unsigned long long)(pr.now() - sp_t0));
                atomicAdd(q + 2, (unsigned long long)pr.v[SP_REGIONS]);
                atomicAdd(q + 3, 1ull);
            }
        }
    }
}

// LSDDetectorC::detectImpl's loop over the segments of the (single) octave (:254-303) and the cut of stereoFrame.cpp:231-240
constexpr int KL_T = 256;
template <bool MIXED>
__global__ __launch_bounds__(KL_T) void lsd_keylines_kernel(LsdDev d, LsdTable<MIXED> tab) {
    extern __shared__ float s_resp[];  // [seg_cap] responses of the kept lines, detection order
    __shared__ int s_wave[KL_T / 64];
    __shared__ int s_run;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if constexpr (MIXED) lsd_take_image(d, tab, b);  // (the clamps, the response divisor, the raster and the minimum length are the image's own)
    const int n = min(d.n_seg[b], d.seg_cap);
    const float4* seg = d.seg + (size_t)b * d.seg_cap;
    int* s_src = reinterpret_cast<int*>(s_resp + d.seg_cap);  // [seg_cap] segment of kept line k
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += KL_T) {  // the lines that pass min_length, in detection order
        const int k = c0 + tid;
        bool keep = false;
        float len = 0.f;
        if (k < n) {
            float4 e = seg[k];
            if (e.x < 0) e.x = 0;  // checkLineExtremes
            if (e.x >= d.cols) e.x = (float)d.cols - 1.0f;
            if (e.z < 0) e.z = 0;
            if (e.z >= d.cols) e.z = (float)d.cols - 1.0f;
            if (e.y < 0) e.y = 0;
            if (e.y >= d.rows) e.y = (float)d.rows - 1.0f;
            if (e.w < 0) e.w = 0;
            if (e.w >= d.rows) e.w = (float)d.rows - 1.0f;
            const double d0 = (double)(e.x - e.z), d1 = (double)(e.y - e.w);
            const double length = (double)(float)sqrt(d0 * d0 + d1 * d1);
            keep = length > d.min_length;
            len = (float)length;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int pos = s_run + __popcll(bal & ((1ull << lane) - 1ull));
        for (int v = 0; v < wv; ++v) pos += s_wave[v];
        if (keep) {
            s_resp[pos] = __fdiv_rn(len, (float)(d.cols > d.rows ? d.cols : d.rows));
            s_src[pos] = k;
        }
        __syncthreads();
        if (tid == 0) {
            int q = 0;
            for (int v = 0; v < KL_T / 64; ++v) q += s_wave[v];
            s_run += q;
        }
        __syncthreads();
    }
    const int m = s_run;
    // the top-N cut of stereoFrame.cpp:231-240 — and when the CAPACITY binds (lsd_nfeatures = 0 or above max_keylines) the same
    // selection for K lines: the K strongest, not the first K in detection order (the uncut count goes to n_pass: stvo_lsd_counts)
    const int n_out = min(d.nfeatures != 0 ? min(d.nfeatures, m) : m, d.K);
    const bool cut = m > n_out;
    for (int i = tid; i < m; i += KL_T) {
        int rank = i;
        if (cut) {  // position in the stable descending order of the responses
            const float r = s_resp[i];
            rank = 0;
            for (int j = 0; j < m; ++j) {
                const float q = s_resp[j];
                rank += (q > r || (q == r && j < i)) ? 1 : 0;
            }
        }
        if (rank >= n_out) continue;
        float4 e = seg[s_src[i]];
        if (e.x < 0) e.x = 0;
        if (e.x >= d.cols) e.x = (float)d.cols - 1.0f;
        if (e.z < 0) e.z = 0;
        if (e.z >= d.cols) e.z = (float)d.cols - 1.0f;
        if (e.y < 0) e.y = 0;
        if (e.y >= d.rows) e.y = (float)d.rows - 1.0f;
        if (e.w < 0) e.w = 0;
        if (e.w >= d.rows) e.w = (float)d.rows - 1.0f;
        stvo_keyline kl;
        kl.sx = e.x; kl.sy = e.y; kl.ex = e.z; kl.ey = e.w;
        kl.angle = (float)atan2((double)(e.w - e.y), (double)(e.z - e.x));
        // cv::LineIterator count: end points rounded to pixels, the line CLIPPED to the image (checkLineExtremes leaves coordinates in
        // [cols - 0.5, cols) / [rows - 0.5, rows) as they are, and those round to the first position outside), 8-connected raster
        kl.num_pixels = line_iterator_count(d.cols, d.rows, e.x, e.y, e.z, e.w);
        d.lines[(size_t)b * d.K + rank] = kl;
        if (d.response) d.response[(size_t)b * d.K + rank] = s_resp[i];
    }
    if (tid == 0) {
        d.n_lines[b] = n_out;
        d.n_pass[b] = m;
    }
}

// the end points of key-line records as the rows stvo_frame_features::kl_l / kl_r take (unused rows zeroed)
__global__ __launch_bounds__(256) void keylines_xy_kernel(int stride, const stvo_keyline* lines, const int32_t* n_lines, float4* xy) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= stride) return;
    const stvo_keyline q = lines[(size_t)b * stride + i];
    xy[(size_t)b * stride + i] = i < n_lines[b] ? make_float4(q.sx, q.sy, q.ex, q.ey) : make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace
}  // namespace stvo

struct stvo_lsd {
    stvo_ctx* ctx = nullptr;
    stvo::LsdDev d{};
    stvo_lsd_params prm{};
    int radius = 0;                     // of the blur (stvo_lsd_geometry)
    int kw[STVO_LSD_MAX_TAPS] = {0};    // its 1 + 2 radius integer weights
    stvo::BlurResizePlan plan{};        // radius != 3: the tile of lsd_blur_resize_kernel
    char* dev = nullptr;
    uint8_t *img = nullptr, *blur = nullptr, *scaled = nullptr;
    stvo_keyline* lines = nullptr;  // device buffers of the host-pointer entry points
    float* response = nullptr;
    int32_t* n_lines = nullptr;
    double* dbg = nullptr;
    char* wdev = nullptr;
    size_t stamp_bytes = 0, pend_ctl_bytes = 0;  // what a call clears of the scratch below (frontend_layout.h: LsdXcdArena)
    stvo::LsdXcd xx{};        // scratch of lsd_grow_xcd_kernel (small batches, the default), or null
    int xcd_lds = 0;          // its dynamic LDS: the committer's bitmap — and at least 84 KB, so that a CU holds ONE of its workgroups (a wave per SIMD)
    // one image size per image (stvo_lsd_set_image_sizes): nothing of it exists until the first call.  The device table holds the n rows
    // the detector's own kernels read (LsdSizeRow), then the 2 n rows that drive the shared blur and resize (lsd_sizes.h: lsd_scale_rows)
    TableTransport sizes;
    int n_sizes = 0;          // entries of the table in force; 0: every image fills its slot
    int table_route = STVO_LSD_TABLE_ONE_WAVE;  // stvo_lsd_set_table_route: what a table does to the search's route (lsd_route.h)
    const stvo::OrbLevelSize* scale_rows() const { return reinterpret_cast<const stvo::OrbLevelSize*>(sizes.dev + (size_t)n_sizes * sizeof(stvo::LsdSizeRow)); }
};

namespace {

// the scaled image of a detector with scale != 1: radius 3 on the two kernels it always had, every other radius on the fused one
void lsd_scaled_enqueue(stvo_lsd* o, const uint8_t* images) {
    const stvo::LsdDev& d = o->d;
    hipStream_t s = o->ctx->stream;
    if (o->radius == 3) {
        // under a size table: the MIXED instances on the slots' grids, each image blurred to its own border and resized from its own size
        const stvo::OrbLevelSize* sz = o->n_sizes ? o->scale_rows() : nullptr;
        stvo::launch_blur7_u8(s, d.B, d.cols, d.rows, images, o->blur, o->kw, sz, o->n_sizes, 2, 0);
        stvo::launch_resize_linear_u8(s, d.B, d.cols, d.rows, d.w, d.h, o->blur, o->scaled, d.scale, d.scale, sz, o->n_sizes, 2, 1);
    } else {
        // under a size table (a detector created with STVO_LSD_SIZES_ANY_RADIUS): the MIXED instance under the slot's plan, which bounds
        // every image that fits the slot (lsd_scale_plan.h)
        const stvo::LsdSizeRow* sz = o->n_sizes ? reinterpret_cast<const stvo::LsdSizeRow*>(o->sizes.dev) : nullptr;
        stvo::launch_blur_resize_u8(s, d.B, d.cols, d.rows, d.w, d.h, images, o->scaled, d.scale, o->radius, o->kw, o->plan, sz, o->n_sizes);
    }
}

static_assert(STVO_LSD_SEARCH_ONE_WAVE == stvo::LSD_SEARCH_ONE_WAVE && STVO_LSD_SEARCH_ONE_WAVE_PLAIN == stvo::LSD_SEARCH_ONE_WAVE_PLAIN &&
                  STVO_LSD_SEARCH_MANY_WAVES == stvo::LSD_SEARCH_MANY_WAVES && STVO_LSD_TABLE_ONE_WAVE == stvo::LSD_TABLE_ONE_WAVE &&
                  STVO_LSD_TABLE_BY_BATCH == stvo::LSD_TABLE_BY_BATCH,
              "lsd_route.h restates the values of stvo_hip.h");

// the facts lsd_route.h decides on, as they stand for the next detection
stvo::LsdRouteFacts lsd_route_facts(const stvo_lsd* o) {
    return stvo::LsdRouteFacts{o->prm.refine, o->wdev != nullptr, o->n_sizes != 0, o->table_route, stvo::dbg().lsd_grow, o->d.dbg != nullptr};
}

int lsd_enqueue(stvo_lsd* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    stvo_ctx* ctx = o->ctx;
    hipStream_t s = ctx->stream;
    stvo::LsdDev d = o->d;
    const uint8_t* src = images;
    if (d.scale != 1) {
        lsd_scaled_enqueue(o, images);
        src = o->scaled;
    }
    d.scaled = src;
    d.lines = lines; d.response = response; d.n_lines = n_lines;
    HIP_TRY(ctx, hipMemsetAsync(d.kmax, 0xFF, (size_t)d.B * 4, s));
    const dim3 grid((d.w + 255) / 256, (d.h + stvo::LSD_ROWS - 1) / stvo::LSD_ROWS, d.B);
    const int nunits = (d.w * d.h + stvo::LSD_UNIT - 1) / stvo::LSD_UNIT;
    const dim3 ug((nunits + 3) / 4, d.B);
    const size_t lds_h = (size_t)4 * d.n_bins * 4, lds = (size_t)d.seg_cap * 8;
    const stvo::LsdRoute route = stvo::lsd_search_route(lsd_route_facts(o));  // the search kernel: decided in lsd_route.h, launched below
    const dim3 xg(8 * ((d.B + 7) / 8) * (1 + o->xx.nsb)), xb(stvo::LSD_XW * 64);
    if (o->n_sizes) {
        // One size per image: the MIXED instances of every kernel on the slots' launch grids.  No PROF instance exists under a table.
        const stvo::LsdTable<true> tab{reinterpret_cast<const stvo::LsdSizeRow*>(o->sizes.dev), o->n_sizes};
        hipLaunchKernelGGL(stvo::lsd_gradient_kernel<true>, grid, dim3(256), 0, s, d, tab);
        hipLaunchKernelGGL(stvo::lsd_hist_kernel<true>, ug, dim3(256), lds_h, s, d, tab);
        hipLaunchKernelGGL(stvo::lsd_scan_kernel<true>, dim3(d.B), dim3(1024), 0, s, d, tab);
        hipLaunchKernelGGL(stvo::lsd_scatter_kernel<true>, ug, dim3(256), lds_h, s, d, tab);
        if (route.search == STVO_LSD_SEARCH_MANY_WAVES) {  // STVO_LSD_TABLE_BY_BATCH: its scratch is cut for the slots and cleared whole
            HIP_TRY(ctx, hipMemsetAsync(o->xx.stamp, 0, o->stamp_bytes, s));
            HIP_TRY(ctx, hipMemsetAsync(o->xx.pend, 0, o->pend_ctl_bytes, s));
            hipLaunchKernelGGL((stvo::lsd_grow_xcd_kernel<false, true>), xg, xb, o->xcd_lds, s, d, o->xx, tab);
        } else if (route.search == STVO_LSD_SEARCH_ONE_WAVE_PLAIN && route.refine) hipLaunchKernelGGL((stvo::lsd_grow_refine_kernel<true, false, true>), dim3(d.B), dim3(64), 0, s, d, o->prm.density_th, tab);
        else if (route.search == STVO_LSD_SEARCH_ONE_WAVE_PLAIN) hipLaunchKernelGGL((stvo::lsd_grow_refine_kernel<false, false, true>), dim3(d.B), dim3(64), 0, s, d, 0.0, tab);
        else hipLaunchKernelGGL((stvo::lsd_grow_kernel<false, true>), dim3(d.B), dim3(64), 0, s, d, tab);
        hipLaunchKernelGGL(stvo::lsd_keylines_kernel<true>, dim3(d.B), dim3(stvo::KL_T), lds, s, d, tab);
        return check_launch(ctx);
    }
    const stvo::LsdTable<false> none{};  // the uniform instances: the kernels and arguments of a detector that was never given a table
    hipLaunchKernelGGL(stvo::lsd_gradient_kernel<false>, grid, dim3(256), 0, s, d, none);
    // the pseudo-ordering: counting sort by bin (histogram per unit, scan per image, stable scatter)
    hipLaunchKernelGGL(stvo::lsd_hist_kernel<false>, ug, dim3(256), lds_h, s, d, none);
    hipLaunchKernelGGL(stvo::lsd_scan_kernel<false>, dim3(d.B), dim3(1024), 0, s, d, none);
    hipLaunchKernelGGL(stvo::lsd_scatter_kernel<false>, ug, dim3(256), lds_h, s, d, none);
    const bool prof = route.prof;  // stvo_lsd_debug has the probes on: the PROF instance of the route's kernel
    if (route.search == STVO_LSD_SEARCH_ONE_WAVE_PLAIN && route.refine) {  // LSD_REFINE_STD: regions may give their pixels back — the plain one-wave kernel with refinement, for every batch size
        hipLaunchKernelGGL((stvo::lsd_grow_refine_kernel<true, false, false>), dim3(d.B), dim3(64), 0, s, d, o->prm.density_th, none);
    } else if (route.search == STVO_LSD_SEARCH_MANY_WAVES) {  // small batches: a committing wave + speculating workgroups on the CUs of one XCD per image (lsd_grow_xcd_kernel)
        HIP_TRY(ctx, hipMemsetAsync(o->xx.stamp, 0, o->stamp_bytes, s));
        HIP_TRY(ctx, hipMemsetAsync(o->xx.pend, 0, o->pend_ctl_bytes, s));  // (the control words lie behind the table)
        if (prof) hipLaunchKernelGGL((stvo::lsd_grow_xcd_kernel<true, false>), xg, xb, o->xcd_lds, s, d, o->xx, none);
        else hipLaunchKernelGGL((stvo::lsd_grow_xcd_kernel<false, false>), xg, xb, o->xcd_lds, s, d, o->xx, none);
    } else if (route.search == STVO_LSD_SEARCH_ONE_WAVE_PLAIN) {  // STVO_LSD_GROW=0: the plain one-wave kernel, nothing refined
        if (prof) hipLaunchKernelGGL((stvo::lsd_grow_refine_kernel<false, true, false>), dim3(d.B), dim3(64), 0, s, d, 0.0, none);
        else hipLaunchKernelGGL((stvo::lsd_grow_refine_kernel<false, false, false>), dim3(d.B), dim3(64), 0, s, d, 0.0, none);
    } else {
        if (prof) hipLaunchKernelGGL((stvo::lsd_grow_kernel<true, false>), dim3(d.B), dim3(64), 0, s, d, none);
        else hipLaunchKernelGGL((stvo::lsd_grow_kernel<false, false>), dim3(d.B), dim3(64), 0, s, d, none);
    }
    hipLaunchKernelGGL(stvo::lsd_keylines_kernel<false>, dim3(d.B), dim3(stvo::KL_T), lds, s, d, none);
    return check_launch(ctx);
}

}  // namespace

extern "C" {

int stvo_lsd_geometry(const stvo_lsd_params* prm, int cols, int rows, int32_t* scaled_cols, int32_t* scaled_rows, double* sigma_out,
                      int32_t* radius, int32_t* weights) {
    if (!prm || cols < 8 || rows < 8) return STVO_ERR_INVALID_ARG;
    if (prm->refine != 0 && prm->refine != 1) return STVO_ERR_UNSUPPORTED;  // LSD_REFINE_ADV (rect_improve + the NFA test) is not built; no shipped configuration uses it
    if (prm->refine == 1 && !(prm->density_th >= 0)) return STVO_ERR_INVALID_ARG;
    if (!(prm->scale > 0) || !(prm->ang_th > 0 && prm->ang_th < 180) || prm->n_bins < 1 || prm->n_bins > 4096 || prm->nfeatures < 0)
        return STVO_ERR_INVALID_ARG;
    // sort key = (n_bins - 1 - bin) << LSD_IDX_BITS | index, LSD_NOKEY = all ones: with 4096 bins the keys of bin 0 would share their
    // top 12 bits with the undefined pixels' key and the bin-bits-only sort would interleave them
    if (prm->n_bins > stvo::LSD_MAX_BINS) return STVO_ERR_UNSUPPORTED;
    int w = cols, h = rows, hk = 0;
    double sigma = 0.0;
    int32_t kw[STVO_LSD_MAX_TAPS] = {0};
    if (prm->scale != 1) {
        if (!(prm->sigma_scale >= 0)) return STVO_ERR_INVALID_ARG;  // (a negative or NaN sigma has no kernel size)
        sigma = prm->scale < 1 ? prm->sigma_scale / prm->scale : prm->sigma_scale;
        const double hd = std::ceil(sigma * std::sqrt(2 * 3.0 * std::log(10.0)));
        // radii 0 .. 15 are built: radius 3 (sigma between 0.54 and 0.80: scale 1.2 / sigma_scale 0.6 and OpenCV's own 0.8 / 0.6) on the
        // 7 x 7 kernel of the ORB front-end, the others on lsd_blur_resize_kernel
        if (!(hd <= STVO_LSD_MAX_RADIUS)) return STVO_ERR_UNSUPPORTED;
        hk = (int)hd;
        const double wd = stvo::lsd_scaled_extent(cols, prm->scale), hd2 = stvo::lsd_scaled_extent(rows, prm->scale);  // resize(..., Size(), scale, scale): cvRound
        if (!(wd >= 1 && hd2 >= 1)) return STVO_ERR_INVALID_ARG;  // nothing is left of the image
        if (wd >= 65536 || hd2 >= 32768) return STVO_ERR_CAPACITY;
        w = (int)wd;
        h = (int)hd2;
    }
    if ((long long)w * h > (1ll << stvo::LSD_IDX_BITS) || w >= 65536 || h >= 32768) return STVO_ERR_CAPACITY;
    stvo::gaussian_q8(hk, sigma, kw);  // orc_lsd_kernel7 with 7 -> 1 + 2 hk (radius 0, where sigma may be 0: the identity)
    if (scaled_cols) *scaled_cols = w;
    if (scaled_rows) *scaled_rows = h;
    if (sigma_out) *sigma_out = sigma;
    if (radius) *radius = hk;
    if (weights)
        for (int i = 0; i < STVO_LSD_MAX_TAPS; ++i) weights[i] = kw[i];
    return STVO_OK;
}

int stvo_lsd_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keylines, const stvo_lsd_params* prm, stvo_lsd** out) {
    if (!ctx || !out || B < 1 || max_keylines < 1) return STVO_ERR_INVALID_ARG;
    int32_t gw = 0, gh = 0, radius = 0, kw[STVO_LSD_MAX_TAPS];
    TRY(stvo_lsd_geometry(prm, cols, rows, &gw, &gh, nullptr, &radius, kw));
    stvo::BlurResizePlan plan{};
    // (a tile of the fused kernel holds the source window of one output pixel at least: scales far below 0.01 do not fit the LDS)
    if (prm->scale != 1 && radius != 3 && !stvo::plan_blur_resize_u8(cols, rows, prm->scale, radius, &plan)) return STVO_ERR_UNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_lsd* o = new (std::nothrow) stvo_lsd();
    if (!o) return STVO_ERR_HIP;
    o->ctx = ctx;
    o->prm = *prm;
    stvo::LsdDev& d = o->d;
    d.B = B; d.cols = cols; d.rows = rows; d.w = cols; d.h = rows;
    d.scale = prm->scale;
    d.w = gw; d.h = gh;  // stvo_lsd_geometry: the scaled size, the blur's radius and weights
    o->radius = radius;
    for (int i = 0; i < STVO_LSD_MAX_TAPS; ++i) o->kw[i] = kw[i];
    o->plan = plan;
    d.n_bins = prm->n_bins;
    d.rho = prm->quant / std::sin(stvo::LSD_PI * prm->ang_th / 180);
    d.prec = stvo::LSD_PI * prm->ang_th / 180;
    d.min_reg_size = stvo::lsd_min_reg_size(d.w, d.h, prm->ang_th);
    d.min_length = prm->min_length;
    d.nfeatures = prm->nfeatures;
    d.K = max_keylines;
    d.seg_cap = 8192;  // segments per image the wrapper ranks (its LDS: 8 bytes each); more are counted, not stored
    const size_t npx = (size_t)d.w * d.h;
    stvo::Carver size;
    stvo::carve_lsd_arena(size, B, cols, rows, d.w, d.h, d.n_bins, d.seg_cap, d.K, radius == 3);
    bool ok = hip_ok(ctx, hipMalloc((void**)&o->dev, size.off), "hipMalloc lsd") && zero_device(ctx, o->dev, size.off, "hipMemset lsd");
    if (ok) {
        stvo::Carver c(o->dev);
        const stvo::LsdArena a = stvo::carve_lsd_arena(c, B, cols, rows, d.w, d.h, d.n_bins, d.seg_cap, d.K, radius == 3);
        o->blur = a.blur; o->scaled = a.scaled; o->img = a.img;
        d.px = a.px; d.k32 = a.k32; d.cnt = a.cnt; d.order = a.order; d.reg = a.reg; d.kmax = a.kmax;
        d.seg = a.seg; d.n_seg = a.n_seg; d.n_pass = a.n_pass;
        o->lines = a.lines; o->response = a.response; o->n_lines = a.n_lines;
    }
    if (ok && (size_t)4 * d.n_bins * 4 > 48 * 1024) {
        ok = stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_hist_kernel<false>), 4 * d.n_bins * 4) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_scatter_kernel<false>), 4 * d.n_bins * 4) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_hist_kernel<true>), 4 * d.n_bins * 4) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_scatter_kernel<true>), 4 * d.n_bins * 4);
    }
    if (ok && (size_t)d.seg_cap * 8 > 48 * 1024)
        ok = stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_keylines_kernel<false>), d.seg_cap * 8) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_keylines_kernel<true>), d.seg_cap * 8);
    if (ok && stvo::dbg().lsd_waves != 0 && stvo::lsd_xcd_route(prm->refine, B, npx)) {  // small batches (STVO_LSD_WAVES=0: one wave per image there too)
        // an XCD has 32 CUs and a CU holds one of the kernel's workgroups: images per XCD x (1 + speculating workgroups) <= 32
        const int per_xcd = (B + 7) / 8;
        int nsb = stvo::dbg().lsd_xcd_blocks == stvo::DBG_UNSET ? (32 / per_xcd - 1 < 16 ? 32 / per_xcd - 1 : 16) : stvo::dbg().lsd_xcd_blocks;  // STVO_LSD_XCD_BLOCKS
        nsb = nsb < 0 ? 0 : (nsb > (stvo::LSD_X_MAXW - 1) / stvo::LSD_XW ? (stvo::LSD_X_MAXW - 1) / stvo::LSD_XW : nsb);
        const size_t nw = 1 + (size_t)nsb * stvo::LSD_XW;
        stvo::Carver wsize;
        stvo::carve_lsd_xcd_arena(wsize, B, npx, nw);
        o->xcd_lds = (int)(((((npx + 31) / 32) + 3) & ~size_t(3)) * 4) + stvo::LSD_FEED_PX * 4 + stvo::LSD_FEED_Q * 32;
        if (o->xcd_lds < 84 * 1024) o->xcd_lds = 84 * 1024;
        ok = stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_grow_xcd_kernel<false, false>), o->xcd_lds) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_grow_xcd_kernel<true, false>), o->xcd_lds) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::lsd_grow_xcd_kernel<false, true>), o->xcd_lds) &&  // (the opt-in is per function)
             hip_ok(ctx, hipMalloc((void**)&o->wdev, wsize.off), "hipMalloc lsd xcd");
        if (ok) {
            stvo::Carver cw(o->wdev);
            const stvo::LsdXcdArena a = stvo::carve_lsd_xcd_arena(cw, B, npx, nw);
            o->xx.stamp = a.stamp; o->xx.wlist = a.wlist; o->xx.pend = a.pend; o->xx.ctl = a.ctl;
            o->stamp_bytes = a.stamp_bytes;
            o->pend_ctl_bytes = a.pend_ctl_bytes;
            o->xx.nsb = nsb;
            const auto& g = stvo::dbg();
            o->xx.feed_ahead = g.lsd_feed_ahead == stvo::DBG_UNSET ? stvo::LSD_FEED_AHEAD : g.lsd_feed_ahead;
            o->xx.sep = g.lsd_sep == stvo::DBG_UNSET ? stvo::LSD_SEP : g.lsd_sep;
            o->xx.ahead = g.lsd_ahead == stvo::DBG_UNSET ? stvo::LSD_AHEAD : g.lsd_ahead;
            o->xx.multi = g.lsd_multi == 0 ? 0 : 1;
        }
    }
    if (!ok) {
        stvo_lsd_destroy(o);
        return STVO_ERR_HIP;
    }
    *out = o;
    return STVO_OK;
}

int stvo_lsd_destroy(stvo_lsd* o) {
    if (!o) return STVO_OK;
    if (o->ctx) {
        (void)hipSetDevice(o->ctx->device);
        (void)hipStreamSynchronize(o->ctx->stream);
    }
    if (o->dbg) (void)hipFree(o->dbg);
    if (o->wdev) (void)hipFree(o->wdev);
    if (o->dev) (void)hipFree(o->dev);
    o->sizes.destroy();
    delete o;
    return STVO_OK;
}

// One image size (and minimum length) per image (stvo_hip.h).  Validated before anything changes; the table is formed with the functions
// stvo_lsd_geometry / stvo_lsd_create form the slot's own values with (lsd_sizes.h) and travels as table_transport.h says.
int stvo_lsd_set_image_sizes(stvo_lsd* o, const int32_t* sizes_host, const double* min_length_host, int n) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (!sizes_host) {  // every image fills its slot again: the uniform kernel instances, which read no table
        o->n_sizes = 0;
        return STVO_OK;
    }
    const stvo::LsdDev& d = o->d;
    if (!stvo::lsd_image_sizes_ok(sizes_host, min_length_host, n, d.B, d.cols, d.rows, d.scale)) return STVO_ERR_INVALID_ARG;
    // the fused blur + resize of the other radii runs every image under the slot's tile plan (lsd_scale_plan.h: the bound) — for a
    // detector that asked for it at creation; without the flag such a detector keeps one size, as it always did
    if (d.scale != 1 && o->radius != 3 && !(o->prm.flags & STVO_LSD_SIZES_ANY_RADIUS)) return STVO_ERR_UNSUPPORTED;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    constexpr size_t entry = sizeof(stvo::LsdSizeRow) + 2 * sizeof(stvo::OrbLevelSize);
    char* tab = o->sizes.begin(ctx, (size_t)d.B * entry);
    if (!tab) return STVO_ERR_HIP;
    stvo::LsdSizeRow* rows = reinterpret_cast<stvo::LsdSizeRow*>(tab);
    stvo::OrbLevelSize* srows = reinterpret_cast<stvo::OrbLevelSize*>(tab + (size_t)n * sizeof(stvo::LsdSizeRow));
    for (int i = 0; i < n; ++i) {
        rows[i] = stvo::lsd_size_row(sizes_host[2 * i], sizes_host[2 * i + 1], d.scale, o->prm.ang_th,
                                     stvo::lsd_entry_min_length(min_length_host, i, d.min_length));
        stvo::lsd_scale_rows(rows[i], d.scale, srows + 2 * i);
    }
    TRY(o->sizes.send(ctx, (size_t)n * entry));
    o->n_sizes = n;
    return STVO_OK;
}

// What a size table does to the route of the search (stvo_hip.h).  Host only: a field the next lsd_enqueue reads.
int stvo_lsd_set_table_route(stvo_lsd* o, int route) {
    if (!o || !stvo::lsd_table_route_ok(route)) return STVO_ERR_INVALID_ARG;
    o->table_route = route;
    return STVO_OK;
}

int stvo_lsd_search_route(stvo_lsd* o, int32_t* route) {
    if (!o || !route) return STVO_ERR_INVALID_ARG;
    *route = stvo::lsd_search_route(lsd_route_facts(o)).search;
    return STVO_OK;
}

int stvo_lsd_detect_dev(stvo_lsd* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    if (!o || !images || !lines || !n_lines) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lsd_enqueue(o, images, lines, response, n_lines);
}

int stvo_lsd_detect(stvo_lsd* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    if (!o || !images || !lines || !n_lines) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::LsdDev& d = o->d;
    const size_t img_bytes = (size_t)d.B * d.cols * d.rows;
    HIP_TRY(ctx, hipMemcpyAsync(o->img, images, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(lsd_enqueue(o, o->img, o->lines, o->response, o->n_lines));
    HIP_TRY(ctx, hipMemcpyAsync(lines, o->lines, (size_t)d.B * d.K * sizeof(stvo_keyline), hipMemcpyDeviceToHost, ctx->stream));
    if (response) HIP_TRY(ctx, hipMemcpyAsync(response, o->response, (size_t)d.B * d.K * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_lines, o->n_lines, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

// developer aid, not part of include/: switches the detector to the PROF instances of its search kernel (enable) or back, and hands out
// what the last detection under them left for its first image — the rectangle intermediates per segment (the one-wave kernels) and the
// counter rows at the end of the block (tools/lsd_probe.py).  lsd_refine = 1 has no such instance.
extern "C" int stvo_lsd_debug(stvo_lsd* o, int enable, double* out /* [seg_cap][8] or NULL */) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (o->prm.refine == 1) return STVO_ERR_UNSUPPORTED;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (enable && !o->dbg) {
        HIP_TRY(ctx, hipMalloc((void**)&o->dbg, (size_t)o->d.B * o->d.seg_cap * 64));
        if (!zero_device(ctx, o->dbg, (size_t)o->d.B * o->d.seg_cap * 64, "hipMemset lsd dbg")) return STVO_ERR_HIP;
    }
    o->d.dbg = enable ? o->dbg : nullptr;
    if (out && o->dbg) {  // (on the context's stream, which the kernels ran on: the null stream does not wait for it)
        HIP_TRY(ctx, hipMemcpyAsync(out, o->dbg, (size_t)o->d.seg_cap * 64, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return STVO_OK;
}

int stvo_keylines_xy_dev(stvo_ctx* ctx, int B, int stride, const stvo_keyline* lines, const int32_t* n_lines, float* kl_xy) {
    if (!ctx || B < 1 || stride < 1 || !lines || !n_lines || !kl_xy) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stvo::keylines_xy_kernel, dim3((stride + 255) / 256, B), dim3(256), 0, ctx->stream, stride, lines, n_lines,
                       reinterpret_cast<float4*>(kl_xy));
    return check_launch(ctx);
}

// What the last detection found BEFORE its cuts, per image: n_segments = segments of the detector core (at most 8192 are ranked),
// n_passing = those longer than min_length (n_lines = min(n_passing, nfeatures if set, max_keylines)).  A caller that asked for
// "keep all" (lsd_nfeatures = 0) learns here whether the capacity cut its lines.  Host arrays [B]; synchronises.
int stvo_lsd_counts(stvo_lsd* o, int32_t* n_segments, int32_t* n_passing) {
    if (!o || (!n_segments && !n_passing)) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::LsdDev& d = o->d;
    if (n_segments) HIP_TRY(ctx, hipMemcpyAsync(n_segments, d.n_seg, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_passing) HIP_TRY(ctx, hipMemcpyAsync(n_passing, d.n_pass, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_lsd_segments(stvo_lsd* o, const uint8_t* images, float* segments, int cap, int32_t* n_segments) {
    if (!o || !images || !segments || !n_segments || cap < 1) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::LsdDev& d = o->d;
    HIP_TRY(ctx, hipMemcpyAsync(o->img, images, (size_t)d.B * d.cols * d.rows, hipMemcpyHostToDevice, ctx->stream));
    TRY(lsd_enqueue(o, o->img, o->lines, o->response, o->n_lines));
    HIP_TRY(ctx, hipMemcpyAsync(n_segments, d.n_seg, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    const int take = cap < d.seg_cap ? cap : d.seg_cap;
    HIP_TRY(ctx, hipMemcpy2DAsync(segments, (size_t)cap * 16, d.seg, (size_t)d.seg_cap * 16, (size_t)take * 16, d.B, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_lsd_scaled_image(stvo_lsd* o, const uint8_t* images, uint8_t* scaled) {
    if (!o || !images || !scaled) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::LsdDev& d = o->d;
    HIP_TRY(ctx, hipMemcpyAsync(o->img, images, (size_t)d.B * d.cols * d.rows, hipMemcpyHostToDevice, ctx->stream));
    if (d.scale != 1) {
        lsd_scaled_enqueue(o, o->img);
        TRY(check_launch(ctx));
    }
    HIP_TRY(ctx, hipMemcpyAsync(scaled, d.scale != 1 ? o->scaled : o->img, (size_t)d.B * d.w * d.h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

}  // extern "C"
