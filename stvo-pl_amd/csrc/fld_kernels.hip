// fld_kernels.hip — the FLD key-line detector on gfx950: what the reference obtains with use_fld_lines = true from
//     createFastLineDetector(min_line_length)->detect(img, fld_lines)  + the top-N cut by length   (src/stereoFrame.cpp:244-303)
// through cv::ximgproc::FastLineDetector (OpenCV contrib 3.x) — third-party code the reference does not hold.  The semantics are
// those of the CPU statement tests/cpp/fld_ref.c (its header lists the points it defines: deterministic atan2 / sin / cos, no fused
// multiply-adds, cvRound half to even, stable ties, the float chain direction), against which these kernels are bit-exact
// (tests/test_gpu_fld.py).  Parity with OpenCV itself is unpinned.
//
//   fld_canny_kernel    one thread per pixel: Sobel 3 x 3 (replicated border), m = |dx| + |dy|, the three-case non-maximum
//                       suppression (TG22), m > floor(th1) (th1 == th2: hysteresis adds nothing), lineDetection's corner quirk;
//                       writes the 1-bit edge map (one ballot per 64 pixels) and the union-find labels' initial state
//   fld_union_kernel / fld_flatten_kernel   8-connected components of the edge map: atomic-min linking (root = the smallest raster
//                       index of the component), then every label points at its root
//   fld_hist / fld_scan / fld_scatter_kernel   the edge pixels grouped by component, raster order inside a component: a stable
//                       counting sort by root in two 10-bit passes (the form of lsd_hist / lsd_scan / lsd_scatter)
//   fld_walk_kernel     one workgroup per image, the edge map in LDS: one lane per component walks its pixels in raster order; each
//                       pixel still set starts a chain, which getPointChain follows exactly as the raster scan of lineDetection does
//                       (clears are LDS atomic ANDs: a word holds bits of several components)
//   fld_segments_kernel one lane per chain of at least L + 1 points: extractSegments, the length / border filters, the orientation
//                       by the brighter side (additionalOperationsOnSegment), in the statement's double and float operations
//   fld_order_kernel    detection order restored: segments by (seed raster index, position in the chain's list) through a scan of
//                       the segment counts per 32-pixel word of seeds
//   fld_keylines_kernel the top-N cut by double length (stable) and the stvo_keyline records / responses
//
// Exactness of the split by component.  getPointChain only moves to a SET 8-neighbour and only clears the pixels it moves to; a set
// 8-neighbour of an edge pixel lies in the same 8-connected component.  So the chains started from seeds of a component C consume
// only pixels of C, and the seed test at a pixel of C reads only that pixel's bit.  Hence C's seeds and chains are exactly those of
// walking C's pixels in raster order, whatever the other components do, and the reference's output order is that of the seeds'
// raster indices (then the position in the chain's segment list).
//
// Stores: a component's chains consume at most its own pixels, so the chain points of the component at sorted positions [s, e) are
// written to [s, e) of an image-sized store; a chain of n points gives at most n / (L + 1) segments, so the segments of the chain at
// point offset o go to slots [o / (L + 1), (o + n) / (L + 1)) of a store of npx / (L + 1) + 1 slots.  No store can fill; the walk
// still flags an overflow (stvo_fld_detect then returns STVO_ERR_CAPACITY) rather than drop a point.
//
// Every kernel is a template on MIXED: the MIXED instances read their image's row of a size table (one image size and length threshold
// per image, stvo_fld_set_image_sizes, csrc/fld_sizes.h), the others are the kernels as they were (fld_take_image below says what an
// image replaces and what stays the slot's).  Under a table an image's chain of n points at offset o goes to segment slots
// [o / (L_i + 1), (o + n) / (L_i + 1)) with its OWN threshold, in the stores cut for (the slot's pixels, the detector's L): the host
// takes an entry only if its own store fits them (fld_sizes.h: the store rule).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "ctx_internal.h"
#include "fast_atan2.h"
#include "fld_sizes.h"
#include "frontend_layout.h"
#include "line_common.h"
#include "table_transport.h"

#pragma clang fp contract(off)

namespace stvo {
namespace {

constexpr double FLD_PI = 3.14159265358979323846;
constexpr int FLD_WALK_T = 1024;
constexpr int FLD_KL_T = 256;
constexpr int FLD_SEG_BLOCKS = 8;              // workgroups per image of fld_segments_kernel (grid-stride over the chains)

struct FldDev {
    int B, cols, rows, npx, nw, nunits;
    int L, low, nfeatures, K, ch_cap, sg_cap;
    float dist_th;
    const uint8_t* img;  // [B][rows][cols]
    uint32_t* ebits;     // [B][nw] edge map, bit p & 31 of word p >> 5
    uint32_t* sbits;     // [B][nw] seeds of the chains that reached L + 1 points
    uint32_t* wsum;      // [B][nw] segments kept from the seeds of a word, then the detection index of its first one
    int32_t* lab;        // [B][npx] union-find labels, then the root of every edge pixel
    uint32_t* tmp;       // [B][npx] edge pixels by the root's low digit
    uint32_t* list;      // [B][npx] edge pixels by root, raster order inside a component
    uint32_t* cnt;       // [B][nunits][FLD_BINS] counting-sort counters, then first ranks
    int32_t* n_edge;     // [B]
    uint32_t* pts;       // [B][npx] chain points x | y << 16
    int32_t* ch_at;      // [B][npx] chain index at a surviving seed
    FldChain* ch;        // [B][ch_cap]
    int32_t* n_ch;       // [B]
    float4* sg;          // [B][sg_cap] segments at their chain's slots
    float4* dseg;        // [B][FLD_SEG_CAP] segments in detection order
    int32_t* n_seg;      // [B] segments found (before the cuts)
    int32_t* err;        // [B] a store overflowed (cannot happen; see the header)
    stvo_keyline* lines;
    float* response;
    int32_t* n_lines;
};

// One image size and length threshold per image (stvo_fld_set_image_sizes): FldTable<MIXED> (fld_sizes.h), an argument of its own behind
// FldDev and empty for the uniform instances — they take the arguments they always took.
//
// The image a workgroup works on.  MIXED = false: the slot itself — the kernel as it was, reading its argument.  MIXED = true: the
// kernel's own copy of its argument takes the image's size, pixels, edge words, sort units and threshold from the image's row of the
// table in place of the slot's, so the code below the call is one text for both.  Every kernel takes its image from a block index: the
// row is uniform over the workgroup and read with scalar loads.  The uniform instances do not make the call (if constexpr): their code
// is the code they had (profiles/mixed_fld_kernel_resources.txt).  FldSlot: the slot's pitch and per-image strides, taken before the
// call.  The strides BETWEEN images (the image buffer, lab, tmp, list, pts, ch_at: the slot's npx; ebits, sbits, wsum: its nw; cnt: its
// nunits; ch, sg: the stores' capacity; dseg) stay the slot's; INSIDE its block an image indexes compactly with its own cols (pixel p =
// y cols_i + x for labels, roots, edge bits and chain seeds: the detection order is the crop's own raster order).  Only Canny and
// orient_segment read the image bytes, at the slot's row pitch with the image's bounds.
//
// Why a table can never index outside the slot, and why the union-find terminates under one.  The host has validated the rows
// (fld_sizes.h), and the call clamps all the same: cols, rows, npx, nw and nunits into [.., the slot's], the threshold to the
// detector's where the stores cut for the slot would not hold the image under its own (the store rule), so a stale or torn table still
// addresses the slot's blocks only.  Every kernel of one detection reads the same table: it travels on the stream between detections,
// never between two kernels of one.  fld_canny_kernel initialises lab[p] = p for exactly the pixels p < npx_i (and the edge, seed and
// sum words w < nw_i); the union, the flatten, the sort and the walk of that launch read a label only at an edge pixel p < npx_i or at a
// neighbour inside the image's own bounds, whose compact index is below npx_i too — initialised by THIS launch, whatever an earlier
// launch under a larger or smaller table left beyond.  Labels only ever take the value of another such index and only decrease, so
// uf_find follows a strictly decreasing chain inside [0, npx_i) and ends; every other loop whose trip count comes from the table (the
// units of the scan, the words of the walk's LDS copy and of the order scan, the walk's blocks of 32 sorted positions up to n_edge <=
// npx_i) takes it after the clamp.
struct FldSlot {
    int cols, npx, nw, nunits;
};
__device__ __forceinline__ void fld_take_image(FldDev& d, const FldTable<true>& tab, int b) {
    const FldSizeRow* e = tab.sz + (b % tab.n_sz);
    d.cols = __builtin_amdgcn_readfirstlane(min(max(e->cols, 1), d.cols));
    d.rows = __builtin_amdgcn_readfirstlane(min(max(e->rows, 1), d.rows));
    d.npx = __builtin_amdgcn_readfirstlane(min(d.cols * d.rows, d.npx));  // (cols_i rows_i: what the row holds, once validated)
    d.nw = __builtin_amdgcn_readfirstlane(min(max(e->nw, (d.npx + 31) >> 5), d.nw));
    d.nunits = __builtin_amdgcn_readfirstlane(min(max(e->nunits, 1), d.nunits));
    const int L = __builtin_amdgcn_readfirstlane(max(e->L, 1));
    d.L = d.npx / (L + 1) + 1 <= d.sg_cap ? L : d.L;  // the store rule (fld_sizes.h); the detector's own always fits
}

// ---- the edge map ----
// (im: the image at row pitch `pitch`; cols, rows: its bounds — the replicated border is the image's own)
__device__ __forceinline__ void sobel_at(const uint8_t* im, int pitch, int cols, int rows, int x, int y, int& dx, int& dy) {
    const int xm = max(x - 1, 0), xp = min(x + 1, cols - 1), ym = max(y - 1, 0), yp = min(y + 1, rows - 1);
    const uint8_t *r0 = im + (size_t)ym * pitch, *r1 = im + (size_t)y * pitch, *r2 = im + (size_t)yp * pitch;
    dx = ((int)r0[xp] + 2 * (int)r1[xp] + (int)r2[xp]) - ((int)r0[xm] + 2 * (int)r1[xm] + (int)r2[xm]);
    dy = ((int)r2[xm] + 2 * (int)r2[x] + (int)r2[xp]) - ((int)r0[xm] + 2 * (int)r0[x] + (int)r0[xp]);
}
__device__ __forceinline__ int mag_at(const uint8_t* im, int pitch, int cols, int rows, int x, int y) {
    if (x < 0 || y < 0 || x >= cols || y >= rows) return 0;
    int dx, dy;
    sobel_at(im, pitch, cols, rows, x, y, dx, dy);
    return abs(dx) + abs(dy);
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_canny_kernel(FldDev d, FldTable<MIXED> tab) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    const uint8_t* im = d.img + (size_t)b * slot.npx;
    bool e = false;
    if (p < d.npx) {
        const int y = p / d.cols, x = p - y * d.cols;
        int dx, dy;
        sobel_at(im, slot.cols, d.cols, d.rows, x, y, dx, dy);
        const int m = abs(dx) + abs(dy);
        if (m > d.low) {
            const int TG22 = (int)(0.4142135623730950488 * (1 << 15) + 0.5);
            const int xs = abs(dx), ys = abs(dy) << 15, tg22x = xs * TG22;
            if (ys < tg22x) {
                e = m > mag_at(im, slot.cols, d.cols, d.rows, x - 1, y) && m >= mag_at(im, slot.cols, d.cols, d.rows, x + 1, y);
            } else if (ys > tg22x + (xs << 16)) {
                e = m > mag_at(im, slot.cols, d.cols, d.rows, x, y - 1) && m >= mag_at(im, slot.cols, d.cols, d.rows, x, y + 1);
            } else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                e = m > mag_at(im, slot.cols, d.cols, d.rows, x - s, y - 1) && m > mag_at(im, slot.cols, d.cols, d.rows, x + s, y + 1);
            }
        }
        if ((y < 6 && x < 6) || (y >= d.rows - 5 && x >= d.cols - 5)) e = false;  // lineDetection: canny(0..5, 0..5) = 0, the far corner too
        d.lab[(size_t)b * slot.npx + p] = p;
    }
    const unsigned long long bal = __ballot(e);
    const int w = ((blockIdx.x * 256 + (threadIdx.x & ~63)) >> 5) + (lane >> 5);
    if ((lane & 31) == 0 && w < d.nw) {
        const size_t q = (size_t)b * slot.nw + w;
        d.ebits[q] = (uint32_t)(bal >> (lane & 32));
        d.sbits[q] = 0u;
        d.wsum[q] = 0u;
    }
}

__device__ __forceinline__ bool ebit(const uint32_t* bits, int p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// ---- components: union-find with atomic-min linking ----
__device__ __forceinline__ int uf_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int uf_find(int32_t* L, int x) {
    int y;
    while ((y = uf_load(&L[x])) != x) x = y;  // labels only ever decrease towards the root
    return x;
}
__device__ void uf_unite(int32_t* L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(&L[b], a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(&L[a], b);
            if (old == a) return;
            a = old;
        }
    }
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_union_kernel(FldDev d, FldTable<MIXED> tab) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    if (p >= d.npx) return;
    const uint32_t* eb = d.ebits + (size_t)b * slot.nw;
    if (!ebit(eb, p)) return;
    int32_t* L = d.lab + (size_t)b * slot.npx;
    const int y = p / d.cols, x = p - y * d.cols;
    if (x > 0 && ebit(eb, p - 1)) uf_unite(L, p, p - 1);
    if (y > 0) {
        const int q = p - d.cols;
        if (x > 0 && ebit(eb, q - 1)) uf_unite(L, p, q - 1);
        if (ebit(eb, q)) uf_unite(L, p, q);
        if (x + 1 < d.cols && ebit(eb, q + 1)) uf_unite(L, p, q + 1);
    }
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_flatten_kernel(FldDev d, FldTable<MIXED> tab) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    if (p >= d.npx || !ebit(d.ebits + (size_t)b * slot.nw, p)) return;
    int32_t* L = d.lab + (size_t)b * slot.npx;
    L[p] = uf_find(L, p);
}

// ---- the edge pixels by root: stable counting sort, pass 0 by the low 10 bits (all pixels, raster order), pass 1 by the high ----
__device__ __forceinline__ bool sort_elem(const FldDev& d, const FldSlot& slot, int b, int pass, int i, uint32_t& val, int& digit) {
    const int32_t* L = d.lab + (size_t)b * slot.npx;
    if (pass == 0) {
        if (i >= d.npx || !ebit(d.ebits + (size_t)b * slot.nw, i)) return false;
        val = (uint32_t)i;
        digit = L[i] & (FLD_BINS - 1);
    } else {
        if (i >= d.n_edge[b]) return false;
        val = d.tmp[(size_t)b * slot.npx + i];
        digit = (L[val] >> 10) & (FLD_BINS - 1);
    }
    return true;
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_hist_kernel(FldDev d, int pass, FldTable<MIXED> tab) {
    __shared__ unsigned s_h[4][FLD_BINS];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y, unit = blockIdx.x * 4 + wv;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    if (unit >= d.nunits) return;
    unsigned* h = s_h[wv];
    for (int t = lane; t < FLD_BINS; t += 64) h[t] = 0u;
    for (int r = 0; r < FLD_UNIT_ROWS; ++r) {
        uint32_t v;
        int dg;
        if (sort_elem(d, slot, b, pass, unit * FLD_UNIT + r * 64 + lane, v, dg)) atomicAdd(&h[dg], 1u);
    }
    unsigned* out = d.cnt + ((size_t)b * slot.nunits + unit) * FLD_BINS;
    for (int t = lane; t < FLD_BINS; t += 64) out[t] = h[t];
}

template <bool MIXED>
__global__ __launch_bounds__(1024) void fld_scan_kernel(FldDev d, int pass, FldTable<MIXED> tab) {
    __shared__ unsigned s_w[16];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    unsigned* cnt = d.cnt + (size_t)b * slot.nunits * FLD_BINS;
    unsigned tot = 0u;
    for (int u = 0; u < d.nunits; ++u) tot += cnt[(size_t)u * FLD_BINS + t];
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        before += v < wv ? s_w[v] : 0u;
        all += s_w[v];
    }
    unsigned run = before + inc - tot;
    for (int u = 0; u < d.nunits; ++u) {
        const unsigned c = cnt[(size_t)u * FLD_BINS + t];
        cnt[(size_t)u * FLD_BINS + t] = run;
        run += c;
    }
    if (pass == 0 && t == 0) d.n_edge[b] = (int)all;
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_scatter_kernel(FldDev d, int pass, FldTable<MIXED> tab) {
    __shared__ unsigned s_h[4][FLD_BINS];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y, unit = blockIdx.x * 4 + wv;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    if (unit >= d.nunits) return;
    unsigned* h = s_h[wv];
    const unsigned* first = d.cnt + ((size_t)b * slot.nunits + unit) * FLD_BINS;
    for (int t = lane; t < FLD_BINS; t += 64) h[t] = first[t];
    uint32_t* out = (pass == 0 ? d.tmp : d.list) + (size_t)b * slot.npx;
    const unsigned long long lt = lane == 0 ? 0ull : ~0ull >> (64 - lane);
    for (int r = 0; r < FLD_UNIT_ROWS; ++r) {
        uint32_t v = 0;
        int dg = 0;
        const bool valid = sort_elem(d, slot, b, pass, unit * FLD_UNIT + r * 64 + lane, v, dg);
        unsigned long long m = __ballot(valid);  // ... the lanes of the row with this lane's digit
        if (!m) continue;                        // uniform
#pragma unroll
        for (int bit = 0; bit < 10; ++bit) {
            const bool one = (dg >> bit) & 1;
            const unsigned long long bb = __ballot(one);
            m &= one ? bb : ~bb;
        }
        if (valid) {
            const int rank = __builtin_popcountll(m & lt);
            const unsigned pos = h[dg] + (unsigned)rank;
            out[pos] = v;
            if (rank == 0) h[dg] = pos + (unsigned)__builtin_popcountll(m);  // (the lowest lane of the digit; one wave, LDS in order)
        }
    }
}

// ---- the walk: lineDetection's raster scan + getPointChain, one lane per component ----
__device__ __forceinline__ bool lbit(const uint32_t* s, int p) { return (s[p >> 5] >> (p & 31)) & 1u; }
__device__ __forceinline__ void lclear(uint32_t* s, int p) { atomicAnd(&s[p >> 5], ~(1u << (p & 31))); }

template <bool MIXED>
__global__ __launch_bounds__(FLD_WALK_T) void fld_walk_kernel(FldDev d, FldTable<MIXED> tab) {
    extern __shared__ uint32_t s_e[];  // [nw] the edge map of this image (the launch gives the slot's nw words)
    __shared__ int s_next, s_nch;
    const int b = blockIdx.x, tid = threadIdx.x;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    const uint32_t* eb = d.ebits + (size_t)b * slot.nw;
    for (int w = tid; w < d.nw; w += FLD_WALK_T) s_e[w] = eb[w];
    if (tid == 0) { s_next = 0; s_nch = 0; }
    __syncthreads();
    const int E = d.n_edge[b], cols = d.cols, rows = d.rows, L = d.L;
    const uint32_t* lst = d.list + (size_t)b * slot.npx;
    const int32_t* lab = d.lab + (size_t)b * slot.npx;
    uint32_t* pts = d.pts + (size_t)b * slot.npx;
    FldChain* ch = d.ch + (size_t)b * d.ch_cap;
    const int dyv[8] = {1, 1, 1, 0, -1, -1, -1, 0}, dxv[8] = {1, 0, -1, -1, -1, 0, 1, 1};
    for (;;) {
        const int a = atomicAdd(&s_next, 1) * 32;  // a block of 32 sorted positions: the components that START there are this lane's
        if (a >= E) break;
        const int a_end = min(a + 32, E);
        for (int j = a; j < a_end; ++j) {
            const int r = lab[lst[j]];
            if (j > 0 && lab[lst[j - 1]] == r) continue;  // not the first pixel of its component
            int w = j;                                     // the component's chain points go to pts[j ..)
            for (int k = j; k < E; ++k) {
                const int q = (int)lst[k];
                if (k > j && lab[q] != r) break;
                if (!lbit(s_e, q)) continue;
                // a seed: the chain from it (lineDetection :points.push_back(pt), getPointChain loop)
                int y = q / cols, x = q - y * cols;
                lclear(s_e, q);
                const int c0 = w;
                pts[w++] = (uint32_t)x | ((uint32_t)y << 16);
                float dir = 0.f;
                for (int step = 0;; ++step) {
                    float mind = 7.0f;
                    int cx = 0, cy = 0, cd = 0;
                    bool first = false;
                    for (int i = 0; i < 8; ++i) {
                        const int ci = x + dxv[i], ri = y + dyv[i];
                        if (ri < 0 || ri == rows || ci < 0 || ci == cols) continue;
                        if (!lbit(s_e, ri * cols + ci)) continue;
                        const int dd = i > 4 ? i - 8 : i;
                        if (step == 0) {
                            cx = ci; cy = ri; cd = dd;
                            first = true;
                            break;
                        }
                        float df = fabsf((float)dd - dir);
                        df = df > 4 ? 8 - df : df;
                        if (df <= mind) {
                            mind = df;
                            cx = ci; cy = ri; cd = dd;
                        }
                    }
                    if (step == 0) {
                        if (!first) break;
                        dir = (float)cd;
                    } else {
                        if (!(mind < 2)) break;
                        dir = __fdiv_rn(dir * (float)step + (float)cd, (float)(step + 1));
                    }
                    x = cx; y = cy;
                    pts[w++] = (uint32_t)x | ((uint32_t)y << 16);
                    lclear(s_e, y * cols + x);
                }
                const int n = w - c0;
                if (n < L + 1) {  // dropped: its pixels stay consumed, its points are overwritten
                    w = c0;
                    continue;
                }
                const int idx = atomicAdd(&s_nch, 1);
                if (idx < d.ch_cap) {
                    FldChain c;
                    c.seed = q; c.off = c0; c.n = n; c.nseg = 0;
                    ch[idx] = c;
                    d.ch_at[(size_t)b * slot.npx + q] = idx;
                    atomicOr(&d.sbits[(size_t)b * slot.nw + (q >> 5)], 1u << (q & 31));
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        d.n_ch[b] = min(s_nch, d.ch_cap);
        d.err[b] = s_nch > d.ch_cap ? 1 : 0;
    }
}

// ---- extractSegments and what lineDetection does with a segment ----
__device__ __forceinline__ uint32_t pt_ld(const uint32_t* P, int i) { return P[i]; }
__device__ __forceinline__ int pt_x(uint32_t v) { return (int)(v & 0xFFFFu); }
__device__ __forceinline__ int pt_y(uint32_t v) { return (int)(v >> 16); }

// fdlibm s_atan.c / e_atan2.c: tests/cpp/fld_ref.c fld_atan2_det, operation for operation
__device__ double atan_det(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double T0 = 3.33333333333329318027e-01, T1 = -1.99999999998764832476e-01, T2 = 1.42857142725034663711e-01,
                 T3 = -1.11111104054623557880e-01, T4 = 9.09088713343650656196e-02, T5 = -7.69187620504482999495e-02,
                 T6 = 6.66107313738753120669e-02, T7 = -5.83357013379057348645e-02, T8 = 4.97687799461593236017e-02,
                 T9 = -3.65315727442169155270e-02, T10 = 1.62858201153657823623e-02;
    const long long u = __double_as_longlong(x);
    const int hx = (int)(u >> 32), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) {
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && (unsigned)u != 0u)) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {
        if (ix < 0x3e400000) return x;
        id = -1;
    } else {
        x = fabs(x);
        if (ix < 0x3ff30000) {
            if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
            else { id = 1; x = (x - 1.0) / (x + 1.0); }
        } else {
            if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
            else { id = 3; x = -1.0 / x; }
        }
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (T0 + w * (T2 + w * (T4 + w * (T6 + w * (T8 + w * T10)))));
    const double s2 = w * (T1 + w * (T3 + w * (T5 + w * (T7 + w * T9))));
    if (id < 0) return x - x * (s1 + s2);
    const double r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -r : r;
}

__device__ double atan2_det(double y, double x) {
    const double pi_o_4 = 7.8539816339744827900e-01, pi_o_2 = 1.5707963267948965580e+00, pi = 3.1415926535897931160e+00,
                 pi_lo = 1.2246467991473531772e-16;
    const long long ux = __double_as_longlong(x), uy = __double_as_longlong(y);
    const int hx = (int)(ux >> 32), ix = hx & 0x7fffffff, hy = (int)(uy >> 32), iy = hy & 0x7fffffff;
    const unsigned lx = (unsigned)ux, ly = (unsigned)uy;
    if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0u) || iy > 0x7ff00000 || (iy == 0x7ff00000 && ly != 0u)) return x + y;
    if (hx == 0x3ff00000 && lx == 0u) return atan_det(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if ((iy | (int)ly) == 0) {
        if (m < 2) return y;
        return m == 2 ? pi : -pi;
    }
    if ((ix | (int)lx) == 0) return hy < 0 ? -pi_o_2 : pi_o_2;
    if (ix == 0x7ff00000) {
        if (iy == 0x7ff00000) return m == 0 ? pi_o_4 : (m == 1 ? -pi_o_4 : (m == 2 ? 3.0 * pi_o_4 : -3.0 * pi_o_4));
        return m == 0 ? 0.0 : (m == 1 ? -0.0 : (m == 2 ? pi : -pi));
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 : pi_o_2;
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0;
    else z = atan_det(fabs(y / x));
    return m == 0 ? z : (m == 1 ? -z : (m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi));
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dist_point_line(double* l, double px, double py) {  // normalises l in place
    const double x = l[0], y = l[1], w = sqrt(x * x + y * y);
    l[0] = x / w; l[1] = y / w; l[2] = l[2] / w;
    return l[0] * px + l[1] * py + l[2] * 1.0;
}
__device__ void fit_line(const uint32_t* P, int n, double* l) {
    double x = 0, y = 0, x2 = 0, y2 = 0, xy = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t v = pt_ld(P, i);
        const float fx = (float)pt_x(v), fy = (float)pt_y(v);
        x += fx; y += fy;
        x2 += fx * fx; y2 += fy * fy; xy += fx * fy;
    }
    const double w = (float)n;
    x /= w; y /= w; x2 /= w; y2 /= w; xy /= w;
    const double dx2 = x2 - x * x, dy2 = y2 - y * y, dxy = xy - x * y;
    const float t = __fdiv_rn((float)atan2_det(2 * dxy, dx2 - dy2), 2.0f);
    double s, c;
    sincos_det((double)t, s, c);
    const float vx = (float)c, vy = (float)s, x0 = (float)x, y0 = (float)y;
    const double a[3] = {x0, y0, 1.0}, bb[3] = {(double)(x0 + vx), (double)(y0 + vy), 1.0};
    cross3(a, bb, l);
}
__device__ __forceinline__ void incident_point(const double* l, float& px, float& py, int cols, int rows) {
    const double a[3] = {(double)px, (double)py, 1.0}, bb[3] = {l[0], l[1], 0.0};
    double lk[3], xk[3];
    cross3(a, bb, lk);
    cross3(lk, l, xk);
    const double sc = 1.0 / xk[2];
    const float fx = (float)(xk[0] * sc + 0.0), fy = (float)(xk[1] * sc + 0.0);
    const float wm = (float)cols - 1.0f, hm = (float)rows - 1.0f;
    px = fx < 0.0f ? 0.0f : (fx >= wm ? wm : fx);
    py = fy < 0.0f ? 0.0f : (fy >= hm ? hm : fy);
}

// lineDetection's filters; true: keep
__device__ __forceinline__ bool keep_segment(float4 s, int L, int cols, int rows) {
    const float a = s.x - s.z, c = s.y - s.w;
    const float len = __fsqrt_rn(a * a + c * c);
    if (len < (float)L) return false;
    return !((s.x <= 5.0f && s.z <= 5.0f) || (s.y <= 5.0f && s.w <= 5.0f) || (s.x >= (float)cols - 5.0f && s.z >= (float)cols - 5.0f) ||
             (s.y >= (float)rows - 5.0f && s.w >= (float)rows - 5.0f));
}
// additionalOperationsOnSegment: the end points swapped when the right side is brighter
__device__ float4 orient_segment(const uint8_t* im, int pitch, int cols, int rows, float4 s) {
    const double ang = (double)(float)((double)__fdiv_rn(fast_atan2_deg(s.w - s.y, s.z - s.x), 180.0f) * FLD_PI);
    const double dx = (double)s.z - (double)s.x, dy = (double)s.w - (double)s.y;
    double sn, cs;
    sincos_det(90.0 * FLD_PI / 180.0 + ang, sn, cs);
    int iR = 0, iL = 0;
    for (int i = 0; i < 10; ++i) {
        float qx, qy;
        if (i == 0) { qx = s.x; qy = s.y; }
        else if (i == 9) { qx = s.z; qy = s.w; }
        else {
            qx = s.x + (__fdiv_rn((float)dx, 9.0f) * (float)i);
            qy = s.y + (__fdiv_rn((float)dy, 9.0f) * (float)i);
        }
        int rx = (int)__builtin_rint(qx + 1.0 * cs), ry = (int)__builtin_rint(qy + 1.0 * sn);
        int lx = (int)__builtin_rint(qx - 1.0 * cs), ly = (int)__builtin_rint(qy - 1.0 * sn);
        rx = rx <= 5 ? 5 : (rx >= cols - 5 ? cols - 5 : rx);
        ry = ry <= 5 ? 5 : (ry >= rows - 5 ? rows - 5 : ry);
        lx = lx <= 5 ? 5 : (lx >= cols - 5 ? cols - 5 : lx);
        ly = ly <= 5 ? 5 : (ly >= rows - 5 ? rows - 5 : ly);
        iR += im[(size_t)ry * pitch + rx];
        iL += im[(size_t)ly * pitch + lx];
    }
    return iR > iL ? make_float4(s.z, s.w, s.x, s.y) : s;
}

template <bool MIXED>
__global__ __launch_bounds__(256) void fld_segments_kernel(FldDev d, FldTable<MIXED> tab) {
    const int b = blockIdx.y;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    const int nch = d.n_ch[b], L = d.L, cols = d.cols, rows = d.rows;
    const double th = (double)d.dist_th;
    const uint8_t* im = d.img + (size_t)b * slot.npx;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < nch; c += FLD_SEG_BLOCKS * 256) {
        FldChain chn = d.ch[(size_t)b * d.ch_cap + c];
        const uint32_t* P = d.pts + (size_t)b * slot.npx + chn.off;
        const int total = chn.n;
        float4* out = d.sg + (size_t)b * d.sg_cap + chn.off / (L + 1);
        int kept = 0;
        for (int i = 0; i + L < total; i++) {
            double l[3];
            {
                const uint32_t u0 = pt_ld(P, i), u1 = pt_ld(P, i + L);
                const double a[3] = {(double)pt_x(u0), (double)pt_y(u0), 1.0}, bb[3] = {(double)pt_x(u1), (double)pt_y(u1), 1.0};
                cross3(a, bb, l);
            }
            bool fail = false;
            for (int j = 1; j < L; j++) {
                const uint32_t u = pt_ld(P, i + j);
                if (fabs(dist_point_line(l, (double)pt_x(u), (double)pt_y(u))) > th) { fail = true; break; }
            }
            if (fail) continue;
            int cnt = L + 1;
            uint32_t pe = pt_ld(P, i + L);
            fit_line(P + i, cnt, l);
            const uint32_t u0 = pt_ld(P, i);
            float psx = (float)pt_x(u0), psy = (float)pt_y(u0);
            incident_point(l, psx, psy, cols, rows);
            const int psi = (int)__builtin_rintf(psx), psj = (int)__builtin_rintf(psy);
            int j;
            for (j = L + 1; i + j < total; j++) {
                const uint32_t pt = pt_ld(P, i + j);
                const double ptx = (double)pt_x(pt), pty = (double)pt_y(pt);
                double dd = dist_point_line(l, ptx, pty);
                if (fabs(dd) > th) {
                    fit_line(P + i, cnt, l);
                    dd = dist_point_line(l, ptx, pty);
                    if (fabs(dd) > th) { j--; break; }
                }
                pe = pt;
                cnt++;
            }
            fit_line(P + i, cnt, l);
            float e1x = (float)psi, e1y = (float)psj, e2x = (float)pt_x(pe), e2y = (float)pt_y(pe);
            incident_point(l, e1x, e1y, cols, rows);
            incident_point(l, e2x, e2y, cols, rows);
            const float4 s = make_float4(e1x, e1y, e2x, e2y);
            if (keep_segment(s, L, cols, rows)) out[kept++] = orient_segment(im, slot.cols, cols, rows, s);
            i = i + j;
        }
        d.ch[(size_t)b * d.ch_cap + c].nseg = kept;
        if (kept) atomicAdd(&d.wsum[(size_t)b * slot.nw + (chn.seed >> 5)], (unsigned)kept);
    }
}

// ---- detection order: scan of the per-word segment counts, then every chain's segments to their place ----
template <bool MIXED>
__global__ __launch_bounds__(1024) void fld_order_kernel(FldDev d, FldTable<MIXED> tab) {
    __shared__ unsigned s_w[16];
    __shared__ unsigned s_total;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const FldSlot slot{d.cols, d.npx, d.nw, d.nunits};
    if constexpr (MIXED) fld_take_image(d, tab, b);
    uint32_t* ws = d.wsum + (size_t)b * slot.nw;
    const int per = (d.nw + 1023) / 1024, w0 = min(t * per, d.nw), w1 = min(w0 + per, d.nw);
    unsigned tot = 0u;
    for (int w = w0; w < w1; ++w) tot += ws[w];
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        before += v < wv ? s_w[v] : 0u;
        all += s_w[v];
    }
    unsigned run = before + inc - tot;
    for (int w = w0; w < w1; ++w) {
        const unsigned c = ws[w];
        ws[w] = run;
        run += c;
    }
    if (t == 0) s_total = all;
    __syncthreads();
    const int nch = d.n_ch[b];
    const FldChain* ch = d.ch + (size_t)b * d.ch_cap;
    const uint32_t* sb = d.sbits + (size_t)b * slot.nw;
    const int32_t* at = d.ch_at + (size_t)b * slot.npx;
    for (int c = t; c < nch; c += 1024) {
        const FldChain q = ch[c];
        if (q.nseg == 0) continue;
        const int w = q.seed >> 5;
        unsigned o = ws[w];
        unsigned below = sb[w] & ((1u << (q.seed & 31)) - 1u);  // earlier seeds of the same word
        while (below) {
            const int bit = __builtin_ctz(below);
            below &= below - 1u;
            o += (unsigned)ch[at[(w << 5) + bit]].nseg;
        }
        const float4* src = d.sg + (size_t)b * d.sg_cap + q.off / (d.L + 1);
        for (int k = 0; k < q.nseg && o + (unsigned)k < (unsigned)FLD_SEG_CAP; ++k) d.dseg[(size_t)b * FLD_SEG_CAP + o + k] = src[k];
    }
    if (t == 0) d.n_seg[b] = (int)s_total;
}

// ---- stereoFrame.cpp:250-298: the cut by length and the KeyLine records ----
__device__ __forceinline__ double sort_length(float4 e) {  // sort_flines_by_length (auxiliar.h:149-154); the squares are exact
    const double a = (double)(e.x - e.z), c = (double)(e.y - e.w);
    return sqrt(a * a + c * c);
}

template <bool MIXED>
__global__ __launch_bounds__(FLD_KL_T) void fld_keylines_kernel(FldDev d, FldTable<MIXED> tab) {
    extern __shared__ double s_len[];  // [FLD_SEG_CAP]
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (MIXED) fld_take_image(d, tab, b);  // (the response divisor and the raster of the pixel count are the image's own)
    const int m = min(d.n_seg[b], FLD_SEG_CAP);
    const float4* seg = d.dseg + (size_t)b * FLD_SEG_CAP;
    for (int i = tid; i < m; i += FLD_KL_T) s_len[i] = sort_length(seg[i]);
    __syncthreads();
    const int n_out = min(d.nfeatures != 0 ? min(d.nfeatures, m) : m, d.K);
    const bool cut = m > n_out;
    const float mx = (float)(d.cols > d.rows ? d.cols : d.rows);
    for (int i = tid; i < m; i += FLD_KL_T) {
        const double li = s_len[i];
        int rank = i;
        if (cut) {  // position in the stable descending order of the lengths
            rank = 0;
            for (int j = 0; j < m; ++j) {
                const double q = s_len[j];
                rank += (q > li || (q == li && j < i)) ? 1 : 0;
            }
        }
        if (rank >= n_out) continue;
        const float4 e = seg[i];
        stvo_keyline kl;
        kl.sx = e.x; kl.sy = e.y; kl.ex = e.z; kl.ey = e.w;
        kl.angle = (float)atan2_det((double)(e.w - e.y), (double)(e.z - e.x));
        kl.num_pixels = line_iterator_count(d.cols, d.rows, e.x, e.y, e.z, e.w);
        d.lines[(size_t)b * d.K + rank] = kl;
        if (d.response) d.response[(size_t)b * d.K + rank] = __fdiv_rn((float)li, mx);
    }
    if (tid == 0) d.n_lines[b] = n_out;
}

}  // namespace
}  // namespace stvo

struct stvo_fld {
    stvo_ctx* ctx = nullptr;
    stvo::FldDev d{};
    stvo_fld_params prm{};
    char* dev = nullptr;
    uint8_t* img = nullptr;         // device buffers of the host-pointer entry points
    stvo_keyline* lines = nullptr;
    float* response = nullptr;
    int32_t* n_lines = nullptr;
    int walk_lds = 0;
    // one image size and threshold per image (stvo_fld_set_image_sizes): nothing of it exists until the first call.  The device table
    // holds the n rows the kernels read (FldSizeRow); `rows` is the host's copy of the table in force (stvo_fld_edges unpacks with it)
    stvo_detail::TableTransport sizes;
    std::vector<stvo::FldSizeRow> rows;
    int n_sizes = 0;          // entries of the table in force; 0: every image fills its slot
};

namespace {

template <bool MIXED>
void fld_launch(stvo_fld* o, const stvo::FldDev& d, dim3 pg, dim3 ug, stvo::FldTable<MIXED> tab) {
    hipStream_t s = o->ctx->stream;
    hipLaunchKernelGGL(stvo::fld_canny_kernel<MIXED>, pg, dim3(256), 0, s, d, tab);
    hipLaunchKernelGGL(stvo::fld_union_kernel<MIXED>, pg, dim3(256), 0, s, d, tab);
    hipLaunchKernelGGL(stvo::fld_flatten_kernel<MIXED>, pg, dim3(256), 0, s, d, tab);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(stvo::fld_hist_kernel<MIXED>, ug, dim3(256), 0, s, d, pass, tab);
        hipLaunchKernelGGL(stvo::fld_scan_kernel<MIXED>, dim3(d.B), dim3(1024), 0, s, d, pass, tab);
        hipLaunchKernelGGL(stvo::fld_scatter_kernel<MIXED>, ug, dim3(256), 0, s, d, pass, tab);
    }
    hipLaunchKernelGGL(stvo::fld_walk_kernel<MIXED>, dim3(d.B), dim3(stvo::FLD_WALK_T), o->walk_lds, s, d, tab);
    hipLaunchKernelGGL(stvo::fld_segments_kernel<MIXED>, dim3(stvo::FLD_SEG_BLOCKS, d.B), dim3(256), 0, s, d, tab);
    hipLaunchKernelGGL(stvo::fld_order_kernel<MIXED>, dim3(d.B), dim3(1024), 0, s, d, tab);
    hipLaunchKernelGGL(stvo::fld_keylines_kernel<MIXED>, dim3(d.B), dim3(stvo::FLD_KL_T), (size_t)stvo::FLD_SEG_CAP * 8, s, d, tab);
}

int fld_enqueue(stvo_fld* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    stvo_ctx* ctx = o->ctx;
    stvo::FldDev d = o->d;
    d.img = images;
    d.lines = lines; d.response = response; d.n_lines = n_lines;
    const dim3 pg((d.npx + 255) / 256, d.B), ug((d.nunits + 3) / 4, d.B);
    if (o->n_sizes) {
        // One size per image: the MIXED instances of every kernel on the slot's launch grids and LDS; threads beyond an image's pixels or
        // units leave as those beyond the slot's do.
        const stvo::FldTable<true> tab{reinterpret_cast<const stvo::FldSizeRow*>(o->sizes.dev), o->n_sizes};
        fld_launch<true>(o, d, pg, ug, tab);
    } else {
        const stvo::FldTable<false> none{};  // the uniform instances: the kernels and arguments of a detector that was never given a table
        fld_launch<false>(o, d, pg, ug, none);
    }
    return check_launch(ctx);
}

int fld_run_host(stvo_fld* o, const uint8_t* images) {
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipMemcpyAsync(o->img, images, (size_t)o->d.B * o->d.npx, hipMemcpyHostToDevice, ctx->stream));
    return fld_enqueue(o, o->img, o->lines, o->response, o->n_lines);
}

}  // namespace

extern "C" {

int stvo_fld_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keylines, const stvo_fld_params* prm, stvo_fld** out) {
    if (!ctx || !prm || !out || B < 1 || cols < 16 || rows < 16 || max_keylines < 1 || prm->nfeatures < 0 || prm->length_threshold < 1 ||
        !(prm->distance_threshold >= 0) || !(prm->canny_th1 >= 0) || !(prm->canny_th2 >= 0))
        return STVO_ERR_INVALID_ARG;
    // not built (no caller of the reference reaches them): merging, hysteresis (th1 != th2), other apertures, images above 2^20 pixels
    if (prm->do_merge != 0 || prm->canny_aperture_size != 3 || prm->canny_th1 != prm->canny_th2 || (long long)cols * rows > (1ll << 20))
        return STVO_ERR_UNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_fld* o = new (std::nothrow) stvo_fld();
    if (!o) return STVO_ERR_HIP;
    o->ctx = ctx;
    o->prm = *prm;
    stvo::FldDev& d = o->d;
    d.B = B; d.cols = cols; d.rows = rows; d.npx = cols * rows;
    d.nw = stvo::fld_words(d.npx);
    d.nunits = stvo::fld_units(d.npx);
    d.L = prm->length_threshold;
    d.low = (int)std::floor(prm->canny_th1 < 32767.0 ? prm->canny_th1 : 32767.0);
    d.dist_th = prm->distance_threshold;
    d.nfeatures = prm->nfeatures;
    d.K = max_keylines;
    d.ch_cap = d.sg_cap = stvo::fld_store_cap(d.npx, d.L);
    stvo::Carver size;
    stvo::carve_fld_arena(size, B, cols, rows, d.L, d.K);
    bool ok = hip_ok(ctx, hipMalloc((void**)&o->dev, size.off), "hipMalloc fld") && zero_device(ctx, o->dev, size.off, "hipMemset fld");
    if (ok) {
        stvo::Carver c(o->dev);
        const stvo::FldArena a = stvo::carve_fld_arena(c, B, cols, rows, d.L, d.K);
        o->img = a.img;
        d.ebits = a.ebits; d.sbits = a.sbits; d.wsum = a.wsum; d.lab = a.lab; d.tmp = a.tmp; d.list = a.list;
        d.cnt = a.cnt; d.n_edge = a.n_edge; d.pts = a.pts; d.ch_at = a.ch_at; d.ch = a.ch; d.n_ch = a.n_ch;
        d.sg = a.sg; d.dseg = a.dseg; d.n_seg = a.n_seg; d.err = a.err;
        o->lines = a.lines; o->response = a.response; o->n_lines = a.n_lines;
    }
    o->walk_lds = d.nw * 4;
    if (ok && o->walk_lds > 48 * 1024)
        ok = stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::fld_walk_kernel<false>), o->walk_lds) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::fld_walk_kernel<true>), o->walk_lds);
    if (ok)
        ok = stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::fld_keylines_kernel<false>), stvo::FLD_SEG_CAP * 8) &&
             stvo::lds_opt_in(reinterpret_cast<const void*>(stvo::fld_keylines_kernel<true>), stvo::FLD_SEG_CAP * 8);
    if (!ok) {
        stvo_fld_destroy(o);
        return STVO_ERR_HIP;
    }
    *out = o;
    return STVO_OK;
}

int stvo_fld_destroy(stvo_fld* o) {
    if (!o) return STVO_OK;
    if (o->ctx) {
        (void)hipSetDevice(o->ctx->device);
        (void)hipStreamSynchronize(o->ctx->stream);
    }
    if (o->dev) (void)hipFree(o->dev);
    o->sizes.destroy();
    delete o;
    return STVO_OK;
}

// One image size and length threshold per image (stvo_hip.h).  Validated before anything changes; the table is formed with the
// functions stvo_fld_create forms the slot's own values with (fld_sizes.h) and travels as table_transport.h says.
int stvo_fld_set_image_sizes(stvo_fld* o, const int32_t* sizes_host, const int32_t* length_threshold_host, int n) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (!sizes_host) {  // every image fills its slot again: the uniform kernel instances, which read no table
        o->n_sizes = 0;
        o->rows.clear();
        return STVO_OK;
    }
    const stvo::FldDev& d = o->d;
    stvo_ctx* ctx = o->ctx;
    int entry = 0, need = 0, have = 0;
    switch (stvo::fld_image_sizes_verdict(sizes_host, length_threshold_host, n, d.B, d.cols, d.rows, d.L, &entry, &need, &have)) {
        case stvo::FLD_SIZES_OK: break;
        case stvo::FLD_SIZES_CAPACITY:
            std::snprintf(ctx->last_error, sizeof(ctx->last_error),
                          "stvo_fld_set_image_sizes: entry %d (%d x %d, length threshold %d) needs a store of %d segments, the detector's "
                          "(%d x %d, length threshold %d) holds %d: create the detector with the smallest threshold it will be given",
                          entry, sizes_host[2 * entry], sizes_host[2 * entry + 1], stvo::fld_entry_threshold(length_threshold_host, entry, d.L),
                          need, d.cols, d.rows, d.L, have);
            return STVO_ERR_CAPACITY;
        default: return STVO_ERR_INVALID_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<stvo::FldSizeRow> rows((size_t)n);
    for (int i = 0; i < n; ++i)
        rows[i] = stvo::fld_size_row(sizes_host[2 * i], sizes_host[2 * i + 1], stvo::fld_entry_threshold(length_threshold_host, i, d.L));
    char* tab = o->sizes.begin(ctx, (size_t)d.B * sizeof(stvo::FldSizeRow));
    if (!tab) return STVO_ERR_HIP;
    std::memcpy(tab, rows.data(), (size_t)n * sizeof(stvo::FldSizeRow));
    TRY(o->sizes.send(ctx, (size_t)n * sizeof(stvo::FldSizeRow)));
    o->rows.swap(rows);
    o->n_sizes = n;
    return STVO_OK;
}

int stvo_fld_detect_dev(stvo_fld* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    if (!o || !images || !lines || !n_lines) return STVO_ERR_INVALID_ARG;
    HIP_TRY(o->ctx, hipSetDevice(o->ctx->device));
    return fld_enqueue(o, images, lines, response, n_lines);
}

// the overflow flags of the last detection (synchronises): STVO_ERR_CAPACITY when a store filled up
static int fld_check(stvo_fld* o) {
    stvo_ctx* ctx = o->ctx;
    std::vector<int32_t> err((size_t)o->d.B);
    HIP_TRY(ctx, hipMemcpyAsync(err.data(), o->d.err, (size_t)o->d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t e : err)
        if (e) {
            std::snprintf(ctx->last_error, sizeof(ctx->last_error), "stvo_fld: a chain store filled up");
            return STVO_ERR_CAPACITY;
        }
    return STVO_OK;
}

int stvo_fld_detect(stvo_fld* o, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines) {
    if (!o || !images || !lines || !n_lines) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::FldDev& d = o->d;
    TRY(fld_run_host(o, images));
    HIP_TRY(ctx, hipMemcpyAsync(lines, o->lines, (size_t)d.B * d.K * sizeof(stvo_keyline), hipMemcpyDeviceToHost, ctx->stream));
    if (response) HIP_TRY(ctx, hipMemcpyAsync(response, o->response, (size_t)d.B * d.K * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_lines, o->n_lines, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    return fld_check(o);
}

int stvo_fld_counts(stvo_fld* o, int32_t* n_segments) {
    if (!o || !n_segments) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(n_segments, o->d.n_seg, (size_t)o->d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_fld_segments(stvo_fld* o, const uint8_t* images, float* segments, int cap, int32_t* n_segments) {
    if (!o || !images || !segments || !n_segments || cap < 1) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::FldDev& d = o->d;
    TRY(fld_run_host(o, images));
    HIP_TRY(ctx, hipMemcpyAsync(n_segments, d.n_seg, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    const int take = cap < stvo::FLD_SEG_CAP ? cap : stvo::FLD_SEG_CAP;
    HIP_TRY(ctx, hipMemcpy2DAsync(segments, (size_t)cap * 16, d.dseg, (size_t)stvo::FLD_SEG_CAP * 16, (size_t)take * 16, d.B,
                                  hipMemcpyDeviceToHost, ctx->stream));
    return fld_check(o);
}

int stvo_fld_edges(stvo_fld* o, const uint8_t* images, uint8_t* edges) {
    if (!o || !images || !edges) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::FldDev& d = o->d;
    TRY(fld_run_host(o, images));
    std::vector<uint32_t> bits((size_t)d.B * d.nw);
    HIP_TRY(ctx, hipMemcpyAsync(bits.data(), d.ebits, bits.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    TRY(fld_check(o));
    if (o->n_sizes) {  // under a table the bits are compact at the image's own cols: its edge map top-left in the slot, 0 around it
        std::memset(edges, 0, (size_t)d.B * d.npx);
        for (int b = 0; b < d.B; ++b) {
            const stvo::FldSizeRow& e = o->rows[(size_t)(b % o->n_sizes)];
            for (int y = 0; y < e.rows; ++y)
                for (int x = 0; x < e.cols; ++x) {
                    const int p = y * e.cols + x;
                    edges[(size_t)b * d.npx + (size_t)y * d.cols + x] = ((bits[(size_t)b * d.nw + (p >> 5)] >> (p & 31)) & 1u) ? 255 : 0;
                }
        }
        return STVO_OK;
    }
    for (int b = 0; b < d.B; ++b)
        for (int p = 0; p < d.npx; ++p)
            edges[(size_t)b * d.npx + p] = ((bits[(size_t)b * d.nw + (p >> 5)] >> (p & 31)) & 1u) ? 255 : 0;
    return STVO_OK;
}

}  // extern "C"
