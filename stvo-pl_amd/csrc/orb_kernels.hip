// orb_kernels.hip — the ORB point front-end on gfx950: what the reference obtains from
//     cv::ORB::create(...)->detectAndCompute(img, Mat(), points, pdesc, false)     (/root/reference/src/stereoFrame.cpp:104-118)
// for orb_nlevels pyramid levels (config_kitti.yaml: 1; config_euroc.yaml / src/config.cpp:96-97: 4 at scale 1.2), FAST_SCORE
// ranking (orb_score 1, the default) or HARRIS_SCORE ranking (orb_score 0: stvo_orb_set_score_type), WTA_K 2 and patch 31 by default,
// orb_wta_k 2 / 3 / 4 and orb_patch_size 2 .. 63 with stvo_orb_set_descriptor (OpenCV's RNG-derived test patterns: csrc/orb_pattern.h;
// a patch size other than 31 needs orb_edge_th >= ceil((P / 2) sqrt 2), and patch sizes above 63 are not built).  Per level:
//   orb_fast_nms_kernel  FAST-9/16 score (cornerScore<16>) + 3x3 non-maximum suppression + border filter per 64 x 64 tile, all in
//                        LDS: compass-point rejection, candidates compacted so that the full score runs on dense lanes;
//                        survivors go to a per-image list + response histogram (no score map in global memory)
//   orb_order_kernel     KeyPointsFilter::retainBest as a histogram cut (ties kept) + row-major ordering (bitonic sort in LDS)
//   orb_harris_kernel    (orb_score 0 only) HarrisResponses of the 2 n FAST-best key-points, 8 lanes per key-point; the ordering
//                        kernel then cuts at the exact n-th largest response (radix select on the float keys, ties kept)
//   orb_blur_kernel      GaussianBlur 7x7, sigma 2, 8-bit fixed point, BORDER_REFLECT_101
//   orb_describe_kernel  intensity-centroid angle (ICAngles, fastAtan2) + rotated BRIEF, 16 lanes per key-point: (WTA_K 2, patch 31) only
//   orb_describe_wta_kernel<WTA_K, reach>  the same for every other setting: any half patch, 2-bit fields for WTA_K 3 / 4, one wave per
//                        key-point (six instances: WTA_K 2 / 3 / 4 x an LDS patch for reach <= 22 or <= 44)
// around them (more than one level): orb_resize_kernel (level l from level l - 1, OpenCV's 8-bit bilinear resize in 11-bit fixed
// point) and orb_concat_kernel (levels in order, coordinates x scale, octave = level).
// One image size per image (stvo_orb_set_image_sizes): the three kernels that see an image border — FAST + NMS, blur, resize — are templates on
// MIXED; the MIXED instances read their image's row of a size table (csrc/orb_sizes.h), the others are the kernels as they were.
// OpenCV is third-party code that is not under /root/reference: the semantics are those of oracle/stvo_orb_oracle.c (a
// restatement of OpenCV's algorithm, parity unpinned), against which these kernels are bit-exact (tests/test_gpu_orb.py); the settings
// other than (2, 31) are pinned to the numpy statement tests/np_orb_wta.py in the same way (tests/test_gpu_orb_wta.py).
// Integer / byte work throughout; the only floating point is the angle polynomial and the rotation of the test pattern, in
// FP32 exactly as OpenCV evaluates them (no fused multiply-adds).
#include <cmath>
#include <cstring>
#include <new>

#include "ctx_internal.h"
#include "fast_atan2.h"
#include "frontend_layout.h"
#include "gaussian_q8.h"
#include "orb_pattern.h"
#include "orb_rotate.h"
#include "orb_sizes.h"

#pragma clang fp contract(off)

namespace stvo {
namespace {

constexpr int ORB_HP = 15;  // half patch

struct OrbDev {
    int B, cols, rows, K, nfeatures, fast_th, edge_th;
    const int32_t* th;    // [n_th] or nullptr: FAST threshold of image i = th[i % n_th] (stvo_orb_set_fast_thresholds[_dev]); nullptr: fast_th
    int n_th;
    int cand_cap;         // rows * cols / 4 + 64: a 3x3 strict maximum every 2 x 2 pixels at most, so the list cannot overflow
    int32_t* n_total;     // [B] or nullptr: key-points that qualified before the cap K
    const uint8_t* img;   // [B][rows][cols]
    uint8_t* blur;        // [B][rows][cols]
    int32_t* hist;        // [B][256] responses of the key-points that survive NMS + border
    uint32_t* cand;       // [B][cand_cap] the survivors, unordered: (y << 20 | x << 8 | response)
    int32_t* n_cand;      // [B]
    int score_harris;     // orb_score 0: rank the 2 * nfeatures FAST-best key-points by Harris response, keep nfeatures of them
    uint32_t* hkey;       // [B][cand_cap] Harris responses as order-preserving words, parallel to cand (0: not among the 2 * nfeatures)
    float* kp;            // [B][K][2]
    float* resp;          // [B][K]
    float* angle;         // [B][K]
    uint8_t* desc;        // [B][K][32]
    int32_t* n_kp;        // [B]
    const int8_t* pattern;  // [256][4]
    // one image size per image (stvo_orb_set_image_sizes; read by the MIXED kernel instances only): image i is the top-left
    // cols x rows of row (i % n_sz) * sz_stride + level of the table, inside its slot of rows x cols above, whose pitch it keeps
    const OrbLevelSize* sz;
    int n_sz, sz_stride, level;
};

// The image a workgroup works on.  MIXED = false: the slot itself, the kernel argument.  MIXED = true: the image's row of the size table —
// blockIdx.z is uniform, so this is one scalar load per workgroup, as the threshold below — clamped into the slot, which the host has
// validated it to fit.  An image whose level is not active yields nothing, and a workgroup wholly outside its image has no work: both leave
// before their first barrier.
struct OrbGeom {
    int cols, rows;
    bool active;
};
template <bool MIXED>
__device__ __forceinline__ OrbGeom orb_geom(const OrbDev& o, int b) {
    if constexpr (MIXED) {
        const OrbLevelSize* e = o.sz + (size_t)(b % o.n_sz) * o.sz_stride + o.level;
        return OrbGeom{__builtin_amdgcn_readfirstlane(min(max(e->cols, 4), o.cols)), __builtin_amdgcn_readfirstlane(min(max(e->rows, 1), o.rows)),
                       __builtin_amdgcn_readfirstlane(e->active) != 0};
    } else {
        return OrbGeom{o.cols, o.rows, true};
    }
}

// circle offsets in OpenCV's order (dx, dy)
__device__ __constant__ int8_t c_circle[16][2] = {{0, 3},  {1, 3},   {2, 2},   {3, 1},   {3, 0},  {3, -1}, {2, -2}, {1, -3},
                                                  {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;  // a word at any byte address (gfx950 global memory allows it)
constexpr int FT_W = 64, FT_H = 64;               // output tile of the fused FAST + NMS kernel (a workgroup's life is a chain of
                                                  // memory round trips and barriers: 64 x 32 halves their share against 64 x 16)
constexpr int SC_W = FT_W + 2, SC_H = FT_H + 2;   // scores are needed one pixel beyond the tile (3x3 maximum test)
constexpr int IM_H = FT_H + 8;                    // image tile rows: + 1 (score halo) + 3 (circle radius) on both sides
constexpr int IM_DW = 19, IM_PITCH = 20;          // image tile row: 19 words = pixels x0 - 5 .. x0 + 70 (score position sx <-> byte sx + 4: word aligned)
constexpr int SC_PITCH = 72;                      // score row, bytes (18 words)

// cornerScore<16> of the pixel at byte (lx, ly) of the LDS image tile: max over the 16 arcs of 9 contiguous circle pixels of
// the smallest (signed) difference in the arc, bright and dark, minus 1 — min / max over every window of 9 by doubling
__device__ __forceinline__ int fast_score_lds(const uint8_t* tile, int lx, int ly) {
    const uint8_t* c = tile + ly * (IM_PITCH * 4) + lx;
    const int v = c[0];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = (int)c[c_circle[k][1] * (IM_PITCH * 4) + c_circle[k][0]] - v;
    int mn2[16], mx2[16], mn4[16], mx4[16], mn8[16], mx8[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn2[k] = min(d[k], d[(k + 1) & 15]);
        mx2[k] = max(d[k], d[(k + 1) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn4[k] = min(mn2[k], mn2[(k + 2) & 15]);
        mx4[k] = max(mx2[k], mx2[(k + 2) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn8[k] = min(mn4[k], mn4[(k + 4) & 15]);
        mx8[k] = max(mx4[k], mx4[(k + 4) & 15]);
    }
    int sb = -255, sd = -255;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        sb = max(sb, min(mn8[k], d[(k + 8) & 15]));
        sd = max(sd, -max(mx8[k], d[(k + 8) & 15]));
    }
    return max(sb, sd) - 1;
}

// One side of cornerScore<16> (round 6): with the differences taken as sgn (p - v) — sgn = +1 for the bright test, -1 for the dark one —
// both are "max over the 16 arcs of the smallest of the arc's 9 differences": half of fast_score_lds' work.  A pixel's score is the larger
// of its two sides minus 1; a side the signed compass test ruled out cannot reach t (a 9-arc holds two compass points), so only the
// sides that passed are evaluated (orb_fast_nms_kernel: one list entry per pixel and side).
__device__ __forceinline__ int fast_score_side_lds(const uint8_t* tile, int lx, int ly, int sgn) {
    const uint8_t* c = tile + ly * (IM_PITCH * 4) + lx;
    const int v = c[0];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = ((int)c[c_circle[k][1] * (IM_PITCH * 4) + c_circle[k][0]] - v) * sgn;
    int mn2[16], mn4[16], mn8[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) mn2[k] = min(d[k], d[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) mn4[k] = min(mn2[k], mn2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) mn8[k] = min(mn4[k], mn4[(k + 4) & 15]);
    int sb = -255;
#pragma unroll
    for (int k = 0; k < 16; ++k) sb = max(sb, min(mn8[k], d[(k + 8) & 15]));
    return sb - 1;
}

// wave-aggregated append of up to four flagged items per lane: ONE LDS atomic per wave (lanes hammering one counter serialise)
__device__ __forceinline__ void append4(const bool (&flag)[4], int* counter, int (&slot)[4]) {
    const int lane = threadIdx.x & 63;
    unsigned long long bal[4];
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bal[j] = __ballot(flag[j]);
        total += __popcll(bal[j]);
    }
    int base = 0;
    if (lane == 0 && total) base = atomicAdd(counter, total);
    base = __shfl(base, 0, 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        slot[j] = base + __popcll(bal[j] & ((1ull << lane) - 1ull));
        base += __popcll(bal[j]);
    }
}

// FAST-9/16 + non-maximum suppression + border filter of one 64 x 32 tile, entirely in LDS:
//   1. the image tile (+ halo) is staged once, word by word (unaligned global words; byte by byte only at the image border);
//   2. every score position (tile + halo 1) takes a cheap NECESSARY test, four positions per thread on words: an arc of 9
//      contiguous circle pixels holds at least two of the four compass points, so a corner has sum |compass - centre| >= 2 (t + 1).
//      The 4 x 4 bytes (north, south, east, west of four pixels; east / west by byte alignment) are transposed with v_perm_b32
//      and each pixel's sum is ONE v_sad_u8 — 8 instructions per pixel instead of the 26 of the signed compass test;
//   3. the survivors (~15 % of the positions) are COMPACTED into a list, so that the signed compass test (at least two compass
//      points brighter, or two darker, than the centre by more than t) and the 150-instruction corner score run on dense lanes;
//      the scores go to an LDS tile and the corners to a second list;
//   4. non-maximum suppression walks that corner list (~3 % of the positions), not the tile; a corner that beats its 8
//      neighbours and lies inside the border is appended to the image's candidate list and counted in the response histogram —
//      no score / keep maps ever reach global memory.
template <bool MIXED>
__global__ __launch_bounds__(256) void orb_fast_nms_kernel(OrbDev o) {
    __shared__ uint32_t tile[IM_H][IM_PITCH];
    __shared__ uint32_t sc_w[SC_H][SC_PITCH / 4];
    __shared__ uint16_t s_list[SC_H * SC_W + 8];
    __shared__ uint16_t s_corner[SC_H * SC_W + 8];
    __shared__ uint32_t s_kp[FT_W * FT_H / 4];  // key-points of this tile (a 3x3 maximum every 4 pixels at most)
    __shared__ int s_n, s_nc, s_nkp, s_base;
    const int b = blockIdx.z, x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H, tid = threadIdx.x, lane = tid & 63;
    const OrbGeom geo = orb_geom<MIXED>(o, b);
    const int cols = geo.cols, rows = geo.rows, pitch = o.cols;  // the image, and the row pitch of its slot
    if (MIXED && (!geo.active || x0 >= cols || y0 >= rows)) return;
    const uint8_t* img = o.img + (size_t)b * o.rows * o.cols;
    const uint8_t* tile8 = reinterpret_cast<const uint8_t*>(&tile[0][0]);
    uint8_t* sc = reinterpret_cast<uint8_t*>(&sc_w[0][0]);
    // one threshold per image: blockIdx.z is uniform, so this is one scalar load and one select per workgroup (the value stays in a
    // scalar register, as the kernel argument does).  The array is written by another kernel (stvo_fast_adapt_dev): what is read is
    // clamped to the range the scalar is validated to on the host
    const int t = o.th ? __builtin_amdgcn_readfirstlane(min(max(o.th[b % o.n_th], 1), 254)) : o.fast_th;
    {
        // every word of the tile is requested before the first is used (as a loop of load -> wait -> LDS store the workgroup began
        // its life with six memory round trips one after the other).  Words that cross the image border are re-read byte by byte
        // afterwards; the first pass reads them from a clamped address so that it needs no branch
        constexpr int ST_TRIPS = (IM_H * IM_DW + 255) / 256;
        uint32_t wv[ST_TRIPS];
#pragma unroll
        for (int k = 0; k < ST_TRIPS; ++k) {
            const int i = min(tid + 256 * k, IM_H * IM_DW - 1);
            const int ty = i / IM_DW, td = i - ty * IM_DW;
            const int gx = x0 - 5 + 4 * td, gy = min(max(y0 + ty - 4, 0), rows - 1);
            wv[k] = *reinterpret_cast<const u32_unaligned*>(img + (size_t)gy * pitch + min(max(gx, 0), cols - 4));
        }
#pragma unroll
        for (int k = 0; k < ST_TRIPS; ++k) {
            const int i = tid + 256 * k;
            if (i < IM_H * IM_DW) {
                const int ty = i / IM_DW, td = i - ty * IM_DW;
                const int gx = x0 - 5 + 4 * td, gy = min(max(y0 + ty - 4, 0), rows - 1);
                uint32_t w = wv[k];
                if (gx < 0 || gx + 4 > cols) {  // image border: replicate (those pixels never pass the border test below, their values only have to exist)
                    const uint8_t* row = img + (size_t)gy * pitch;
                    w = 0u;
#pragma unroll
                    for (int c = 0; c < 4; ++c) w |= (uint32_t)row[min(max(gx + c, 0), cols - 1)] << (8 * c);
                }
                tile[ty][td] = w;
            }
        }
    }
    for (int i = tid; i < SC_H * (SC_PITCH / 4); i += 256) (&sc_w[0][0])[i] = 0u;
    if (tid == 0) {
        s_n = 0;
        s_nc = 0;
        s_nkp = 0;
    }
    __syncthreads();
    // (all lanes of a wave run the same number of trips: the ballots of append4 need the whole wave)
    constexpr int GROUPS = (SC_W + 3) / 4;  // 17 groups of four score positions per row
    const uint32_t sad_min = 2u * (uint32_t)(t + 1);
    for (int i0 = 0; i0 < SC_H * GROUPS; i0 += 256) {
        const int i = i0 + tid;
        const bool item = i < SC_H * GROUPS;
        const int sy = item ? i / GROUPS : 0, g = item ? i - sy * GROUPS : 0;
        const int r = sy + 3, y = y0 + sy - 1;
        const uint32_t C = tile[r][g + 1], L = tile[r][g], R = tile[r][g + 2], N = tile[r - 3][g + 1], S = tile[r + 3][g + 1];
        const uint32_t W4 = __builtin_amdgcn_alignbyte(C, L, 1), E4 = __builtin_amdgcn_alignbyte(R, C, 3);
        // 4 x 4 byte transpose: Q[j] = (N, S, E, W) of pixel j
        const uint32_t ns01 = __builtin_amdgcn_perm(S, N, 0x05010400u), ns23 = __builtin_amdgcn_perm(S, N, 0x07030602u);
        const uint32_t ew01 = __builtin_amdgcn_perm(W4, E4, 0x05010400u), ew23 = __builtin_amdgcn_perm(W4, E4, 0x07030602u);
        uint32_t Q[4];
        Q[0] = __builtin_amdgcn_perm(ew01, ns01, 0x05040100u);
        Q[1] = __builtin_amdgcn_perm(ew01, ns01, 0x07060302u);
        Q[2] = __builtin_amdgcn_perm(ew23, ns23, 0x05040100u);
        Q[3] = __builtin_amdgcn_perm(ew23, ns23, 0x07060302u);
        const bool row_ok = item && y >= 3 && y < rows - 3;
        const int xb = x0 + 4 * g - 1;  // image column of pixel 0
        bool cand[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t V = __builtin_amdgcn_perm(C, C, 0x01010101u * (uint32_t)j);  // the centre in all four bytes
            const uint32_t sad = __builtin_amdgcn_sad_u8(Q[j], V, 0u);
            cand[j] = row_ok && 4 * g + j < SC_W && xb + j >= 3 && xb + j < cols - 3 && sad >= sad_min;
        }
        int slot[4];
        append4(cand, &s_n, slot);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cand[j]) s_list[slot[j]] = (uint16_t)(sy * SC_W + 4 * g + j);
    }
    __syncthreads();
    const int n = s_n;
    // 3a. the signed compass test on the dense list (circle points 0, 4, 8, 12 = south, east, north, west): at least two of them brighter, or two
    //     darker, than the centre by more than t — what passes (~40 % of the list) is compacted ONCE MORE, into s_corner, so that the ~200
    //     instructions of the corner score run on dense lanes too (round 6: a wave of the first list ran the score if any of its lanes passed)
    for (int j = tid; j < n; j += 256) {  // lanes of a wave carry consecutive j: lane 0 is active whenever any lane is
        const int i = s_list[j], sy = i / SC_W, sx = i - sy * SC_W;
        const uint8_t* c = tile8 + (sy + 3) * (IM_PITCH * 4) + (sx + 4);
        const int v = c[0];
        const int c0 = (int)c[3 * (IM_PITCH * 4)] - v, c4 = (int)c[3] - v, c8 = (int)c[-3 * (IM_PITCH * 4)] - v, c12 = (int)c[-3] - v;
        const int nb = (c0 > t) + (c4 > t) + (c8 > t) + (c12 > t), nd = (c0 < -t) + (c4 < -t) + (c8 < -t) + (c12 < -t);
        // one entry per pixel with the side(s) that passed: bit 15 = the dark side only, bit 14 = both (a saddle: rare)
        const bool pb = nb >= 2, pd = nd >= 2, pass = pb || pd;
        const unsigned long long bal = __ballot(pass);
        int base = 0;
        if (lane == 0 && bal) base = atomicAdd(&s_nc, __popcll(bal));
        base = __shfl(base, 0, 64);
        if (pass) s_corner[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)(i | (pb && pd ? 0x4000 : (pd ? 0x8000 : 0)));
    }
    __syncthreads();
    const int n_pass = s_nc;
    __syncthreads();  // (s_nc is counted anew below; s_list is free: the corners go there)
    if (tid == 0) {
        s_nc = 0;
        s_n = 0;
    }
    __syncthreads();
    // 3b. the score of the side that passed, on the dense list (both sides for the rare entries that ask for it: a uniform branch most
    //     waves skip); a pixel whose score reaches t is a corner: score tile + corner list (s_list)
    for (int j = tid; j < n_pass; j += 256) {
        const int e = s_corner[j], i = e & 0x3FFF, sy = i / SC_W, sx = i - sy * SC_W;
        int s = fast_score_side_lds(tile8, sx + 4, sy + 3, (e & 0x8000) ? -1 : 1);
        if (__any((e & 0x4000) != 0)) {
            const int s2 = fast_score_side_lds(tile8, sx + 4, sy + 3, -1);
            if (e & 0x4000) s = max(s, s2);
        }
        const bool corner = s >= t;  // t >= 1, so a corner's score is positive
        if (corner) sc[sy * SC_PITCH + sx] = (uint8_t)s;
        const unsigned long long bal = __ballot(corner);
        int base = 0;
        if (lane == 0 && bal) base = atomicAdd(&s_nc, __popcll(bal));
        base = __shfl(base, 0, 64);
        if (corner) s_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
    __syncthreads();
    const int nc = s_nc;
    for (int j = tid; j < nc; j += 256) {
        const int i = s_list[j], sy = i / SC_W, sx = i - sy * SC_W;
        const int x = x0 + sx - 1, y = y0 + sy - 1;
        bool kp = false;
        uint32_t s = 0u;
        if (sy >= 1 && sy <= FT_H && sx >= 1 && sx <= FT_W && x < cols && y < rows) {  // inside the tile proper (the halo only serves as neighbours)
            const uint8_t* q = sc + sy * SC_PITCH + sx;
            s = q[0];
            const uint32_t m8 = max(max(max((uint32_t)q[-SC_PITCH - 1], (uint32_t)q[-SC_PITCH]), max((uint32_t)q[-SC_PITCH + 1], (uint32_t)q[-1])),
                                    max(max((uint32_t)q[1], (uint32_t)q[SC_PITCH - 1]), max((uint32_t)q[SC_PITCH], (uint32_t)q[SC_PITCH + 1])));
            // 3x3 strict maximum, then KeyPointsFilter::runByImageBorder
            kp = s > m8 && x >= o.edge_th && x < cols - o.edge_th && y >= o.edge_th && y < rows - o.edge_th;
        }
        const unsigned long long bal = __ballot(kp);
        int base = 0;
        if (lane == 0 && bal) base = atomicAdd(&s_nkp, __popcll(bal));
        base = __shfl(base, 0, 64);
        if (kp) s_kp[base + __popcll(bal & ((1ull << lane) - 1ull))] = ((uint32_t)y << 20) | ((uint32_t)x << 8) | s;
    }
    __syncthreads();
    const int nkp = s_nkp;
    if (nkp == 0) return;
    if (tid == 0) s_base = atomicAdd(&o.n_cand[b], nkp);  // ONE global reservation per tile
    __syncthreads();
    for (int k = tid; k < nkp; k += 256) {
        const uint32_t c = s_kp[k];
        const int slot = s_base + k;
        if (slot < o.cand_cap) o.cand[(size_t)b * o.cand_cap + slot] = c;
        atomicAdd(&o.hist[(size_t)b * 256 + (c & 255u)], 1);
    }
}

// retainBest(nfeatures) as a histogram cut (the smallest response such that at least nfeatures key-points are >= it; ties at
// the cut are all kept) + ROW-MAJOR ordering of the survivors: one workgroup per image, bitonic sort of (y, x, response) words
// in LDS.  Writes key-points and responses, n_kp (capped at K), n_total, and resets the image's counters for the next frame.
// When more key-points qualify than the LDS holds (ORD_CAP; masses of equal responses at the cut), the FIRST K of the row-major
// order are selected exactly — histogram of the qualifying key-points over image rows, then over the columns of the boundary
// row — so the output never depends on the order in which tiles appended their candidates.
constexpr int ORD_CAP = 4096;
__device__ __forceinline__ void order_block_scan(int* bins /* [4096], in place -> inclusive prefix */, int* s_part /* [1024] */) {
    const int tid = threadIdx.x;
    int v0 = bins[4 * tid], v1 = bins[4 * tid + 1], v2 = bins[4 * tid + 2], v3 = bins[4 * tid + 3];
    v1 += v0; v2 += v1; v3 += v2;
    s_part[tid] = v3;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    const int base = tid ? s_part[tid - 1] : 0;
    bins[4 * tid] = base + v0; bins[4 * tid + 1] = base + v1; bins[4 * tid + 2] = base + v2; bins[4 * tid + 3] = base + v3;
    __syncthreads();
}
// the largest s in 1 .. 255 such that at least `need` entries of the 256-bin histogram lie in bins >= s (1 when there is none): the
// cut of retainBest on 8-bit keys.  Called by the whole workgroup (>= 256 threads); bins[] becomes its own suffix sums.
__device__ __forceinline__ void suffix_sums_256(int* bins) {
    const int tid = threadIdx.x;
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid + off < 256 ? bins[tid + off] : 0;
        __syncthreads();
        if (tid < 256) bins[tid] += add;
        __syncthreads();
    }
}

// A float as a word whose unsigned order is the float order (never 0 for a finite value), and back
__device__ __forceinline__ uint32_t float_to_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// HARRIS = false: the FAST_SCORE ranking described above.  HARRIS = true (orb_score 0): the candidates carry a second key, the Harris
// response of orb_harris_kernel as an order-preserving word (0 = not among the 2 n FAST-best).  retainBest(n) on it is the EXACT n-th
// largest key, found by an 8-bit radix select over the candidate list in global memory (four histogram passes; the list may hold
// any number of entries — 2 n plus the FAST ties — so it is never clamped before the cut), ties at the cut kept; the survivors are
// ordered and, beyond ORD_CAP, truncated to the first K of the row-major order exactly as in FAST mode.  `response` out is the float.
template <bool HARRIS>
__global__ __launch_bounds__(1024) void orb_order_kernel(OrbDev o) {
    __shared__ uint32_t s_key[ORD_CAP];
    __shared__ uint32_t s_val[HARRIS ? ORD_CAP : 1];  // the response words travel with the keys through the sort
    __shared__ int s_part[1024];
    __shared__ int s_cut, s_n, s_acc, s_ystar, s_xstar;
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t* hk = HARRIS ? o.hkey + (size_t)b * o.cand_cap : nullptr;
    uint32_t kcut = 1u;  // HARRIS: keep the candidates whose response word is >= kcut
    if constexpr (HARRIS) {
        const int nc0 = min(o.n_cand[b], o.cand_cap);
        uint32_t prefix = 0u, mask = 0u;
        int need = o.nfeatures, above = 0;  // the need-th largest among the keys that match the prefix; `above` keys are larger than all of those
        if (tid == 0) s_n = 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) s_part[tid] = 0;
            __syncthreads();
            for (int i = tid; i < nc0; i += 1024) {
                const uint32_t k = hk[i];
                if (k != 0u && (k & mask) == prefix) atomicAdd(&s_part[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            suffix_sums_256(s_part);
            if (pass == 0 && s_part[0] < need) {  // fewer ranked key-points than the budget: all of them stay (block-uniform)
                above = s_part[0];
                prefix = 1u;
                need = 0;
                break;
            }
            if (tid < 256) {
                const int ge = s_part[tid], gt = tid < 255 ? s_part[tid + 1] : 0;
                if (ge >= need && gt < need) {
                    s_cut = tid;
                    s_acc = gt;
                    s_ystar = ge - gt;
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_cut << shift;
            mask |= 255u << shift;
            above += s_acc;
            need -= s_acc;
            if (pass == 3) above += s_ystar;  // the keys equal to the cut: the ties
            __syncthreads();
        }
        kcut = prefix;
        __syncthreads();
        if (tid == 0) s_acc = above;
    } else if (tid == 0) {
        int cut = 1, acc = 0;
        for (int s = 255; s >= 1; --s) {
            acc += o.hist[(size_t)b * 256 + s];
            if (acc >= o.nfeatures) {
                cut = s;
                break;
            }
        }
        s_cut = cut;
        s_acc = acc;  // key-points with response >= cut (all of them when fewer than nfeatures exist: cut stays 1)
        s_n = 0;
    }
    __syncthreads();
    const int nc = min(o.n_cand[b], o.cand_cap), cut = s_cut, n_acc = s_acc;
    const uint32_t* cand = o.cand + (size_t)b * o.cand_cap;
    auto keep = [&](int i, uint32_t c) {
        if constexpr (HARRIS) return hk[i] >= kcut;
        else return (int)(c & 255u) >= cut;
    };
    uint32_t bound = 0xFFFFFFFFu;  // accept keys (y << 12 | x) <= bound
    if (n_acc > ORD_CAP) {  // block-uniform, rare: select the first K of the row-major order exactly
        const int want = min(o.K, ORD_CAP);
        int* bins = reinterpret_cast<int*>(s_key);
        for (int i = tid; i < ORD_CAP; i += 1024) bins[i] = 0;
        __syncthreads();
        for (int i = tid; i < nc; i += 1024) {
            const uint32_t c = cand[i];
            if (keep(i, c)) atomicAdd(&bins[c >> 20], 1);
        }
        __syncthreads();
        order_block_scan(bins, s_part);
        for (int i = tid; i < ORD_CAP; i += 1024)  // the row in which the cumulative count reaches `want`
            if (bins[i] >= want && (i == 0 || bins[i - 1] < want)) s_ystar = i;
        __syncthreads();
        const int ystar = s_ystar;
        const int before = ystar ? bins[ystar - 1] : 0;  // key-points in the rows above
        __syncthreads();
        for (int i = tid; i < ORD_CAP; i += 1024) bins[i] = 0;
        __syncthreads();
        for (int i = tid; i < nc; i += 1024) {
            const uint32_t c = cand[i];
            if (keep(i, c) && (int)(c >> 20) == ystar) atomicAdd(&bins[(c >> 8) & 0xFFFu], 1);
        }
        __syncthreads();
        order_block_scan(bins, s_part);
        const int need = want - before;  // >= 1 key-points of the boundary row, lowest columns first
        for (int i = tid; i < ORD_CAP; i += 1024)
            if (bins[i] >= need && (i == 0 || bins[i - 1] < need)) s_xstar = i;
        __syncthreads();
        bound = ((uint32_t)ystar << 12) | (uint32_t)s_xstar;
        __syncthreads();
    }
    for (int i = tid; i < ORD_CAP; i += 1024) s_key[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < nc; i += 1024) {
        const uint32_t c = cand[i];
        if (keep(i, c) && (c >> 8) <= bound) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < ORD_CAP) {
                s_key[slot] = c;
                if constexpr (HARRIS) s_val[slot] = hk[i];
            }
        }
    }
    __syncthreads();
    const int n = min(s_n, ORD_CAP);
    int np2 = 64;
    while (np2 < n) np2 <<= 1;
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = s_key[i], c = s_key[l];
                    const bool up = (i & k) == 0;
                    if ((a > c) == up) {
                        s_key[i] = c;
                        s_key[l] = a;
                        if constexpr (HARRIS) {
                            const uint32_t va = s_val[i];
                            s_val[i] = s_val[l];
                            s_val[l] = va;
                        }
                    }
                }
            }
            __syncthreads();
        }
    const int n_out = min(n, o.K);
    for (int i = tid; i < n_out; i += 1024) {
        const uint32_t c = s_key[i];
        const size_t k = (size_t)b * o.K + i;
        o.kp[2 * k] = (float)((c >> 8) & 0xFFFu);
        o.kp[2 * k + 1] = (float)(c >> 20);
        if constexpr (HARRIS) o.resp[k] = key_to_float(s_val[i]);
        else o.resp[k] = (float)(c & 255u);
    }
    __syncthreads();
    if (tid < 256) o.hist[(size_t)b * 256 + tid] = 0;  // ready for the next frame
    if (tid == 0) {
        o.n_kp[b] = n_out;
        if (o.n_total) o.n_total[b] = n_acc;
        o.n_cand[b] = 0;
    }
}

// HarrisResponses (features2d/src/orb.cpp; blockSize 7, harris_k 0.04) of the key-points that survive retainBest(2 n) by FAST score —
// the same histogram cut as orb_order_kernel's, with twice the budget, ties kept — on the LEVEL image.  8 lanes per key-point (8
// key-points per wave, 32 per workgroup): the 9 x 9 byte patch around the key-point is staged in LDS once, as 9 rows of 3 unaligned
// words = 27 words, four loads per lane all in flight together; lane j < 7 then owns row j of the 7 x 7 block (lane 7 only loads):
// it reads the three patch rows j .. j + 2 as 9 words, forms per column the vertical smoothing r0 + 2 r1 + r2 and difference r2 - r0
// once (the Sobel sums of the row's 7 positions share them: Ix = H[c + 1] - H[c - 1], Iy = V[c - 1] + 2 V[c] + V[c + 1], all exact in
// integers), and three shuffle steps add the a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy of the rows.  One lane per key-point would leave 7 of
// 8 lanes of the few thousand key-points' waves idle through 27 dependent loads; 64 lanes would spend their time in the reduction.
// The response is formed in FP32 operation by operation as OpenCV writes it (no contraction: see the pragma above) and stored as an
// order-preserving word beside the candidate (0 for the candidates below the FAST cut).
constexpr int HR_LANES = 8, HR_KP_PER_WG = 256 / HR_LANES, HR_BLOCKS = 32;  // a grid-stride loop of HR_BLOCKS workgroups per image
constexpr int HR_PW = 3;                                                    // patch: 9 rows of 3 words = bytes x - 4 .. x + 7
__global__ __launch_bounds__(256) void orb_harris_kernel(OrbDev o) {
    __shared__ uint32_t s_patch[HR_KP_PER_WG][HR_LANES * 4];  // 27 words used; every lane stores every word it loaded
    __shared__ int s_bins[256];
    __shared__ int s_cut;
    const int b = blockIdx.y, tid = threadIdx.x, g = tid / HR_LANES, l = tid % HR_LANES;
    const int nc = min(o.n_cand[b], o.cand_cap);
    if (nc == 0) return;
    s_bins[tid] = tid ? o.hist[(size_t)b * 256 + tid] : 0;
    if (tid == 0) s_cut = 1;
    __syncthreads();
    suffix_sums_256(s_bins);
    {
        const int need = 2 * min(o.nfeatures, 1 << 29);
        if (tid >= 1 && s_bins[tid] >= need && (tid == 255 || s_bins[tid + 1] < need)) s_cut = tid;
    }
    __syncthreads();
    const int cut = s_cut;
    const uint32_t* cand = o.cand + (size_t)b * o.cand_cap;
    uint32_t* hkey = o.hkey + (size_t)b * o.cand_cap;
    const uint8_t* img = o.img + (size_t)b * o.rows * o.cols;
    const int off_hi = o.rows * o.cols - 4;
    uint32_t* patch = s_patch[g];
    for (int base = blockIdx.x * HR_KP_PER_WG; base < nc; base += gridDim.x * HR_KP_PER_WG) {  // (block-uniform trip count)
        const int i = base + g;
        const bool valid = i < nc;
        const uint32_t c = cand[valid ? i : nc - 1];
        const bool ranked = valid && (int)(c & 255u) >= cut;
        if (!__any(ranked)) {  // wave-uniform
            if (valid && l == 0) hkey[i] = 0u;
            continue;
        }
        const int x = (int)((c >> 8) & 0xFFFu), y = (int)(c >> 20);
        // the patch lies inside the image (edge threshold >= 19); the words beyond the 27 are clamped into the buffer and never read
        const int org = (y - 4) * o.cols + (x - 4);
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = l + HR_LANES * j, r = k / HR_PW, q = k - r * HR_PW;
            w[j] = *reinterpret_cast<const u32_unaligned*>(img + min(max(org + r * o.cols + 4 * q, 0), off_hi));
        }
        // (the previous round's reads of this patch are complete: its shuffles below synchronise the group)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[l + HR_LANES * j] = w[j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int a = 0, bb = 0, cc = 0;
        {
            const uint32_t* rw = patch + (l < 7 ? l : 0) * HR_PW;
            uint32_t R[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) R[r][q] = rw[r * HR_PW + q];
            int H[9], V[9];
#pragma unroll
            for (int n = 0; n < 9; ++n) {
                const int p0 = (int)((R[0][n >> 2] >> (8 * (n & 3))) & 255u), p1 = (int)((R[1][n >> 2] >> (8 * (n & 3))) & 255u),
                          p2 = (int)((R[2][n >> 2] >> (8 * (n & 3))) & 255u);
                H[n] = p0 + 2 * p1 + p2;
                V[n] = p2 - p0;
            }
#pragma unroll
            for (int n = 1; n < 8; ++n) {  // block column n - 1 = patch column n
                const int ix = H[n + 1] - H[n - 1], iy = V[n - 1] + 2 * V[n] + V[n + 1];
                a += ix * ix;
                bb += iy * iy;
                cc += ix * iy;
            }
            if (l == 7) a = bb = cc = 0;
        }
#pragma unroll
        for (int off = HR_LANES / 2; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            bb += __shfl_xor(bb, off, 64);
            cc += __shfl_xor(cc, off, 64);
        }
        constexpr float scale = 1.f / (4 * 7 * 255.f), scale4 = scale * scale * scale * scale, harris_k = 0.04f;
        const float fa = (float)a, fb = (float)bb, fc = (float)cc;
        const float resp = (fa * fb - fc * fc - harris_k * (fa + fb) * (fa + fb)) * scale4 + 0.f;  // (+ 0: one zero, the positive one)
        if (valid && l == 0) hkey[i] = ranked ? float_to_key(resp) : 0u;
    }
}

// Level l of the pyramid from level l - 1: OpenCV's resize(src, dst, dsize, 0, 0, INTER_LINEAR) for 8-bit images — source
// position (d + 0.5) scale - 0.5 in double -> float, weights cvRound((1 - f) 2048) / cvRound(f 2048) as shorts, horizontal pass
// in integers, rows combined as (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2 (oracle/stvo_orb_oracle.c:
// orc_resize_linear).  One thread per output pixel; the coefficient arithmetic is a few FP ops next to four byte loads.
struct ResizeArgs {
    int B, scols, srows, dcols, drows;
    double scale_x, scale_y;  // 1 / inv_scale as OpenCV forms them: inv_scale = dsize / ssize for a given dsize, = fx, fy for Size()
    const uint8_t* src;
    uint8_t* dst;
    // MIXED only: the sizes above are the slots' (and the pitches of both buffers); image b is resized from row `level - 1` to row
    // `level` of its entry of the size table, with that row's inverse scales
    const OrbLevelSize* sz;
    int n_sz, sz_stride, level;
};
template <bool MIXED>
__global__ __launch_bounds__(256) void orb_resize_kernel(ResizeArgs r) {
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
    int scols = r.scols, srows = r.srows, dcols = r.dcols;
    double scale_x = r.scale_x, scale_y = r.scale_y;
    if constexpr (MIXED) {  // (uniform over the workgroup: scalar loads)
        const OrbLevelSize* e = r.sz + (size_t)(b % r.n_sz) * r.sz_stride + r.level;
        scols = min(max(e[-1].cols, 1), r.scols);
        srows = min(max(e[-1].rows, 1), r.srows);
        dcols = min(e->cols, r.dcols);
        scale_x = e->inv_sx;
        scale_y = e->inv_sy;
        if (dy >= e->rows) return;
    }
    if (dx >= dcols) return;
    float fx = (float)(((double)dx + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) {
        fx = 0.f;
        sx = 0;
    }
    if (sx >= scols - 1) {
        fx = 0.f;
        sx = scols - 1;
    }
    const int a0 = (short)__float2int_rn((1.f - fx) * 2048.f), a1 = (short)__float2int_rn(fx * 2048.f);
    float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int b0 = (short)__float2int_rn((1.f - fy) * 2048.f), b1 = (short)__float2int_rn(fy * 2048.f);
    const uint8_t* img = r.src + (size_t)b * r.srows * r.scols;
    const int y0 = min(max(sy, 0), srows - 1), y1 = min(max(sy + 1, 0), srows - 1);
    const uint8_t* r0 = img + (size_t)y0 * r.scols;
    const uint8_t* r1 = img + (size_t)y1 * r.scols;
    int S0, S1;
    if (sx < scols - 1) {
        S0 = (int)r0[sx] * a0 + (int)r0[sx + 1] * a1;
        S1 = (int)r1[sx] * a0 + (int)r1[sx + 1] * a1;
    } else {
        S0 = (int)r0[sx] * 2048;
        S1 = (int)r1[sx] * 2048;
    }
    const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    r.dst[((size_t)b * r.drows + dy) * r.dcols + dx] = (uint8_t)min(max(v, 0), 255);
}

// Key-points of all levels in level order (ORB_Impl::computeKeyPoints appends level after level): coordinates multiplied by the
// level's scale in float (pt *= scale), octave = level; one workgroup per image, capped at K.
struct ConcatArgs {
    int B, K, nlevels, Kl;  // Kl: stride of the per-level arrays
    float scale[STVO_ORB_MAX_LEVELS];
    const float* kp[STVO_ORB_MAX_LEVELS];
    const float* resp[STVO_ORB_MAX_LEVELS];
    const float* ang[STVO_ORB_MAX_LEVELS];
    const uint8_t* desc[STVO_ORB_MAX_LEVELS];
    const int32_t* n[STVO_ORB_MAX_LEVELS];
    const int32_t* n_tot[STVO_ORB_MAX_LEVELS];
    float* kp_o;
    float* resp_o;
    float* ang_o;
    int32_t* oct_o;  // may be nullptr
    uint8_t* desc_o;
    int32_t* n_o;
    int32_t* n_total_o;  // may be nullptr
};
__global__ __launch_bounds__(256) void orb_concat_kernel(ConcatArgs c) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int off = 0, total = 0;
    for (int l = 0; l < c.nlevels; ++l) {
        const int nl = c.n[l][b];
        total += c.n_tot[l][b];
        const float sc = c.scale[l];
        for (int i = tid; i < nl && off + i < c.K; i += 256) {
            const size_t s = (size_t)b * c.Kl + i, d = (size_t)b * c.K + off + i;
            const float x = c.kp[l][2 * s], y = c.kp[l][2 * s + 1];
            c.kp_o[2 * d] = l ? x * sc : x;
            c.kp_o[2 * d + 1] = l ? y * sc : y;
            c.resp_o[d] = c.resp[l][s];
            c.ang_o[d] = c.ang[l][s];
            if (c.oct_o) c.oct_o[d] = l;
            const uint4* src = reinterpret_cast<const uint4*>(c.desc[l] + s * 32);
            uint4* dst = reinterpret_cast<uint4*>(c.desc_o + d * 32);
            dst[0] = src[0];
            dst[1] = src[1];
        }
        off += nl;
    }
    if (tid == 0) {
        c.n_o[b] = min(off, c.K);
        if (c.n_total_o) c.n_total_o[b] = total;
    }
}

__device__ __forceinline__ int reflect101(int p, int n) {
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        if (p >= n) p = 2 * n - 2 - p;
    }
    return p;
}

struct BlurK {
    int k[7];
};

// Separable 7 x 7 blur in registers, no LDS: a thread produces 4 adjacent pixels (one packed word) of BL_R consecutive rows.
// Per input row it loads the 12 bytes x - 4 .. x + 7 as three (unaligned) words, forms the four horizontal sums with byte
// alignment + 4-way byte dot products (v_alignbyte_b32 / v_dot4_u32_u8: 16 instructions instead of 12 extractions + 28
// multiply-adds), keeps the last seven rows of sums in a register ring and emits one output row per input row.  The arithmetic
// is the integer one of the tile version (weights * 2^8 per pass, (s + 2^15) >> 16), so the sums may be taken in any order.
constexpr int BL_R = 16, BL_T = 64;

template <bool MIXED>
__global__ __launch_bounds__(BL_T) void orb_blur_kernel(OrbDev o, BlurK kk) {
    const int b = blockIdx.z, x = (blockIdx.x * BL_T + threadIdx.x) * 4, y0 = blockIdx.y * BL_R;
    const OrbGeom geo = orb_geom<MIXED>(o, b);
    const int cols = geo.cols, rows = geo.rows, pitch = o.cols;  // BORDER_REFLECT_101 at the image's own border; the row pitch of its slot
    if (MIXED && (!geo.active || y0 >= rows)) return;
    if (x >= cols) return;
    const uint8_t* img = o.img + (size_t)b * o.rows * o.cols;
    uint8_t* out = o.blur + (size_t)b * o.rows * o.cols;
    const uint32_t k03 = (uint32_t)kk.k[0] | ((uint32_t)kk.k[1] << 8) | ((uint32_t)kk.k[2] << 16) | ((uint32_t)kk.k[3] << 24);
    const uint32_t k46 = (uint32_t)kk.k[4] | ((uint32_t)kk.k[5] << 8) | ((uint32_t)kk.k[6] << 16);
    // The three words of a row — bytes x - 4 .. x - 1, x .. x + 3, x + 4 .. x + 7 under BORDER_REFLECT_101 — as ONE word load + ONE v_perm each,
    // for every thread alike: four consecutive positions reflect into a window of at most four bytes, so each word is a word of the row (at
    // a per-thread offset) with its bytes permuted (a per-thread selector; the identity away from the border).  Offsets and selectors are
    // computed once, not per row.  (Round 6: the border threads used to take a byte-by-byte path — 12 byte loads and 12 reflections per
    // row, inlined 22 times — and dragged their whole wave through it: two of the five waves of an image row.)
    int woff[3];
    uint32_t wsel[3];
#pragma unroll
    for (int wi = 0; wi < 3; ++wi) {
        int q[4], lo = 0x7FFFFFFF;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q[i] = reflect101(x - 4 + 4 * wi + i, cols);
            lo = min(lo, q[i]);
        }
        lo = max(min(lo, cols - 4), 0);
        woff[wi] = lo;
        wsel[wi] = (uint32_t)(q[0] - lo) | ((uint32_t)(q[1] - lo) << 8) | ((uint32_t)(q[2] - lo) << 16) | ((uint32_t)(q[3] - lo) << 24);
    }
    uint32_t h[7][4];
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) h[j][i] = 0u;
#pragma unroll
    for (int r = 0; r < BL_R + 6; ++r) {
        const int yo = y0 + r - 6;                  // output row completed by this input row
        if (r >= 6 && yo >= rows) break;            // uniform over the workgroup
        const int gy = reflect101(y0 + r - 3, rows);
        const uint8_t* row = img + (size_t)gy * pitch;
        const uint32_t w0 = __builtin_amdgcn_perm(0u, *reinterpret_cast<const u32_unaligned*>(row + woff[0]), wsel[0]);
        const uint32_t w1 = __builtin_amdgcn_perm(0u, *reinterpret_cast<const u32_unaligned*>(row + woff[1]), wsel[1]);
        const uint32_t w2 = __builtin_amdgcn_perm(0u, *reinterpret_cast<const u32_unaligned*>(row + woff[2]), wsel[2]);
        // output i: taps x + i - 3 .. x + i + 3 = bytes i + 1 .. i + 7 of (w0, w1, w2)
        uint32_t hs[4];
        hs[0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 1), k03, 0u, false);
        hs[0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 1), k46, hs[0], false);
        hs[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 2), k03, 0u, false);
        hs[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 2), k46, hs[1], false);
        hs[2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 3), k03, 0u, false);
        hs[2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 3), k46, hs[2], false);
        hs[3] = __builtin_amdgcn_udot4(w1, k03, 0u, false);
        hs[3] = __builtin_amdgcn_udot4(w2, k46, hs[3], false);
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) h[j][i] = h[j + 1][i];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[6][i] = hs[i];
        if (r >= 6) {
            uint32_t px = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t sv = 1u << 15;
#pragma unroll
                for (int j = 0; j < 7; ++j) sv += __umul24((uint32_t)kk.k[j], h[j][i]);  // (weights <= 2^8, row sums <= 2^16: the 24-bit multiply-add is exact and full rate)
                px |= min(sv >> 16, 255u) << (8 * i);
            }
            uint8_t* dst = out + (size_t)yo * pitch + x;
            if (x + 4 <= cols) {
                *reinterpret_cast<u32_unaligned*>(dst) = px;
            } else {
                for (int i = 0; x + i < cols; ++i) dst[i] = (uint8_t)(px >> (8 * i));
            }
        }
    }
}

struct Umax {
    int u[ORB_HP + 2];
};

// 16 lanes per key-point (4 key-points per wave, 16 per workgroup): intensity-centroid angle on the image, rotated BRIEF on the
// blurred image.  Both patches are first copied into LDS with word loads (a row of a patch is 32 / 40 contiguous bytes, one
// cache line per key-point and load instruction); the 512 rotated test points of a key-point are then gathered from LDS.
// Gathered from global memory, every test load of a wave touched up to 64 different cache lines — the texture-address path,
// not arithmetic, set the pace of the first two versions (675 / 450 us per 512 k key-points).  The sine / cosine of the angle
// (double precision, like the oracle's libm call) runs once per wave: four key-points share it.
constexpr int DESC_KP_PER_WG = 16;
constexpr int DESC_R = 19;                        // |rotated pattern coordinate| <= 13 sqrt 2 < 19
constexpr int DESC_PW = 10, DESC_PH = 2 * DESC_R + 1;  // blurred patch: 39 rows of 10 words = bytes x - 20 .. x + 19
constexpr int IC_PW = 8, IC_PH = 2 * ORB_HP + 1;       // image patch: 31 rows of 8 words = bytes x - 16 .. x + 15
__global__ __launch_bounds__(256) void orb_describe_kernel(OrbDev o, Umax um) {
    constexpr int PATCH_W = ((DESC_PH * DESC_PW + 15) / 16) * 16;  // rounded up to the 16 lanes of a group: every lane stores every word it loaded
    __shared__ uint32_t s_patch[DESC_KP_PER_WG][PATCH_W];  // the image patch first (31 x 8 words), then the blurred one
    // XCD-aware 1-D grid: workgroup L runs on XCD L mod 8 (round-robin dispatch), so image = 8 (L / 8 / blocks per image) + L mod 8
    // keeps every workgroup of an image on ONE XCD — the patches of neighbouring key-points overlap (2000 key-points read 11 x the
    // image), and with the image's workgroups dealt over all eight private L2s each of them fetched the image from HBM again
    // (FETCH_SIZE 6.6 x the image bytes in round 3)
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
    const int bpi = (o.K + DESC_KP_PER_WG - 1) / DESC_KP_PER_WG;  // workgroups per image
    const int b = (kq / bpi) * 8 + xcd, kb = kq % bpi;
    if (b >= o.B) return;
    const int lane = threadIdx.x & 63, l = lane & 15;
    // the circular patch as byte masks of the row words: row |dy| keeps columns |u| <= umax[|dy|] (byte k of word w is column 4 w + k - 16)
    __shared__ uint32_t s_mask[ORB_HP + 1][IC_PW];
    if (threadIdx.x < (ORB_HP + 1) * IC_PW) {
        const int v = threadIdx.x >> 3, w = threadIdx.x & 7;
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int u = 4 * w + k - 16;
            if ((u < 0 ? -u : u) <= um.u[v]) m |= 0xFFu << (8 * k);
        }
        s_mask[v][w] = m;
    }
    __syncthreads();
    const int n = o.n_kp[b];
    const int k_first = kb * DESC_KP_PER_WG + (threadIdx.x >> 6) * 4;
    if (k_first >= n) return;  // wave-uniform
    const int slot = (threadIdx.x >> 6) * 4 + (lane >> 4);
    const int k_own = k_first + (lane >> 4);
    const bool valid = k_own < n;
    const int k = valid ? k_own : n - 1;  // idle groups shadow the last key-point (the shuffles below want every lane)
    const size_t kk = (size_t)b * o.K + k;
    const int x = (int)o.kp[2 * kk], y = (int)o.kp[2 * kk + 1];
    const size_t base = (size_t)b * o.rows * o.cols;
    uint32_t* patch = s_patch[slot];
    const uint8_t* patch8 = reinterpret_cast<const uint8_t*>(patch);
    // the patches lie inside the image (edge threshold >= 19 + 1 word of slack is NOT guaranteed on the left / right: clamp the
    // word address into the image buffer; the clamped words hold columns the disc / the pattern never reads)
    // (round 6: 32-bit offsets into the image, clamped with one v_med3 — the clamped POINTERS cost two 64-bit compares and four selects per word,
    //  a quarter of the kernel's vector instructions)
    const uint8_t* img_b = o.img + base;
    const int off_hi = o.rows * o.cols - 4;
    {
        // all 16 words of a lane's share are requested before the first is stored (as a loop the compiler made four groups of four
        // loads with a wait after each: four memory round trips one after the other at the start of every wave)
        constexpr int IW_N = (IC_PH * IC_PW + 15) / 16;
        uint32_t iw[IW_N];
        const int org = (y - ORB_HP) * o.cols + (x - 16);
#pragma unroll
        for (int j = 0; j < IW_N; ++j) {
            const int i = l + 16 * j;
            const int r = i >> 3, w = i & 7;
            const int off = min(max(org + (int)__umul24((unsigned)r, (unsigned)o.cols) + 4 * w, 0), off_hi);  // (i beyond the patch: a clamped, unused word)
            iw[j] = *reinterpret_cast<const u32_unaligned*>(img_b + off);
        }
#pragma unroll
        for (int j = 0; j < IW_N; ++j) patch[l + 16 * j] = iw[j];  // (unconditional: a store under `i < 248` took its load along, into a round trip of its own)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the blurred patch is requested NOW, into registers (25 words per lane), and stored to LDS behind the moments: its memory round
    // trip runs beside the computation instead of after it
    constexpr int BW_N = (DESC_PH * DESC_PW + 15) / 16;
    uint32_t bw[BW_N];
    {
        const uint8_t* blur_b = o.blur + base;
        const int org = (y - DESC_R) * o.cols + (x - 20);
#pragma unroll
        for (int j = 0; j < BW_N; ++j) {
            const int i = l + 16 * j;
            const int r = i / DESC_PW, w = i - r * DESC_PW;
            const int off = min(max(org + (int)__umul24((unsigned)r, (unsigned)o.cols) + 4 * w, 0), off_hi);  // (i beyond the patch: a clamped, unused word)
            bw[j] = *reinterpret_cast<const u32_unaligned*>(blur_b + off);
        }
    }
    // ICAngles: lane l owns ROWS l and l + 16 of the patch (dy = row - 15).  Integer moments, so the summation order is free: a row is 8
    // words — masked to the disc, then m10 += sum u I and the row sum for m01 come from byte dot products (v_dot4_u32_u8: weights u + 16
    // and 1) instead of 31 byte loads per column (~70 instead of ~300 instructions per lane)
    int m10 = 0, m01 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = l + 16 * h;
        const bool row_ok = r < IC_PH;
        const int dy = r - ORB_HP, ady = dy < 0 ? -dy : dy;
        const uint32_t* row = patch + (row_ok ? r : 0) * IC_PW;
        const uint32_t* msk = s_mask[row_ok ? ady : 0];
        uint32_t s1 = 0u, su = 0u;
#pragma unroll
        for (int w = 0; w < IC_PW; ++w) {
            const uint32_t W = row[w] & msk[w];
            s1 = __builtin_amdgcn_udot4(W, 0x01010101u, s1, false);
            su = __builtin_amdgcn_udot4(W, 0x03020100u + 0x04040404u * (uint32_t)w, su, false);
        }
        if (row_ok) {
            m10 += (int)su - 16 * (int)s1;
            m01 += dy * (int)s1;
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off, 64);
        m01 += __shfl_xor(m01, off, 64);
    }
    const float ang = fast_atan2_deg((float)m01, (float)m10);
    if (valid && l == 0) o.angle[kk] = ang;
    // the blurred patch replaces the image patch (every lane of the group is past its reads: the shuffles above synchronise)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < BW_N; ++j) patch[l + 16 * j] = bw[j];  // (unconditional: the row is padded to 16 x BW_N words)
    // computeOrbDescriptors, WTA_K = 2: lane l evaluates tests 16 l .. 16 l + 15 = bytes 2 l, 2 l + 1 of the descriptor
    // (float)cos, (float)sin of the float radians in double precision, like the oracle's library calls (orb_rotate.h: the same floats, which
    // tests/cpp/orb_rotate_host_main.cpp holds for every float angle in [0, 360])
    float a, sb;
    orb_rotation(ang, a, sb);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint8_t* bl = patch8 + DESC_R * (DESC_PW * 4) + 20;  // the key-point's own pixel
    const int* pat = reinterpret_cast<const int*>(o.pattern) + 16 * l;  // (x0, y0, x1, y1) of a test as one word
    uint32_t bits = 0u;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int w = pat[t];
        const float px0 = (float)(int8_t)(w & 0xFF), py0 = (float)(int8_t)((w >> 8) & 0xFF);
        const float px1 = (float)(int8_t)((w >> 16) & 0xFF), py1 = (float)(int8_t)((w >> 24) & 0xFF);
        const int ix0 = ORB_ROTATE_X(px0, py0, a, sb), iy0 = ORB_ROTATE_Y(px0, py0, a, sb);
        const int ix1 = ORB_ROTATE_X(px1, py1, a, sb), iy1 = ORB_ROTATE_Y(px1, py1, a, sb);
        const int t0 = bl[iy0 * (DESC_PW * 4) + ix0], t1 = bl[iy1 * (DESC_PW * 4) + ix1];
        bits |= (uint32_t)(t0 < t1) << t;
    }
    if (valid) *reinterpret_cast<uint16_t*>(o.desc + kk * 32 + 2 * l) = (uint16_t)bits;
}

// Every descriptor setting other than (WTA_K 2, patch 31) — stvo_orb_set_descriptor — in place of orb_describe_kernel: ICAngles on the
// disc of half patch h = P / 2, then the tests of the EFFECTIVE pattern (csrc/orb_pattern.h) on the blurred image, WTA_K 2 as above,
// WTA_K 3 / 4 as the index of the largest of a tuple's 3 / 4 values in a 2-bit field (four tuples per byte).  ONE WAVE per key-point, four
// key-points per workgroup, no workgroup barrier: a patch of up to 63 rows gives a row to every lane, 256 tests / 128 tuples give every
// lane four bits of the descriptor, and at the largest patch (P = 63: 89 x 89 blurred bytes, reach 44) a workgroup holds 4 x 8188 bytes
// of LDS — five workgroups fit the 160 KB of a CU.  RMAX is the largest reach an instance holds: 22 serves P <= 31 (2160 bytes per
// key-point), 44 the rest.  The image patch (2 h + 1 rows) and the blurred patch (2 R + 1 rows, R = the reach of the setting) share the
// buffer one after the other; rows are staged as unaligned words from the patch's first column on, so a word holds needed bytes from
// its first byte and only the row's last word can look beyond the image buffer: it is read from the last word of the buffer and shifted.
// Moments: a row's bytes are masked to the disc and summed with byte dot products into 32-bit sums (|m10| reaches 5.1e6 at h = 31).
struct WtaArgs {
    int h;                  // half patch
    int R;                  // reach of the rotated pattern points: rows / columns y - R .. y + R of the blurred image are staged
    const int8_t* pattern;  // the effective point list: 512 / 384 / 512 (x, y) pairs
    const int8_t* umax;     // [h + 1]
};
constexpr int WTA_KP_PER_WG = 4;
template <int WTA, int RMAX>
__global__ __launch_bounds__(256) void orb_describe_wta_kernel(OrbDev o, WtaArgs wa) {
    constexpr int PW = (2 * RMAX + 1 + 3) / 4, PH = 2 * RMAX + 1;  // words per row, rows
    __shared__ uint32_t s_patch[WTA_KP_PER_WG][PH * PW];
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;  // (the XCD-aware grid of orb_describe_kernel)
    const int bpi = (o.K + WTA_KP_PER_WG - 1) / WTA_KP_PER_WG;
    const int b = (kq / bpi) * 8 + xcd, kb = kq % bpi;
    if (b >= o.B) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = kb * WTA_KP_PER_WG + wave;
    if (k >= o.n_kp[b]) return;  // wave-uniform; the kernel has no workgroup barrier
    const int h = min(wa.h, RMAX), R = min(max(wa.R, h), RMAX);  // (validated on the host; the buffer is never left whatever arrives)
    const size_t kk = (size_t)b * o.K + k;
    const int x = (int)o.kp[2 * kk], y = (int)o.kp[2 * kk + 1];
    const size_t base = (size_t)b * o.rows * o.cols;
    const int off_hi = o.rows * o.cols - 4;
    uint32_t* patch = s_patch[wave];
    // rows y - r .. y + r, bytes x - r .. of `src` into the buffer: row i at word i * PW
    auto stage = [&](const uint8_t* src, int r) {
        const int nw = (2 * r + 1 + 3) / 4, n = (2 * r + 1) * nw;
        const int org = (y - r) * o.cols + (x - r);
        for (int i = lane; i < n; i += 64) {
            const int row = i / nw, w = i - row * nw;
            const int off = max(org + row * o.cols + 4 * w, 0);
            const int over = min(max(off - off_hi, 0), 3);  // bytes by which the word would leave the buffer (the row's last word on the last rows)
            patch[row * PW + w] = *reinterpret_cast<const u32_unaligned*>(src + min(off, off_hi)) >> (8 * over);
        }
    };
    stage(o.img + base, h);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ICAngles: lane r owns row r of the patch (dy = r - h); byte j of the row is column u = j - h
    int m10 = 0, m01 = 0;
    if (lane <= 2 * h) {
        const int dy = lane - h, um = wa.umax[dy < 0 ? -dy : dy];
        const uint32_t* row = patch + lane * PW;
        const int nw = (2 * h + 1 + 3) / 4;
        uint32_t s1 = 0u, su = 0u;
        for (int w = 0; w < nw; ++w) {
            uint32_t m = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = 4 * w + j - h;
                if ((u < 0 ? -u : u) <= um) m |= 0xFFu << (8 * j);
            }
            const uint32_t W = row[w] & m;
            s1 = __builtin_amdgcn_udot4(W, 0x01010101u, s1, false);
            su = __builtin_amdgcn_udot4(W, 0x03020100u + 0x04040404u * (uint32_t)w, su, false);  // weights u + h <= 63
        }
        m10 = (int)su - h * (int)s1;
        m01 = dy * (int)s1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off, 64);
        m01 += __shfl_xor(m01, off, 64);
    }
    const float ang = fast_atan2_deg((float)m01, (float)m10);
    if (lane == 0) o.angle[kk] = ang;
    float a, sb;
    orb_rotation(ang, a, sb);
    // the blurred patch replaces the image patch (every lane is past its reads: the shuffles above synchronise the wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stage(o.blur + base, R);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint8_t* bl = reinterpret_cast<const uint8_t*>(patch) + R * (PW * 4) + R;  // the key-point's own pixel
    // lane l: tests 4 l .. 4 l + 3 (WTA_K 2) or tuples 2 l, 2 l + 1 (WTA_K 3 / 4) = bits 4 l .. 4 l + 3 of the descriptor
    constexpr int NPT = WTA == 3 ? 6 : 8;  // points per lane: 12 / 16 bytes of the pattern
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(wa.pattern) + lane * (NPT / 2);
    int t[NPT];
#pragma unroll
    for (int q = 0; q < NPT / 2; ++q) {
        const uint32_t w = pw[q];
        const float px0 = (float)(int8_t)(w & 0xFF), py0 = (float)(int8_t)((w >> 8) & 0xFF);
        const float px1 = (float)(int8_t)((w >> 16) & 0xFF), py1 = (float)(int8_t)((w >> 24) & 0xFF);
        // (clamped into the staged patch: a no-op for every pattern the host lets through)
        const int ix0 = min(max(ORB_ROTATE_X(px0, py0, a, sb), -R), R), iy0 = min(max(ORB_ROTATE_Y(px0, py0, a, sb), -R), R);
        const int ix1 = min(max(ORB_ROTATE_X(px1, py1, a, sb), -R), R), iy1 = min(max(ORB_ROTATE_Y(px1, py1, a, sb), -R), R);
        t[2 * q] = bl[iy0 * (PW * 4) + ix0];
        t[2 * q + 1] = bl[iy1 * (PW * 4) + ix1];
    }
    uint32_t nib = 0u;
    if constexpr (WTA == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) nib |= (uint32_t)(t[2 * j] < t[2 * j + 1]) << j;
    } else if constexpr (WTA == 3) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t0 = t[3 * j], t1 = t[3 * j + 1], t2 = t[3 * j + 2];
            const uint32_t v = t2 > t1 ? (t2 > t0 ? 2u : 0u) : (uint32_t)(t1 > t0);
            nib |= v << (2 * j);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int t0 = t[4 * j], t2 = t[4 * j + 2];
            const int t1 = t[4 * j + 1], t3 = t[4 * j + 3];
            uint32_t va = 0u, vb = 2u;
            if (t1 > t0) { t0 = t1; va = 1u; }
            if (t3 > t2) { t2 = t3; vb = 3u; }
            nib |= (t0 > t2 ? va : vb) << (2 * j);
        }
    }
    // eight nibbles -> one word of the descriptor, written by every eighth lane
    uint32_t word = nib | (__shfl_down(nib, 1, 64) << 4);
    word |= __shfl_down(word, 2, 64) << 8;
    word |= __shfl_down(word, 4, 64) << 16;
    if ((lane & 7) == 0) *reinterpret_cast<uint32_t*>(o.desc + kk * 32 + (lane >> 1)) = word;
}

}  // namespace

// the two 8-bit image operations other front-ends share (lsd_kernels.hip: the scaled image of the line detector)
void launch_blur7_u8(hipStream_t s, int B, int cols, int rows, const uint8_t* src, uint8_t* dst, const int* k7, const OrbLevelSize* sz, int n_sz,
                     int sz_stride, int level) {
    OrbDev o{};
    o.B = B; o.cols = cols; o.rows = rows; o.img = src; o.blur = dst;
    o.sz = sz; o.n_sz = n_sz; o.sz_stride = sz_stride; o.level = level;
    BlurK kk{};
    for (int i = 0; i < 7; ++i) kk.k[i] = k7[i];
    const dim3 tiles((cols + 4 * BL_T - 1) / (4 * BL_T), (rows + BL_R - 1) / BL_R, B);
    if (sz) hipLaunchKernelGGL(orb_blur_kernel<true>, tiles, dim3(BL_T), 0, s, o, kk);
    else hipLaunchKernelGGL(orb_blur_kernel<false>, tiles, dim3(BL_T), 0, s, o, kk);
}
void launch_resize_linear_u8(hipStream_t s, int B, int scols, int srows, int dcols, int drows, const uint8_t* src, uint8_t* dst, double fx, double fy,
                             const OrbLevelSize* sz, int n_sz, int sz_stride, int level) {
    ResizeArgs r{};
    r.B = B; r.scols = scols; r.srows = srows; r.dcols = dcols; r.drows = drows;
    // fx, fy > 0: resize(src, dst, Size(), fx, fy) — cv::resize keeps inv_scale = fx and rounds only the output size; 0: a given dsize
    r.scale_x = 1.0 / (fx > 0 ? fx : (double)dcols / scols);
    r.scale_y = 1.0 / (fy > 0 ? fy : (double)drows / srows);
    r.src = src; r.dst = dst;
    r.sz = sz; r.n_sz = n_sz; r.sz_stride = sz_stride; r.level = level;
    const dim3 grid((dcols + 255) / 256, drows, B);
    if (sz) hipLaunchKernelGGL(orb_resize_kernel<true>, grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL(orb_resize_kernel<false>, grid, dim3(256), 0, s, r);
}
}  // namespace stvo

struct stvo_orb {
    stvo_ctx* ctx = nullptr;
    int B = 0, K = 0, nlevels = 1;
    int score_type = STVO_ORB_SCORE_FAST;
    stvo_orb_params prm{};
    struct Level {
        stvo::OrbDev d{};      // geometry, budget and scratch of the level (img / outputs are set per call)
        float scale = 1.f;
        uint8_t* img = nullptr;  // the resized image of the level (levels > 0)
        // per-level outputs when there is more than one level (level coordinates; orb_concat_kernel assembles the result)
        float *kp = nullptr, *resp = nullptr, *ang = nullptr;
        uint8_t* desc = nullptr;
        int32_t *n = nullptr, *n_tot = nullptr;
        bool active = true;    // a level without budget, or smaller than the border, yields nothing
    } lev[STVO_ORB_MAX_LEVELS];
    char* dev = nullptr;  // every device array of the object, carved from one allocation
    Staging io;           // staging for the host-buffer entry point: images in, results out
    int8_t pattern[1024];             // the pool of patch size 31 (stvo_orb_set_pattern; the stand-in by default)
    int8_t* d_pattern = nullptr;
    // the descriptor setting (stvo_orb_set_descriptor).  (2, 31) runs orb_describe_kernel on d_pattern; every other setting runs
    // orb_describe_wta_kernel on the effective pattern and the umax table of its half patch
    int wta_k = 2, patch_size = 31;
    int8_t effective[1024];           // what stvo_orb_get_pattern returns
    int8_t* d_effective = nullptr;    // [1024] + umax [64], carved from dev
    int32_t* d_th_own = nullptr;  // [B] device copy behind stvo_orb_set_fast_thresholds (carved from dev)
    stvo::BlurK blur_k{};
    stvo::Umax umax{};
    // one image size per image (stvo_orb_set_image_sizes): nothing of it exists until the first call.  The device table is an allocation
    // of its own ([B][nlevels] rows: the largest n); two pinned staging blocks are used alternately, each with the event of the copy
    // that last read it
    int nf[STVO_ORB_MAX_LEVELS] = {};       // the feature budget of every level
    stvo::OrbLevelSize* d_sizes = nullptr;
    int n_sizes = 0;                        // entries of the table in force; 0: every image fills its slot
    stvo::OrbLevelSize* sizes_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_sizes[2] = {nullptr, nullptr};
    bool sizes_busy[2] = {false, false};
    int sizes_next = 0;
};

namespace {

int pattern_verdict(int v) {
    return v == stvo::ORB_PATTERN_OK ? STVO_OK : (v == stvo::ORB_PATTERN_UNSUPPORTED ? STVO_ERR_UNSUPPORTED : STVO_ERR_INVALID_ARG);
}

}  // namespace

extern "C" {

int stvo_orb_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keypoints, const stvo_orb_params* prm, stvo_orb** out) {
    if (!ctx || !out || !prm || B <= 0 || cols < 64 || rows < 64 || max_keypoints <= 0) return STVO_ERR_INVALID_ARG;
    // the patch (radius 15) and the rotated pattern (|coordinate| <= 13 sqrt 2) must stay inside the image: edge >= 19
    if (prm->nfeatures <= 0 || prm->fast_threshold < 1 || prm->fast_threshold > 254 || prm->edge_threshold < 19 ||
        2 * prm->edge_threshold >= cols || 2 * prm->edge_threshold >= rows)
        return STVO_ERR_INVALID_ARG;
    const int nlevels = prm->nlevels <= 0 ? 1 : prm->nlevels;
    if (nlevels > STVO_ORB_MAX_LEVELS || (nlevels > 1 && !(prm->scale_factor > 1.0 && prm->scale_factor <= 2.0))) return STVO_ERR_INVALID_ARG;
    if (rows >= 4096 || cols >= 4096) return STVO_ERR_CAPACITY;  // candidates pack (y, x) in 12 bits each
    // the ordering kernel emits at most ORD_CAP key-points per level (its LDS sort): an output capacity beyond it cannot be honoured.
    // (nfeatures may be anything: when more key-points qualify than max_keypoints, the first max_keypoints of the row-major order
    // are selected exactly and n_total reports how many qualified)
    if (max_keypoints > stvo::ORD_CAP) return STVO_ERR_CAPACITY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_orb* o = new (std::nothrow) stvo_orb();
    if (!o) return STVO_ERR_HIP;
    o->ctx = ctx;
    o->prm = *prm;
    o->B = B; o->K = max_keypoints; o->nlevels = nlevels;
    // level geometry and feature budgets exactly as ORB_Impl forms them (orb_sizes.h)
    int* nf = o->nf;
    stvo::orb_level_budgets(prm->nfeatures, nlevels, prm->scale_factor, nf);
    stvo::OrbLevelSize slot[STVO_ORB_MAX_LEVELS];
    stvo::orb_level_sizes(cols, rows, nlevels, prm->scale_factor, prm->edge_threshold, nf, slot);
    int lcols[STVO_ORB_MAX_LEVELS], lrows[STVO_ORB_MAX_LEVELS];
    for (int l = 0; l < nlevels; ++l) {
        stvo_orb::Level& L = o->lev[l];
        L.scale = stvo::orb_level_scale(prm->scale_factor, l);
        stvo::OrbDev& d = L.d;
        d.B = B; d.K = max_keypoints;
        d.cols = lcols[l] = slot[l].cols;
        d.rows = lrows[l] = slot[l].rows;
        d.nfeatures = nf[l]; d.fast_th = prm->fast_threshold; d.edge_th = prm->edge_threshold;
        d.cand_cap = stvo::orb_cand_cap(d.cols, d.rows);
        L.active = slot[l].active != 0;
    }
    stvo::Carver size;
    stvo::carve_orb_arena(size, B, max_keypoints, nlevels, lcols, lrows);
    if (!hip_ok(ctx, hipMalloc((void**)&o->dev, size.off), "hipMalloc orb") || !zero_device(ctx, o->dev, size.off, "hipMemset orb")) {
        stvo_orb_destroy(o);
        return STVO_ERR_HIP;
    }
    stvo::Carver c(o->dev);
    const stvo::OrbArena a = stvo::carve_orb_arena(c, B, max_keypoints, nlevels, lcols, lrows);
    o->d_pattern = a.pattern; o->d_th_own = a.th_own; o->d_effective = a.effective;
    stvo::orb_default_pool(o->pattern);
    std::memcpy(o->effective, o->pattern, 1024);
    if (!upload_now(ctx, o->d_pattern, o->pattern, 1024, "hipMemcpy pattern")) {
        stvo_orb_destroy(o);
        return STVO_ERR_HIP;
    }
    for (int l = 0; l < nlevels; ++l) {
        stvo_orb::Level& L = o->lev[l];
        const stvo::OrbLevelBufs& q = a.lev[l];
        stvo::OrbDev& d = L.d;
        d.blur = q.blur; d.hist = q.hist; d.cand = q.cand; d.hkey = q.hkey; d.n_cand = q.n_cand;
        d.pattern = o->d_pattern;
        L.img = q.img;
        L.kp = q.kp; L.resp = q.resp; L.ang = q.ang; L.desc = q.desc; L.n = q.n; L.n_tot = q.n_tot;
    }
    stvo::gaussian_q8(3, 2.0, o->blur_k.k);  // getGaussianKernel(7, 2)
    stvo::orb_umax(stvo::ORB_HP, o->umax.u);  // umax of ICAngles
    *out = o;
    return STVO_OK;
}

int stvo_orb_destroy(stvo_orb* o) {
    if (!o) return STVO_OK;
    if (o->ctx) {
        (void)hipSetDevice(o->ctx->device);
        (void)hipStreamSynchronize(o->ctx->stream);
    }
    if (o->dev) (void)hipFree(o->dev);
    if (o->io.p) (void)hipFree(o->io.p);
    if (o->d_sizes) (void)hipFree(o->d_sizes);
    if (o->sizes_stage[0]) (void)hipHostFree(o->sizes_stage[0]);  // (one allocation for both blocks)
    for (hipEvent_t e : o->ev_sizes)
        if (e) (void)hipEventDestroy(e);
    delete o;
    return STVO_OK;
}

int stvo_orb_set_pattern(stvo_orb* o, const int8_t* pattern) {
    if (!o || !pattern) return STVO_ERR_INVALID_ARG;
    for (int i = 0; i < 1024; ++i)
        if (pattern[i] < -13 || pattern[i] > 13) return STVO_ERR_INVALID_ARG;  // rotated points must stay within the border
    // the effective pattern of the setting in force is derived again (it depends on the pool only at patch size 31); a pool the
    // setting cannot use — fewer different points than a tuple of WTA_K 3 / 4 holds — is refused and nothing changes
    int8_t eff[1024];
    if (o->patch_size == 31) {
        const int v = pattern_verdict(stvo::orb_effective_pattern(o->wta_k, 31, pattern, eff, nullptr));
        if (v != STVO_OK) return v;
    } else {
        std::memcpy(eff, o->effective, 1024);
    }
    HIP_TRY(o->ctx, hipSetDevice(o->ctx->device));
    HIP_TRY(o->ctx, hipStreamSynchronize(o->ctx->stream));
    std::memcpy(o->pattern, pattern, 1024);
    std::memcpy(o->effective, eff, 1024);
    if (!upload_now(o->ctx, o->d_pattern, o->pattern, 1024, "hipMemcpy pattern")) return STVO_ERR_HIP;
    if (!upload_now(o->ctx, o->d_effective, o->effective, 1024, "hipMemcpy pattern")) return STVO_ERR_HIP;
    return STVO_OK;
}

int stvo_orb_set_descriptor(stvo_orb* o, int wta_k, int patch_size) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (wta_k == o->wta_k && patch_size == o->patch_size) return STVO_OK;  // in force already (stvo_orb_set_pattern keeps its tables current)
    int8_t eff[1024];
    const int v = pattern_verdict(stvo::orb_effective_pattern(wta_k, patch_size, o->pattern, eff, nullptr));
    if (v != STVO_OK) return v;
    // everything the kernels read lies inside the level image: key-points keep edge_threshold from its border, the moments reach the
    // half patch and the rotated points the reach of the setting (19 at patch size 31, which stvo_orb_create has already required)
    if (patch_size != 31 && o->prm.edge_threshold < stvo::orb_reach(patch_size)) return STVO_ERR_INVALID_ARG;
    int8_t tab[1024 + 64];
    std::memcpy(tab, eff, 1024);
    {
        int u[stvo::ORB_MAX_HALF_PATCH + 2];
        stvo::orb_umax(stvo::orb_half_patch(patch_size), u);
        for (int i = 0; i < 64; ++i) tab[1024 + i] = i <= stvo::orb_half_patch(patch_size) ? (int8_t)u[i] : 0;
    }
    HIP_TRY(o->ctx, hipSetDevice(o->ctx->device));
    HIP_TRY(o->ctx, hipStreamSynchronize(o->ctx->stream));  // (detections already enqueued may still read the previous tables)
    if (!upload_now(o->ctx, o->d_effective, tab, sizeof tab, "hipMemcpy pattern")) return STVO_ERR_HIP;
    std::memcpy(o->effective, eff, 1024);
    o->wta_k = wta_k;
    o->patch_size = patch_size;
    return STVO_OK;
}

int stvo_orb_pattern(int wta_k, int patch_size, const int8_t* pool, int8_t* out, int32_t* n_points) {
    if (!out) return STVO_ERR_INVALID_ARG;
    int n = 0;
    const int v = pattern_verdict(stvo::orb_effective_pattern(wta_k, patch_size, pool, out, &n));
    if (v == STVO_OK && n_points) *n_points = n;
    return v;
}

int stvo_orb_set_fast_threshold(stvo_orb* o, int fast_threshold) {
    if (!o || fast_threshold < 1 || fast_threshold > 254) return STVO_ERR_INVALID_ARG;
    o->prm.fast_threshold = fast_threshold;
    for (int l = 0; l < o->nlevels; ++l) o->lev[l].d.fast_th = fast_threshold;  // kernel argument of the next launches
    return STVO_OK;
}

int stvo_orb_set_fast_thresholds_dev(stvo_orb* o, const int32_t* th_dev, int n_th) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (th_dev && (n_th <= 0 || n_th > o->B || o->B % n_th != 0)) return STVO_ERR_INVALID_ARG;
    for (int l = 0; l < o->nlevels; ++l) {  // kernel arguments of the next launches; the array itself is read by those launches
        o->lev[l].d.th = th_dev;
        o->lev[l].d.n_th = th_dev ? n_th : 0;
    }
    return STVO_OK;
}

int stvo_orb_set_fast_thresholds(stvo_orb* o, const int32_t* th_host, int n_th) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (!th_host) return stvo_orb_set_fast_thresholds_dev(o, nullptr, 0);
    if (n_th <= 0 || n_th > o->B || o->B % n_th != 0) return STVO_ERR_INVALID_ARG;
    for (int i = 0; i < n_th; ++i)
        if (th_host[i] < 1 || th_host[i] > 254) return STVO_ERR_INVALID_ARG;
    HIP_TRY(o->ctx, hipSetDevice(o->ctx->device));
    // (ordered behind the detections already enqueued, which may still read the previous contents)
    HIP_TRY(o->ctx, hipMemcpyAsync(o->d_th_own, th_host, (size_t)n_th * 4, hipMemcpyHostToDevice, o->ctx->stream));
    HIP_TRY(o->ctx, hipStreamSynchronize(o->ctx->stream));
    return stvo_orb_set_fast_thresholds_dev(o, o->d_th_own, n_th);
}

// One image size per image (stvo_hip.h).  Validated before anything changes.  The table is formed on the host (orb_sizes.h) in a pinned
// block and copied on the context's stream, so it arrives behind the detections already enqueued (which read the previous contents) and in
// front of the next one; nothing waits for it.  A pinned block is written again only after the copy that last read it (two calls ago) has
// completed — long since, unless nothing has synchronised in between.
int stvo_orb_set_image_sizes(stvo_orb* o, const int32_t* sizes_host, int n) {
    if (!o) return STVO_ERR_INVALID_ARG;
    if (!sizes_host) {  // every image fills its slot again: the uniform kernel instances, which read no table
        o->n_sizes = 0;
        return STVO_OK;
    }
    const stvo::OrbDev& d0 = o->lev[0].d;
    if (!stvo::orb_image_sizes_ok(sizes_host, n, o->B, d0.cols, d0.rows, o->prm.edge_threshold)) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t span = ((size_t)o->B * o->nlevels * sizeof(stvo::OrbLevelSize) + 255) & ~size_t(255);
    if (!o->d_sizes) HIP_TRY(ctx, hipMalloc((void**)&o->d_sizes, span));
    if (!o->sizes_stage[0]) {
        HIP_TRY(ctx, hipHostMalloc((void**)&o->sizes_stage[0], 2 * span, hipHostMallocDefault));
        o->sizes_stage[1] = reinterpret_cast<stvo::OrbLevelSize*>(reinterpret_cast<char*>(o->sizes_stage[0]) + span);
    }
    for (auto& e : o->ev_sizes)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int hb = o->sizes_next;
    if (o->sizes_busy[hb]) {
        HIP_TRY(ctx, hipEventSynchronize(o->ev_sizes[hb]));
        o->sizes_busy[hb] = false;
    }
    stvo::OrbLevelSize* tab = o->sizes_stage[hb];
    for (int i = 0; i < n; ++i)
        stvo::orb_level_sizes(sizes_host[2 * i], sizes_host[2 * i + 1], o->nlevels, o->prm.scale_factor, o->prm.edge_threshold, o->nf, tab + (size_t)i * o->nlevels);
    HIP_TRY(ctx, hipMemcpyAsync(o->d_sizes, tab, (size_t)n * o->nlevels * sizeof(stvo::OrbLevelSize), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(o->ev_sizes[hb], ctx->stream));
    o->sizes_busy[hb] = true;
    o->sizes_next = hb ^ 1;
    o->n_sizes = n;
    return STVO_OK;
}

int stvo_orb_set_score_type(stvo_orb* o, int score_type) {
    if (!o || (score_type != STVO_ORB_SCORE_HARRIS && score_type != STVO_ORB_SCORE_FAST)) return STVO_ERR_INVALID_ARG;
    o->score_type = score_type;
    for (int l = 0; l < o->nlevels; ++l) o->lev[l].d.score_harris = score_type == STVO_ORB_SCORE_HARRIS;  // kernel argument of the next launches
    return STVO_OK;
}

int stvo_orb_get_pattern(const stvo_orb* o, int8_t* pattern) {
    if (!o || !pattern) return STVO_ERR_INVALID_ARG;
    std::memcpy(pattern, o->effective, 1024);
    return STVO_OK;
}

int stvo_orb_detect_levels_dev(stvo_orb* o, const uint8_t* images, float* kp_xy, float* response, float* angle, int32_t* octave,
                               uint8_t* desc, int32_t* n_kp, int32_t* n_total) {
    if (!o || !images || !kp_xy || !response || !angle || !desc || !n_kp) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool multi = o->nlevels > 1;
    // one size per image: the MIXED instances of the three kernels that see an image border (FAST + NMS, blur, resize) on the slots' launch
    // grids; the others index with the slot's pitch and stay inside the image through the edge threshold.  A level the slot is too small
    // for is too small for every entry (cvRound is monotone), so the slot's `active` below still skips it as a whole.
    const bool mixed = o->n_sizes > 0;
    const uint8_t* prev = images;
    for (int l = 0; l < o->nlevels; ++l) {
        stvo_orb::Level& L = o->lev[l];
        stvo::OrbDev d = L.d;
        d.sz = mixed ? o->d_sizes : nullptr; d.n_sz = o->n_sizes; d.sz_stride = o->nlevels; d.level = l;
        if (l) {  // resize(level l - 1): needed by the next level even when this one yields nothing
            const stvo::OrbDev& p = o->lev[l - 1].d;
            stvo::ResizeArgs r{d.B, p.cols, p.rows, d.cols, d.rows, 1.0 / ((double)d.cols / p.cols), 1.0 / ((double)d.rows / p.rows), prev, L.img,
                               d.sz, d.n_sz, d.sz_stride, l};
            const dim3 rgrid((d.cols + 255) / 256, d.rows, d.B);
            if (mixed) hipLaunchKernelGGL(stvo::orb_resize_kernel<true>, rgrid, dim3(256), 0, s, r);
            else hipLaunchKernelGGL(stvo::orb_resize_kernel<false>, rgrid, dim3(256), 0, s, r);
            d.img = L.img;
        } else {
            d.img = images;
        }
        prev = d.img;
        if (multi) {
            d.kp = L.kp; d.resp = L.resp; d.angle = L.ang; d.desc = L.desc; d.n_kp = L.n; d.n_total = L.n_tot;
        } else {
            d.kp = kp_xy; d.resp = response; d.angle = angle; d.desc = desc; d.n_kp = n_kp; d.n_total = n_total;
        }
        if (!L.active) {
            HIP_TRY(ctx, hipMemsetAsync(d.n_kp, 0, (size_t)d.B * 4, s));
            if (d.n_total) HIP_TRY(ctx, hipMemsetAsync(d.n_total, 0, (size_t)d.B * 4, s));
            continue;
        }
        const dim3 tiles((d.cols + 4 * stvo::BL_T - 1) / (4 * stvo::BL_T), (d.rows + stvo::BL_R - 1) / stvo::BL_R, d.B), tb(stvo::BL_T);
        const dim3 ftiles((d.cols + stvo::FT_W - 1) / stvo::FT_W, (d.rows + stvo::FT_H - 1) / stvo::FT_H, d.B);
        if (mixed) {
            hipLaunchKernelGGL(stvo::orb_fast_nms_kernel<true>, ftiles, dim3(256), 0, s, d);
            hipLaunchKernelGGL(stvo::orb_blur_kernel<true>, tiles, tb, 0, s, d, o->blur_k);
        } else {
            hipLaunchKernelGGL(stvo::orb_fast_nms_kernel<false>, ftiles, dim3(256), 0, s, d);
            hipLaunchKernelGGL(stvo::orb_blur_kernel<false>, tiles, tb, 0, s, d, o->blur_k);
        }
        if (d.score_harris) {
            hipLaunchKernelGGL(stvo::orb_harris_kernel, dim3(stvo::HR_BLOCKS, d.B), dim3(256), 0, s, d);
            hipLaunchKernelGGL(stvo::orb_order_kernel<true>, dim3(d.B), dim3(1024), 0, s, d);
        } else {
            hipLaunchKernelGGL(stvo::orb_order_kernel<false>, dim3(d.B), dim3(1024), 0, s, d);
        }
        if (o->wta_k == 2 && o->patch_size == 31) {
            hipLaunchKernelGGL(stvo::orb_describe_kernel, dim3((unsigned)(((d.K + stvo::DESC_KP_PER_WG - 1) / stvo::DESC_KP_PER_WG) * ((d.B + 7) / 8) * 8)), dim3(256),
                               0, s, d, o->umax);
        } else {
            const stvo::WtaArgs wa{stvo::orb_half_patch(o->patch_size), stvo::orb_reach(o->patch_size), o->d_effective, o->d_effective + 1024};
            const dim3 grid((unsigned)(((d.K + stvo::WTA_KP_PER_WG - 1) / stvo::WTA_KP_PER_WG) * ((d.B + 7) / 8) * 8));
            const bool big = wa.R > 22;  // the instance whose LDS patch holds the reach
            auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, d, wa); };
            if (o->wta_k == 2) big ? launch(stvo::orb_describe_wta_kernel<2, 44>) : launch(stvo::orb_describe_wta_kernel<2, 22>);
            else if (o->wta_k == 3) big ? launch(stvo::orb_describe_wta_kernel<3, 44>) : launch(stvo::orb_describe_wta_kernel<3, 22>);
            else big ? launch(stvo::orb_describe_wta_kernel<4, 44>) : launch(stvo::orb_describe_wta_kernel<4, 22>);
        }
    }
    if (multi) {
        stvo::ConcatArgs c{};
        c.B = o->B; c.K = o->K; c.nlevels = o->nlevels; c.Kl = o->K;
        for (int l = 0; l < o->nlevels; ++l) {
            const stvo_orb::Level& L = o->lev[l];
            c.scale[l] = L.scale; c.kp[l] = L.kp; c.resp[l] = L.resp; c.ang[l] = L.ang; c.desc[l] = L.desc; c.n[l] = L.n; c.n_tot[l] = L.n_tot;
        }
        c.kp_o = kp_xy; c.resp_o = response; c.ang_o = angle; c.oct_o = octave; c.desc_o = desc; c.n_o = n_kp; c.n_total_o = n_total;
        hipLaunchKernelGGL(stvo::orb_concat_kernel, dim3(o->B), dim3(256), 0, s, c);
    } else if (octave) {
        HIP_TRY(ctx, hipMemsetAsync(octave, 0, (size_t)o->B * o->K * 4, s));
    }
    return check_launch(ctx);
}

int stvo_orb_detect_dev(stvo_orb* o, const uint8_t* images, float* kp_xy, float* response, float* angle, uint8_t* desc,
                        int32_t* n_kp) {
    return stvo_orb_detect_levels_dev(o, images, kp_xy, response, angle, nullptr, desc, n_kp, nullptr);
}

int stvo_orb_detect_levels(stvo_orb* o, const uint8_t* images, float* kp_xy, float* response, float* angle, int32_t* octave, uint8_t* desc,
                           int32_t* n_kp, int32_t* n_total) {
    if (!o || !images || !kp_xy || !response || !angle || !desc || !n_kp) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = o->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const stvo::OrbDev& d = o->lev[0].d;
    const size_t px = (size_t)d.B * d.rows * d.cols, nk = (size_t)d.B * d.K;
    stvo::Carver size;
    stvo::carve_orb_staging(size, d.B, d.cols, d.rows, d.K);
    TRY(staging_reserve(ctx, o->io, size.off));
    stvo::Carver c(o->io.p);
    const stvo::OrbStaging S = stvo::carve_orb_staging(c, d.B, d.cols, d.rows, d.K);
    HIP_TRY(ctx, hipMemcpyAsync(S.img, images, px, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(S.kp, 0, (size_t)(o->io.p + c.off - (char*)S.kp), ctx->stream));
    TRY(stvo_orb_detect_levels_dev(o, S.img, S.kp, S.resp, S.ang, S.oct, S.desc, S.n, S.n_total));
    HIP_TRY(ctx, hipMemcpyAsync(kp_xy, S.kp, nk * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(response, S.resp, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(angle, S.ang, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (octave) HIP_TRY(ctx, hipMemcpyAsync(octave, S.oct, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(desc, S.desc, nk * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_kp, S.n, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_total) HIP_TRY(ctx, hipMemcpyAsync(n_total, S.n_total, (size_t)d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_orb_detect(stvo_orb* o, const uint8_t* images, float* kp_xy, float* response, float* angle, uint8_t* desc, int32_t* n_kp) {
    return stvo_orb_detect_levels(o, images, kp_xy, response, angle, nullptr, desc, n_kp, nullptr);
}

}  // extern "C"
