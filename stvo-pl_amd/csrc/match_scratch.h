// match_scratch.h — the scratch of the brute-force descriptor matcher (match_kernels.hip, match_mfma.hip), stated ONCE: which arrays a
// match works in, what each path keeps where in them, and when a problem fits.  Also the two small rules host and device share: the
// train segments of a scan (knn_pick_nseg) and the largest distance that still blocks a claim (block_threshold).  Host-pure: g++ alone
// compiles it (under hipcc uint2 is HIP's); tests/cpp/match_scratch_host.cpp runs everything here without a device.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>
#else
struct alignas(8) uint2 { unsigned x, y; };
#endif
#if defined(__HIPCC__)
#define STVO_MATCH_HD __host__ __device__
#else
#define STVO_MATCH_HD
#endif

namespace stvo {

// The arrays a context (stvo_ctx, or the key-line scratch of a pipeline: seq_state.h) owns for the matcher.  knn12 / knn21 hold
// knn_capacity packed (best_key, second_key) pairs each, key = (distance << 16) | train index; the per-row arrays hold at least
// B * row_stride entries of every problem the owner admits, nsel at least 5 * B.
struct MatchScratch {
    uint2* knn12;         // [nseg][B][row_stride] forward top-2 per train segment; consumers merge the segments
    uint2* knn21;         // BOTH_DIRS: the reverse top-2, as knn12.  LAZY: `blocked` (VALU path) or `tsel` (matrix-core path), see MatchViews
    int32_t* cand;        // [B][row_stride] forward ratio-tested best (VALU path)
    uint32_t* claim;      // [B][row_stride] per-column claim (d0 << 16 | claimant), 0xFFFFFFFF = unclaimed
    int32_t* qsel;        // [B][row_stride] claimed columns: compacted (VALU path); light from the front, heavy from the back (matrix-core path)
    int32_t* nsel;        // [5][B] claimed columns; light, heavy, |S|, tau of the matrix-core reverse check (forward_plan_kernel)
    size_t knn_capacity;  // elements of knn12 and of knn21
};

// A lazy match of (B, row_stride) keeps nseg >= 1 segments of forward top-2 in knn12 and B * row_stride int32 at either end of knn21:
// the problem fits when two segments' worth of pairs do (knn_pick_nseg never picks more segments than fit).
inline bool match_scratch_fits(int B, int row_stride, size_t knn_capacity) {
    return B >= 0 && row_stride >= 0 && (size_t)2 * (size_t)B * (size_t)row_stride <= knn_capacity;
}

// What the kernels of one match are handed, typed.  Within knn21 (2 * knn_capacity int32): `blocked` is its first B * row_stride int32,
// `tsel` its last B * row_stride; no launch uses both.
struct MatchViews {
    size_t per;        // B * row_stride: entries of a per-row array, and of one knn12 segment
    uint2* knn12;      // segment s at knn12_seg(s)
    uint32_t* claim;
    int32_t* cand;
    int32_t* qsel;
    int32_t* nsel;     // row k at nsel_row(k)
    int32_t* blocked;  // VALU path: [B][row_stride] verdict of hamming_verify_kernel per claimed column
    int32_t* tsel;     // matrix-core path: [B][row_stride] the rows of S (forward_plan_kernel)
    int B;
    uint2* knn12_seg(int s) const { return knn12 + (size_t)s * per; }
    int32_t* nsel_row(int k) const { return nsel + (size_t)k * (size_t)B; }
};
inline MatchViews match_views(const MatchScratch& w, int B, int row_stride) {
    MatchViews v;
    v.per = (size_t)B * (size_t)row_stride;
    v.knn12 = w.knn12;
    v.claim = w.claim;
    v.cand = w.cand;
    v.qsel = w.qsel;
    v.nsel = w.nsel;
    v.blocked = reinterpret_cast<int32_t*>(w.knn21);
    v.tsel = reinterpret_cast<int32_t*>(w.knn21) + (2 * w.knn_capacity - v.per);
    v.B = B;
    return v;
}

constexpr int KNN_MIN_NSEG = 2, KNN_MAX_NSEG = 16;  // train-range segments per query tile in K1
// Segments per query tile: 1 for very big batches, 2 for big ones (short dispatch rounds), up to 16 for a single frame pair so
// that one 2000 x 2000 problem still spreads over a few hundred workgroups (single-stream latency).
// `capacity` = elements of the knn scratch arrays: nseg * B * max_n must fit.  `forced` > 0: a developer's choice (STVO_KNN_NSEG).
inline int knn_pick_nseg(int B, int max_n, size_t capacity, int forced) {
    const int tiles = (max_n + 255) / 256;
    int nseg = (2048 + B * tiles - 1) / (B * tiles > 0 ? B * tiles : 1);
    nseg = nseg < KNN_MIN_NSEG ? KNN_MIN_NSEG : (nseg > KNN_MAX_NSEG ? KNN_MAX_NSEG : nseg);
    if ((long long)B * tiles >= 4096) nseg = 1;  // >= 5 dispatch rounds even unsegmented: a workgroup's fixed cost is paid once per query tile
                                                 // (1024 frames: K1m 0.562 -> 0.551 ms, reverse check 0.054 -> 0.050 ms)
    if (forced > 0) nseg = forced;
    const size_t per_seg = (size_t)(B > 0 ? B : 1) * (size_t)(max_n > 0 ? max_n : 1);
    while (nseg > 1 && (size_t)nseg * per_seg > capacity) --nseg;
    return nseg;
}

// A row claims a column at distance d0; the claim survives the reverse ratio test iff no other row lies within
// block_threshold(d0) = the largest d' in [d0, 256] for which float(d0) < float(d') * nnr is FALSE (match_kernels.hip: lazy mutual matching).
STVO_MATCH_HD inline __attribute__((always_inline)) uint32_t block_threshold(uint32_t d0, float nnr) {
    const float f0 = (float)d0;
    uint32_t thr = d0;
    while (thr < 256u && !(f0 < (float)(thr + 1u) * nnr)) ++thr;  // largest distance that still blocks
    return thr;
}

}  // namespace stvo
