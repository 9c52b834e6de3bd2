// seq_layout.h — the memory layouts of the device-resident pipeline, each stated ONCE: the raw frame slot, a stereo set, the block of
// match indices and inlier masks the host mirrors, all cut with the carver of carver.h.  Host-pure (g++ alone compiles it; under
// hipcc the vector types are HIP's): tests/cpp/seq_layout_host.cpp runs every layout here without a device.
#pragma once

#include <type_traits>

#include "../../include/stvo_types.h"
#include "carver.h"

namespace stvo {

// ---- a raw frame slot: the features of one frame of all B sequences as uploaded, K / M rows per image ------------------------------
// One field list, two views: the kernels of a step read a slot (RawFrameView), the two upload routes write one (RawFrame).
template <bool CONST>
struct RawFrameT {
    template <typename T>
    using P = typename std::conditional<CONST, const T, T>::type*;
    P<float> kp_l; P<int32_t> oct_l; P<uint8_t> desc_l; P<int32_t> n_kp_l;    // left key-points: [B][K][2], [B][K], [B][K][32], [B]
    P<float> kp_r; P<uint8_t> desc_r; P<int32_t> n_kp_r;                      // right key-points
    P<float> kl_l; P<int32_t> oct_ll; P<uint8_t> ldesc_l; P<int32_t> n_kl_l;  // left key-lines: [B][M][4], [B][M], [B][M][32], [B]
    P<float> kl_r; P<uint8_t> ldesc_r; P<int32_t> n_kl_r;                     // right key-lines
};
typedef RawFrameT<false> RawFrame;
typedef RawFrameT<true> RawFrameView;

struct RawFrameSpan {
    size_t lines_off;  // first byte of the key-line part: a split upload copies [0, lines_off) on one stream, [lines_off, bytes) on another
    size_t bytes;      // of one slot
};

// The arrays of the slot at `base` (device memory, or its pinned mirror).  The key-line arrays are the tail by construction: everything
// cut behind `lines_off` belongs to them.
template <bool CONST>
inline RawFrameT<CONST> raw_frame(typename RawFrameT<CONST>::template P<char> base, int B, int K, int M, RawFrameSpan* span = nullptr) {
    const size_t nb = (size_t)B, nK = nb * K, nM = nb * M;
    Carver c(base);
    RawFrameT<CONST> r;
    r.kp_l = c.take<float>(nK * 2); r.oct_l = c.take<int32_t>(nK); r.desc_l = c.take<uint8_t>(nK * STVO_DESC_BYTES); r.n_kp_l = c.take<int32_t>(nb);
    r.kp_r = c.take<float>(nK * 2); r.desc_r = c.take<uint8_t>(nK * STVO_DESC_BYTES); r.n_kp_r = c.take<int32_t>(nb);
    const size_t lines_off = c.off;
    r.kl_l = c.take<float>(nM * 4); r.oct_ll = c.take<int32_t>(nM); r.ldesc_l = c.take<uint8_t>(nM * STVO_DESC_BYTES); r.n_kl_l = c.take<int32_t>(nb);
    r.kl_r = c.take<float>(nM * 4); r.ldesc_r = c.take<uint8_t>(nM * STVO_DESC_BYTES); r.n_kl_r = c.take<int32_t>(nb);
    if (span) *span = RawFrameSpan{lines_off, c.off};
    return r;
}
inline RawFrameSpan raw_frame_span(int B, int K, int M) { RawFrameSpan s; (void)raw_frame<true>(nullptr, B, K, M, &s); return s; }
inline size_t raw_frame_bytes(int B, int K, int M) { return raw_frame_span(B, K, M).bytes; }

// ---- a stereo set: what the association of one frame leaves, [B][K] / [B][M] rows each ----------------------------------------------
// The pipeline rotates through three of them (seq_state.h); a key-frame set (track_kernel.hip) is one without the counts.
struct StereoSetPtrs {
    float4* rc;     // [B][K] {u, v, disparity, level}: the stereo point (point_tail.h)
    uint8_t* desc;  // [B][K][32]
    int32_t* n;     // [B]
    double *spl, *epl;      // [B][M][2]
    double *sP, *eP, *le;   // [B][M][3]
    double* s2l;    // [B][M] stereo sigma2
    double* s2lm;   // [B][M] sigma2 after LineFeature::safeCopy's re-scaling (what matched_ls carries)
    uint8_t* ldesc;  // [B][M][32]
    int32_t* nl;     // [B]
};
inline StereoSetPtrs carve_stereo_set(Carver& c, int B, int K, int M, bool with_counts) {
    const size_t nb = (size_t)B, nK = nb * K, nM = nb * M;
    StereoSetPtrs q;
    q.rc = c.take<float4>(nK); q.desc = c.take<uint8_t>(nK * STVO_DESC_BYTES); q.n = with_counts ? c.take<int32_t>(nb) : nullptr;
    q.spl = c.take<double>(nM * 2); q.epl = c.take<double>(nM * 2);
    q.sP = c.take<double>(nM * 3); q.eP = c.take<double>(nM * 3); q.le = c.take<double>(nM * 3);
    q.s2l = c.take<double>(nM); q.s2lm = c.take<double>(nM);
    q.ldesc = c.take<uint8_t>(nM * STVO_DESC_BYTES); q.nl = with_counts ? c.take<int32_t>(nb) : nullptr;
    return q;
}

// ---- the fetch block: the by-products a caller may want on the host (stvo_seq_enable_fetch) -----------------------------------------
// Six device arrays cut back to back, so that one pinned block mirrors them at the same offsets: [m12s_p | m12s_l | m12p | m12l] leaves
// behind the f2f stage in one copy, [inlp | inll] behind the pose kernel in another, and a flag word follows (PoseSync::fetch_flag).
struct FetchBlock {
    int32_t *m12s_p, *m12s_l;  // [B][K] / [B][M] stereo matches of the left features
    int32_t *m12p, *m12l;      // f2f matches of the previous stereo features
    int32_t *inlp, *inll;      // the pose kernel's inlier masks
    size_t off_m12s_l, off_m12p, off_m12l, off_inlp, off_inll, off_flag;  // byte offsets from m12s_p, i.e. inside the pinned mirror
    size_t m12_span() const { return off_inlp; }             // bytes of [m12s_p | m12s_l | m12p | m12l]
    size_t inl_span() const { return off_flag - off_inlp; }  // bytes of [inlp | inll]
    size_t mirror_bytes() const { return off_flag + 64; }
};
inline FetchBlock carve_fetch_block(Carver& c, int B, int K, int M) {
    const size_t nb = (size_t)B, o0 = c.off;
    FetchBlock f;
    f.m12s_p = c.take<int32_t>(nb * K);
    f.off_m12s_l = c.off - o0; f.m12s_l = c.take<int32_t>(nb * M);
    f.off_m12p = c.off - o0;   f.m12p = c.take<int32_t>(nb * K);
    f.off_m12l = c.off - o0;   f.m12l = c.take<int32_t>(nb * M);
    f.off_inlp = c.off - o0;   f.inlp = c.take<int32_t>(nb * K);
    f.off_inll = c.off - o0;   f.inll = c.take<int32_t>(nb * M);
    f.off_flag = c.off - o0;
    return f;
}

}  // namespace stvo
