// orb_sizes.h — the geometry of the ORB pyramid, host-pure (no HIP): level sizes, feature budgets, the resize ratios and the rule by which
// a level yields anything, stated once for stvo_orb_create (one size for all images) and stvo_orb_set_image_sizes (one size per image).
// Exactly as ORB_Impl forms them (oracle/stvo_orb_oracle.c: orc_orb_levels): level l of an image cols x rows is
//   cvRound((float)cols / scale_l) x cvRound((float)rows / scale_l),  scale_l = (float)pow(scale_factor, l),  cvRound = half to even,
// and level l is resized from level l - 1 with cv::resize's inverse scales for a given dsize, 1.0 / ((double)dsize / ssize), per axis.
// tests/test_orb_sizes_host.py runs this header on the host (tests/cpp/orb_sizes_host.cpp) against the oracle's statement.
#pragma once
#include <cmath>
#include <cstdint>

namespace stvo {

// One row of the per-image size table: level l of entry e is row e * nlevels + l.  32 bytes, read by a workgroup with scalar loads.
struct OrbLevelSize {
    int32_t cols, rows;      // the level image (it occupies the top-left of the slot's level buffer; the pitch stays the slot's)
    double inv_sx, inv_sy;   // resize from level l - 1: source position = (d + 0.5) inv_s - 0.5 (1.0 at level 0, which is never resized)
    int32_t active;          // 0: the level yields nothing for this entry (no budget, or smaller than the border)
    int32_t pad;
};
static_assert(sizeof(OrbLevelSize) == 32, "the kernels read a row as 32 bytes");

inline int orb_size_round(float v) { return (int)std::lrintf(v); }  // cvRound: half to even

inline float orb_level_scale(double scale_factor, int l) { return l ? (float)std::pow(scale_factor, (double)l) : 1.f; }

// the feature budget of every level (ORB_Impl::computeKeyPoints); one level takes everything
inline void orb_level_budgets(int nfeatures, int nlevels, double scale_factor, int* nf /* [nlevels] */) {
    const float factor = (float)(1.0 / (nlevels > 1 ? scale_factor : 1.2));
    float nd = (float)nfeatures * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        nf[l] = orb_size_round(nd);
        sum += nf[l];
        nd *= factor;
    }
    nf[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
    if (nlevels == 1) nf[0] = nfeatures;
}

// a level runs when it has a budget and is larger than the border on both axes (and large enough for the word loads of the kernels)
inline bool orb_level_active(int nf, int edge_th, int cols, int rows) {
    return nf > 0 && 2 * edge_th < cols && 2 * edge_th < rows && cols >= 16 && rows >= 16;
}

// the nlevels rows of one image size.  nf: orb_level_budgets of the detector
inline void orb_level_sizes(int cols, int rows, int nlevels, double scale_factor, int edge_th, const int* nf, OrbLevelSize* out /* [nlevels] */) {
    for (int l = 0; l < nlevels; ++l) {
        const float sc = orb_level_scale(scale_factor, l);
        OrbLevelSize& e = out[l];
        e.cols = l ? orb_size_round((float)cols / sc) : cols;
        e.rows = l ? orb_size_round((float)rows / sc) : rows;
        e.inv_sx = l ? 1.0 / ((double)e.cols / out[l - 1].cols) : 1.0;
        e.inv_sy = l ? 1.0 / ((double)e.rows / out[l - 1].rows) : 1.0;
        e.active = orb_level_active(nf[l], edge_th, e.cols, e.rows) ? 1 : 0;
        e.pad = 0;
    }
}

// what stvo_orb_create asks of an image size (beyond the 12-bit coordinate range, which the slot already satisfies)
inline bool orb_image_size_ok(int cols, int rows, int edge_th) {
    return cols >= 64 && rows >= 64 && 2 * edge_th < cols && 2 * edge_th < rows;
}

// stvo_orb_set_image_sizes: n entries for B images in slots of slot_cols x slot_rows
inline bool orb_image_sizes_ok(const int32_t* sizes /* [n][2] = cols, rows */, int n, int B, int slot_cols, int slot_rows, int edge_th) {
    if (!sizes || n <= 0 || n > B || B % n != 0) return false;
    for (int i = 0; i < n; ++i) {
        const int c = sizes[2 * i], r = sizes[2 * i + 1];
        if (c > slot_cols || r > slot_rows || !orb_image_size_ok(c, r, edge_th)) return false;
    }
    return true;
}

}  // namespace stvo
