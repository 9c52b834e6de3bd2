// lsd_sizes.h — the geometry of one image size under a line detector's parameters, host-pure (no HIP): the scaled size, the smallest
// region the search keeps, the resize's inverse ratio and the minimum line length, stated once for stvo_lsd_geometry / stvo_lsd_create
// (one size for all images) and stvo_lsd_set_image_sizes (one size per image); and the same check of a size list for the descriptor of
// those key-lines (stvo_lbd_set_image_sizes).  Exactly as the detector forms them (oracle/stvo_lsd_oracle.c):
//   scaled size    cv::resize(img, Size(), scale, scale): cvRound(cols scale) x cvRound(rows scale), cvRound = half to even; the image
//                  itself at scale 1
//   min_reg_size   -(5 (log10 w + log10 h) / 2 + log10 11) / log10(ang_th / 180) of the SCALED size, truncated
//   inverse ratio  1 / scale: the sample step of the resize (Size() + fx keeps inv_scale = fx, only the size is rounded)
// tests/test_lsd_sizes_host.py runs this header on the host (tests/cpp/lsd_sizes_host.cpp) against stvo_lsd_geometry and the oracle.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "orb_sizes.h"

namespace stvo {

// One row of the detector's per-image table, entry e = row e.  32 bytes, read by a workgroup with scalar loads.
struct LsdSizeRow {
    int32_t cols, rows;    // the input image (top-left of its slot, whose pitch it keeps)
    int32_t w, h;          // the scaled image (top-left of the slot's scaled buffer; compact inside the search arena)
    int32_t min_reg_size;  // regions below it leave no segment
    int32_t pad;
    double min_length;     // key-lines must be longer (pixels of the input image)
};
static_assert(sizeof(LsdSizeRow) == 32, "the kernels read a row as 32 bytes");

// One image size per image (stvo_lsd_set_image_sizes) as the kernels take it: image i is sized by row i % n_sz of the table.  A kernel
// argument of its own behind the kernel's arguments, and empty for the uniform instances — they take the arguments they always took
// (lsd_kernels.hip and lsd_scale_kernels.hip).
template <bool MIXED>
struct LsdTable {};
template <>
struct LsdTable<true> {
    const LsdSizeRow* sz;
    int n_sz;
};

// one axis of the scaled image, as a double: the callers look at its range before they narrow it
inline double lsd_scaled_extent(int n, double scale) { return scale != 1 ? std::rint((double)n * scale) : (double)n; }

inline int lsd_min_reg_size(int w, int h, double ang_th) {
    const double p = ang_th / 180;
    const double log_nt = 5 * (std::log10((double)w) + std::log10((double)h)) / 2 + std::log10(11.0);
    return (int)(size_t)(-log_nt / std::log10(p));
}

inline double lsd_inv_ratio(double scale) { return 1.0 / scale; }

// entry i's minimum length: its own where the caller gave a list, else the detector's
inline double lsd_entry_min_length(const double* min_length, int i, double detector_min_length) {
    return min_length ? min_length[i] : detector_min_length;
}

// what stvo_lsd_create asks of an image size beyond the capacity limits (those grow with the size: a size inside a slot that was
// accepted satisfies them, std::rint being monotone)
inline bool lsd_image_size_ok(int cols, int rows, double scale) {
    return cols >= 8 && rows >= 8 && lsd_scaled_extent(cols, scale) >= 1 && lsd_scaled_extent(rows, scale) >= 1;
}

// stvo_lsd_set_image_sizes: n entries for B images in slots of slot_cols x slot_rows
inline bool lsd_image_sizes_ok(const int32_t* sizes /* [n][2] = cols, rows */, const double* min_length /* [n] or null */, int n, int B,
                               int slot_cols, int slot_rows, double scale) {
    if (!sizes || n <= 0 || n > B || B % n != 0) return false;
    for (int i = 0; i < n; ++i) {
        const int c = sizes[2 * i], r = sizes[2 * i + 1];
        if (c > slot_cols || r > slot_rows || !lsd_image_size_ok(c, r, scale)) return false;
        if (min_length && !(min_length[i] == min_length[i])) return false;  // (a NaN keeps every line and none)
    }
    return true;
}

// the row of one entry.  std::rint is monotone, so w <= the slot's scaled width and h <= its scaled height whenever cols, rows fit the slot:
// every entry's scaled image and search arrays fit what stvo_lsd_create cut for the slot (the kernels rely on it)
inline LsdSizeRow lsd_size_row(int cols, int rows, double scale, double ang_th, double min_length) {
    LsdSizeRow e;
    e.cols = cols;
    e.rows = rows;
    e.w = (int)lsd_scaled_extent(cols, scale);
    e.h = (int)lsd_scaled_extent(rows, scale);
    e.min_reg_size = lsd_min_reg_size(e.w, e.h, ang_th);
    e.pad = 0;
    e.min_length = min_length;
    return e;
}

// the two rows per entry that drive the MIXED blur and resize of orb_kernels.hip for the scaled image: the input size, then the scaled
// size with the inverse ratio on both axes
inline void lsd_scale_rows(const LsdSizeRow& e, double scale, OrbLevelSize* out /* [2] */) {
    out[0] = OrbLevelSize{e.cols, e.rows, 1.0, 1.0, 1, 0};
    out[1] = OrbLevelSize{e.w, e.h, lsd_inv_ratio(scale), lsd_inv_ratio(scale), 1, 0};
}

// stvo_lbd_set_image_sizes: the same list for the descriptor (stvo_lbd_create asks for 8 x 8)
inline bool lbd_image_sizes_ok(const int32_t* sizes, int n, int B, int slot_cols, int slot_rows) {
    if (!sizes || n <= 0 || n > B || B % n != 0) return false;
    for (int i = 0; i < n; ++i) {
        const int c = sizes[2 * i], r = sizes[2 * i + 1];
        if (c > slot_cols || r > slot_rows || c < 8 || r < 8) return false;
    }
    return true;
}

}  // namespace stvo
