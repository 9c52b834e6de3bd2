// fld_sizes.h — what one image means to the FLD kernels under a detector's parameters, host-pure (no HIP): its size, its pixels, the
// words of its edge map, the units of its counting sort and its own length threshold, stated once for stvo_fld_set_image_sizes (one
// size and threshold per image) with the functions stvo_fld_create forms the slot's own values with (frontend_layout.h: fld_words,
// fld_units, fld_store_cap).
//   What the kernels rely on.  fld_words and fld_units are monotone in npx, and npx = cols rows is monotone in either side: an image
// that fits its slot on both sides has no more pixels, edge words (the walk's LDS edge map among them) or sort units than the slot, so
// every per-image block cut for the slot holds it.
//   The store rule.  A chain of n points is written at segment slot off / (L + 1) of a store of fld_store_cap(npx, L) = npx / (L + 1)
// + 1 slots (fld_kernels.hip, frontend_layout.h).  Under a threshold per image the mapping uses the image's L_i, while the stores were
// cut for (the slot's pixels, the detector's L): an entry is taken only if fld_store_cap(npx_i, L_i) <= fld_store_cap(slot npx,
// detector's L).  L_i >= the detector's L is sufficient (npx_i <= slot npx), so a detector meant for mixed sizes is created with the
// smallest threshold it will be given.
// tests/test_fld_sizes_host.py runs this header on the host (tests/cpp/fld_sizes_host.cpp).
#pragma once
#include <cstdint>

#include "frontend_layout.h"

namespace stvo {

// One row of the detector's per-image table, entry e = row e.  32 bytes, read by a workgroup with scalar loads.
struct FldSizeRow {
    int32_t cols, rows;  // the image (top-left of its slot, whose pitch it keeps)
    int32_t npx;         // cols rows
    int32_t nw;          // fld_words(npx)
    int32_t nunits;      // fld_units(npx)
    int32_t L;           // the image's own length threshold
    int32_t pad[2];
};
static_assert(sizeof(FldSizeRow) == 32, "the kernels read a row as 32 bytes");

// One image size per image (stvo_fld_set_image_sizes) as the kernels take it: image i is sized by row i % n_sz of the table.  A kernel
// argument of its own behind the kernel's arguments, and empty for the uniform instances — they take the arguments they always took.
template <bool MIXED>
struct FldTable {};
template <>
struct FldTable<true> {
    const FldSizeRow* sz;
    int n_sz;
};

// entry i's threshold: its own where the caller gave a list, else the detector's
inline int fld_entry_threshold(const int32_t* L, int i, int L_det) { return L ? L[i] : L_det; }

inline FldSizeRow fld_size_row(int cols, int rows, int L) {
    FldSizeRow e;
    e.cols = cols;
    e.rows = rows;
    e.npx = cols * rows;
    e.nw = fld_words(e.npx);
    e.nunits = fld_units(e.npx);
    e.L = L;
    e.pad[0] = e.pad[1] = 0;
    return e;
}

enum FldSizesVerdict { FLD_SIZES_OK = 0, FLD_SIZES_INVALID = 1, FLD_SIZES_CAPACITY = 2 };

// stvo_fld_set_image_sizes: n entries for B images in slots of slot_cols x slot_rows of a detector created with threshold L_det.
// The shape of the list and every entry's size and threshold first (FLD_SIZES_INVALID), then the store rule (FLD_SIZES_CAPACITY, the
// first entry that breaks it in *entry with what it needs and what the stores hold).
inline FldSizesVerdict fld_image_sizes_verdict(const int32_t* sizes /* [n][2] = cols, rows */, const int32_t* L /* [n] or null */, int n, int B,
                                               int slot_cols, int slot_rows, int L_det, int* entry = nullptr, int* need = nullptr,
                                               int* have = nullptr) {
    if (!sizes || n < 1 || n > B || B % n != 0) return FLD_SIZES_INVALID;
    for (int i = 0; i < n; ++i) {
        const int c = sizes[2 * i], r = sizes[2 * i + 1];
        if (c > slot_cols || r > slot_rows || c < 16 || r < 16) return FLD_SIZES_INVALID;  // (16: what stvo_fld_create asks)
        if (fld_entry_threshold(L, i, L_det) < 1) return FLD_SIZES_INVALID;
    }
    const int cap = fld_store_cap(slot_cols * slot_rows, L_det);
    for (int i = 0; i < n; ++i) {
        const int want = fld_store_cap(sizes[2 * i] * sizes[2 * i + 1], fld_entry_threshold(L, i, L_det));
        if (want > cap) {
            if (entry) *entry = i;
            if (need) *need = want;
            if (have) *have = cap;
            return FLD_SIZES_CAPACITY;
        }
    }
    return FLD_SIZES_OK;
}

inline bool fld_image_sizes_ok(const int32_t* sizes, const int32_t* L, int n, int B, int slot_cols, int slot_rows, int L_det) {
    return fld_image_sizes_verdict(sizes, L, n, B, slot_cols, slot_rows, L_det) == FLD_SIZES_OK;
}

}  // namespace stvo
