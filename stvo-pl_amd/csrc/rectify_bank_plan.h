// rectify_bank_plan.h — the work split of the rectifier bank (rectify_bank.hip), stated ONCE: which (calibration, quad range, list of
// pairs) items one launch runs for an assignment of calibrations to pairs, how many there can be, and how the table the kernel reads is
// laid out.  stvo_rectify_bank_assign runs plan_rectify_bank into pinned staging and uploads the result; the kernel only reads it.
// Host-pure: g++ alone compiles it; tests/cpp/rectify_bank_plan_host.cpp runs everything here without a device.
//
// A quad is 4 consecutive output pixels of one image (the pixel index runs over rows * cols of the image's OWN size, as in the
// uniform kernel, so the resident maps of a rectifier are read as they are).  An item is one workgroup of RBANK_BLOCK threads per
// side: thread t takes quad (qblock * RBANK_BLOCK + t) of calibration `calib`, loads its maps once and walks the item's pairs
// pairs[pair_begin .. pair_begin + pair_count) with the maps in registers.  The pairs of a calibration are cut in chunks by
// rbank_chunks: enough workgroups to fill 256 CUs a few times over, at least 4 images per thread where there are.  The uniform launch
// (color_kernels.hip) cuts its n pairs by the same function, as one calibration that has them all.
#pragma once

#include <cstddef>
#include <cstdint>

namespace stvo {

constexpr int RBANK_BLOCK = 256;  // threads of a workgroup = quads of an item

struct RectBankItem {
    int32_t calib;       // calibration of every pair of the item
    int32_t qblock;      // quads [qblock * RBANK_BLOCK, (qblock + 1) * RBANK_BLOCK) of that calibration's images
    int32_t pair_begin;  // into the pair list
    int32_t pair_count;  // >= 1
};
static_assert(sizeof(RectBankItem) == 16, "the kernel reads an item as 16 bytes");

inline int rbank_nquads(int cols, int rows) { return (int)(((size_t)cols * (size_t)rows + 3) / 4); }
inline int rbank_qblocks(int cols, int rows) { return (rbank_nquads(cols, rows) + RBANK_BLOCK - 1) / RBANK_BLOCK; }

// chunks the m pairs of a calibration with `qblocks` quad blocks are cut in (m >= 1), and the pairs of every chunk but the last
inline int rbank_chunks(int qblocks, int m, int* per_chunk) {
    const int want = (256 * 8 + 2 * qblocks - 1) / (2 * qblocks);  // (>= 1 for every qblocks >= 1: no max(1, want))
    int chunks = (m + 3) / 4;
    if (chunks > want) chunks = want;
    if (chunks < 1) chunks = 1;
    *per_chunk = (m + chunks - 1) / chunks;
    return (m + *per_chunk - 1) / *per_chunk;
}

// The most items any assignment of B pairs to K calibrations no larger than the slot yields: a calibration with m >= 1 pairs has at most
// (m + 3) / 4 chunks of at most the slot's quad blocks each, and at most min(K, B) calibrations have a pair.
inline size_t rbank_max_items(int B, int K, int slot_cols, int slot_rows) {
    const int used = K < B ? K : B;
    return (size_t)rbank_qblocks(slot_cols, slot_rows) * (size_t)((B + 3 * used) / 4);
}

// The table of one assignment, device memory and its pinned staging alike: [B] pair list (the pairs of calibration 0 first, each
// calibration's in ascending order), then the items from a 16-byte-aligned offset.
inline size_t rbank_items_offset(int B) { return ((size_t)B * sizeof(int32_t) + 15) & ~size_t(15); }
inline size_t rbank_table_bytes(int B, size_t n_items) { return rbank_items_offset(B) + n_items * sizeof(RectBankItem); }

// calib_of_pair [B] in 0 .. K - 1 (the caller has checked), cols / rows [K] the calibrations' sizes.  Writes the pair list and at most
// max_items items; returns the number of items, or -1 when they would not fit (never, for max_items = rbank_max_items).
inline int plan_rectify_bank(int B, int K, const int32_t* calib_of_pair, const int32_t* cols, const int32_t* rows, int32_t* pairs,
                             RectBankItem* items, size_t max_items) {
    size_t n_items = 0;
    int filled = 0;
    for (int k = 0; k < K; ++k) {
        const int begin = filled;
        for (int b = 0; b < B; ++b)
            if (calib_of_pair[b] == k) pairs[filled++] = b;
        const int m = filled - begin;
        if (m == 0) continue;  // a calibration without pairs runs nothing
        const int qblocks = rbank_qblocks(cols[k], rows[k]);
        int per_chunk = 0;
        const int chunks = rbank_chunks(qblocks, m, &per_chunk);
        for (int c = 0; c < chunks; ++c) {
            const int p0 = c * per_chunk, p1 = p0 + per_chunk < m ? p0 + per_chunk : m;
            for (int q = 0; q < qblocks; ++q) {
                if (n_items >= max_items) return -1;
                items[n_items++] = RectBankItem{k, q, begin + p0, p1 - p0};
            }
        }
    }
    return (int)n_items;
}

}  // namespace stvo
