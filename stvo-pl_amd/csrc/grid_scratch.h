// grid_scratch.h — the scratch of the K3 stereo grid matchers (grid_kernels.hip), stated ONCE: which arrays a match works in, how many
// elements each holds for a problem of (B, rows1, rows2), and how an owner cuts them from its allocation.  The pipeline (seq_state.h)
// carves one for the key-points and one for the key-lines; the C-ABI calls (run_grid) take the same counts to the context's arena.
// Host-pure: g++ alone compiles it; tests/cpp/grid_scratch_host.cpp runs everything here without a device.
#pragma once

#include <cstddef>
#include <cstdint>

#include "carver.h"

namespace stvo {

constexpr int GRID_ELIG = 16;  // eligible pairs a right feature keeps from scan pass 1

// rows1 / rows2: rows per frame of the left / right feature arrays.
struct GridScratch {
    unsigned long long* cover;  // [B][words64][n1p] candidate bit-matrix, or nullptr: the caller's route never reads one (range form)
    unsigned long long* top2;   // [B][rows1] low word: best eligible key (d << 16 | i2), high word: blocked flag
    int32_t* owner2;            // [B][rows2]
    // the single-scan formulation (mutual != 0): the ELIGIBLE (left feature, distance) pairs every right feature met in scan pass 1 —
    // elig == nullptr: two full scan passes
    uint32_t* elig;             // [B][GRID_ELIG][rows2]  (i1 << 16 | d), slot-major
    int32_t* elig_cnt;          // [B][rows2]
    int32_t* ovf;               // [B] set when some right feature of the frame met more than GRID_ELIG eligible pairs
    // [B] or nullptr: written by the one-workgroup-per-frame point matcher (1: frame left to the scan formulation).  ONE buffer with
    // ovf, misfit == ovf + B: stvo_seq_debug_point_route reads both in one copy of grid_route_words(B) words from ovf.
    int32_t* misfit;
};
inline size_t grid_route_words(int B) { return (size_t)2 * (size_t)B; }

// The bit-matrix of one frame: words64 rows (one per 64 scan positions of right features) of n1p masks (one per left feature, rounded
// up to the scan's block of 64).
struct GridMatrixDims {
    int words64, n1p;
    size_t words() const { return (size_t)words64 * (size_t)n1p; }
};
inline GridMatrixDims grid_matrix_dims(int rows1, int rows2) { return GridMatrixDims{(rows2 + 63) / 64, (rows1 + 63) & ~63}; }

// elements of every array (cover: 0 without a bit-matrix; ovf: B words, 2 B with misfit behind them)
struct GridScratchCounts {
    size_t cover, top2, owner2, elig, elig_cnt, ovf;
};
inline GridScratchCounts grid_scratch_counts(int B, int rows1, int rows2, bool with_bit_matrix, bool with_misfit) {
    const size_t nb = (size_t)B, n1 = nb * (size_t)rows1, n2 = nb * (size_t)rows2;
    return GridScratchCounts{with_bit_matrix ? nb * grid_matrix_dims(rows1, rows2).words() : 0, n1, n2, n2 * GRID_ELIG, n2,
                             with_misfit ? grid_route_words(B) : nb};
}

// Cuts the arrays in the order of the struct.  The pipeline's allocation keeps the key-lines' eligible-pair arrays in front of its
// fetch block and their other arrays behind it, so a carve may be made in two halves (`parts`); a half leaves the other's pointers alone.
enum GridScratchParts { GRID_SCRATCH_ROWS = 1, GRID_SCRATCH_ELIG = 2, GRID_SCRATCH_ALL = 3 };  // cover / top2 / owner2; elig / elig_cnt / ovf + misfit
inline void carve_grid_scratch(Carver& c, GridScratch& g, int B, int rows1, int rows2, bool with_bit_matrix, bool with_misfit,
                               int parts = GRID_SCRATCH_ALL) {
    const GridScratchCounts n = grid_scratch_counts(B, rows1, rows2, with_bit_matrix, with_misfit);
    if (parts & GRID_SCRATCH_ROWS) {
        g.cover = with_bit_matrix ? c.take<unsigned long long>(n.cover) : nullptr;
        g.top2 = c.take<unsigned long long>(n.top2);
        g.owner2 = c.take<int32_t>(n.owner2);
    }
    if (parts & GRID_SCRATCH_ELIG) {
        g.elig = c.take<uint32_t>(n.elig);
        g.elig_cnt = c.take<int32_t>(n.elig_cnt);
        g.ovf = c.take<int32_t>(n.ovf);
        g.misfit = with_misfit ? g.ovf + B : nullptr;
    }
}

}  // namespace stvo
