// match_mfma.hip — K1m `hamming_knn2_mfma`: the brute-force Hamming 2-NN scan of K1 (match_kernels.hip) with the
// 256-bit distances taken from the gfx950 matrix cores instead of 8 x (v_xor + v_bcnt) per pair.
//
// Same contract as hamming_knn2_kernel — cv::BFMatcher(NORM_HAMMING).knnMatch(desc1, desc2, ., 2) as called from
// StVO::matchNNR (/root/reference/src/matching.cpp:47-48): per query row the two smallest distances in ascending
// order, lowest train index first among equal distances — and the same output ([nseg][B][row_stride] packed keys).
//
// Why this is a matrix product and not a reshaping trick: the all-pairs Hamming distance of bit rows IS a Gram
// matrix.  With bits mapped to x = -+a (query: -a for a set bit) and y = +-a (train: +a for a set bit),
//       sum_k x_k * y_k = a^2 * (#differing - #equal) = 2 a^2 * h - 256 a^2.
// Operands are FP4 (e2m1) on gfx950's block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (round 4; rounds 1-3 used i8 on
// v_mfma_i32_32x32x32_i8): +-4 is an e2m1 value (0b0110 / 0b1110), so a bit becomes a NIBBLE and a 256-bit row four K = 64
// steps, each as long as one of the eight i8 steps it replaces — the matrix pipe needs half the time per tile
// (tools/fp4_probe.hip on MI355X: 151 cycles per 32 x 32 tile of 256-bit distances against 265 - 330 for i8, 16 - 17 T pairs/s
// register-only against 9 - 10; the probe also checks the operand convention used here against a CPU product, entry for
// entry).  With both block scales at 2^4, a = 64 and the f32 accumulator holds 8192 h - 2^20 exactly; the C operand of a
// tile's first matrix instruction carries the (tile-relative) train index, so the accumulator leaves the matrix pipe already
// as the packed key 8192 h + j - 2^20 (|key| < 2^22 after every rebasing: exact in f32) whose order is the (distance, train
// index) order knnMatch uses.  The VALU work per (query, train) pair drops from 16 + ~2 ops (K1) to 2: v_med3_f32 + v_min_f32.
//
// Mapping (wave64, 32x32 tiles):
//   * MFMA "A" operand = 32 TRAIN rows, expanded from bits to nibbles once per workgroup into LDS (4 KB per tile, 2 MF_TPB
//     buffers, one barrier per MF_TPB tiles) and read back as ready-made fragments (one contiguous ds_read_b128 per K step);
//   * MFMA "B" operand = 32 QUERY rows per block, expanded once and kept in VGPRs for the whole scan (16 per block;
//     QB blocks per wave -> every train fragment read from LDS feeds QB matrix instructions);
//   * D[train][query]: a lane owns ONE query column and 16 train rows of the tile, so the running (best, second)
//     of a query is two VGPRs per lane and the final cross-lane merge is a single swap of the wave halves.
//   * bit -> K element mapping: K step kk covers descriptor words 2 kk (lower wave half) and 2 kk + 1 (upper); dword d of a
//     lane's fragment holds bits d, d + 4, ..., d + 28 of its word as nibbles: ((w << (3 - d)) & 0x88888888) | 0x66666666 —
//     and + shift-or per eight elements in the forward scan (expand_fp4_lshl_or).  Any mapping works as long as both operands use the same one (a sum over k).
//   * the tile loop of the forward scan exists in two forms: the GENERAL barrier group (any tile count, conditional fetch and staging, the
//     first group and the last two or three of a segment) and the STEADY loop between them (all tiles it touches are full: nothing
//     conditional, two groups per turn).  One-op nibble codes that leave a bit where it is in its nibble (0 / 0.5, 0 / 1, 0 / 2, +1 / -1
//     against query magnitudes 4, 2, 1, 1, scales 2^6, a per-query constant 4096 (192 - 2 popcount(q & 0x77..7)) in every key) were built
//     and are exact on the hardware, but measured slower, not faster: NOTES.md, profiles/k1m_codes_ab.json.
#include <type_traits>

#include "kernels.h"

namespace stvo {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

#ifndef MF_TPB
#define MF_TPB 2  // train tiles per workgroup barrier
#endif
#ifndef MF_FOLD_SLOTS
#define MF_FOLD_SLOTS 5  // vector instructions scheduled behind each matrix instruction of the forward scan
#endif
constexpr int MF_BLOCK = 256;        // 4 waves
constexpr int MF_TILE = 32;          // train rows per tile
constexpr int MF_KEY_SHIFT = 13;     // key = (h << 13) + j - MF_KEY_BIAS, j < 8192
constexpr int MF_KEY_BIAS = 1 << 20;
constexpr int MF_NO_KEY = 0x7FFFFFFF;
constexpr int MF_NO_KEY_MIN = 0x40000000;  // the sentinel after any number of per-tile rebasings (<= 256 x 32)

// FP4: the 32 bits of a descriptor word as 32 e2m1 nibbles, 0b0110 (+4) for a clear bit, 0b1110 (-4) for a set one
__device__ __forceinline__ v4i expand_fp4(uint32_t w) {
    v4i r;
    r.x = (int)(((w << 3) & 0x88888888u) | 0x66666666u);
    r.y = (int)(((w << 2) & 0x88888888u) | 0x66666666u);
    r.z = (int)(((w << 1) & 0x88888888u) | 0x66666666u);
    r.w = (int)((w & 0x88888888u) | 0x66666666u);
    return r;
}
// The same nibbles for the forward scan's tile loop, where every vector operation counts: written as above the compiler emits
// shift + and + or per dword (11 operations; gfx950's VOP3 takes no literal, so no v_and_or_b32 forms).  Masking FIRST leaves
// (w & (0x11111111 << d)) << (3 - d) | 0x66666666 = one v_and_b32 with a literal and one v_lshl_or_b32 whose shift is an inline
// constant and whose third operand is a scalar register: 8 operations.
__device__ __forceinline__ v4i expand_fp4_lshl_or(uint32_t w) {
    const uint32_t base = 0x66666666u;
    v4i r;
    asm("v_lshl_or_b32 %0, %1, 3, %2" : "=v"(r.x) : "v"(w & 0x11111111u), "s"(base));
    asm("v_lshl_or_b32 %0, %1, 2, %2" : "=v"(r.y) : "v"(w & 0x22222222u), "s"(base));
    asm("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(r.z) : "v"(w & 0x44444444u), "s"(base));
    r.w = (int)((w & 0x88888888u) | base);
    return r;
}
__device__ __forceinline__ float med3_f32(float a, float b, float c) {
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float min_f32(float a, float b) {  // (no canonicalisation of the operands: they are exact integers)
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float max_f32(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float min3_f32(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
constexpr float MF_NO_KEY_F = 1.0e30f;      // the float form's sentinel: rebasing by -32 / -64 never changes it
constexpr float MF_NO_KEY_MIN_F = 1.0e29f;
constexpr int MF_SCALE_2_4 = 127 + 4;       // E8M0 block scale 2^4 on both operands: (+-4 * 16)^2 = 4096

// tile-relative key -> K1's (distance << 16) | train index; base = first train row of the tile the key is relative to
__device__ __forceinline__ uint32_t key_to_knn(int key, int base) {
    if (key >= MF_NO_KEY_MIN) return 0xFFFFFFFFu;
    const uint32_t u = (uint32_t)(key + base + MF_KEY_BIAS);
    return ((u >> MF_KEY_SHIFT) << 16) | (u & ((1u << MF_KEY_SHIFT) - 1u));
}

// Every row of the direction's query side against every row of its train side.
template <int QB, int MODE>
__global__ __launch_bounds__(MF_BLOCK, (QB == 1 ? 4 : QB == 2 ? 3 : 1)) void hamming_knn2_mfma_kernel(int B, int tiles, int ndir, int dir0, int nseg, int row_stride,
                                                                      const uint8_t* __restrict__ d1,
                                                                      const int32_t* __restrict__ n1,
                                                                      const uint8_t* __restrict__ d2,
                                                                      const int32_t* __restrict__ n2,
                                                                      uint2* __restrict__ knn12, uint2* __restrict__ knn21,
                                                                      uint32_t* __restrict__ claim_init) {
    // the second template argument is part of the name traces and the committed counter files know this kernel by (<QB, 0>)
    static_assert(MODE == 0, "only the forward scan exists");
    constexpr int ROWS = 4 * QB * 32;  // query rows per workgroup
    constexpr int KSTEPS = 4;  // matrix instructions (K = 64) per 32 x 32 tile of 256-bit distances
    using key_t = float;
    using acc_t = v16f;
    // one 16-byte fragment per (K step, wave half, train row): [tile parity][(kk * 2 + hf) * 32 + train row]
    constexpr int NBUF = 2 * MF_TPB;
    __shared__ v4i s_tile[NBUF][KSTEPS * 2 * 32];
    // XCD-aware block -> (frame pair, direction, tile, segment) mapping: as hamming_knn2_kernel
    const int per_frame = tiles * ndir * nseg;
    const int L = blockIdx.x;
    const int xcd = L & 7, k = L >> 3;
    int fb = k / per_frame, local = k % per_frame;
    // Forward scan, which workgroup takes which query tile — decided from the frame's OWN row count, the host knows none:
    // a frame has tiles - 1 slots in the MAIN section of the launch and one in the END section (all frames' end slots behind
    // all main slots).  With full = nq / ROWS, main slot j takes tile j if j < min(full, tiles - 1) and leaves otherwise; the
    // end slot takes tile min(full, tiles - 1) if it has rows: the ragged tile, or the last full one of a frame that fills its
    // capacity.  The main section then holds full tiles only and the launch ends on the short workgroups at every capacity and
    // row count (1647 rows in slots of 2048: main slots 0 - 5 scan, slot 6 leaves, the end slot scans the 111 rows of tile 6).
    const bool remap = ndir == 1 && tiles > 1;
    bool end_slot = false;
    if (remap) {
        const int groups = (int)(gridDim.x >> 3) / per_frame;  // frames per XCD
        const int full_pf = (tiles - 1) * nseg, full = full_pf * groups;
        if (k < full) {
            fb = k / full_pf;
            local = k % full_pf;
        } else {
            fb = (k - full) / nseg;
            local = full_pf + (k - full) % nseg;
            end_slot = true;
        }
    }
    const int b = fb * 8 + xcd;
    if (b >= B) return;
    const int seg = local % nseg;
    const int dir = dir0 + (local / nseg) / tiles;
    const int slot = (local / nseg) % tiles;
    const size_t frame_off = (size_t)b * row_stride;
    // (the wave's number as a scalar: what is derived from it — its first row, wave_active — holds no vector register through the scan)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, hf = lane >> 5;
    const uint32_t* __restrict__ Q = reinterpret_cast<const uint32_t*>((dir == 0 ? d1 : d2) + frame_off * STVO_DESC_BYTES);
    // A slot that knows its tile before the counts arrive fetches its query rows while n1 / n2 are still on their way (rows
    // past the count are inside the frame's slot, are scanned like any other row and never stored).  An end slot learns its
    // tile from the count and fetches behind it; one that leaves requests nothing.
    uint4 qw[QB][2];
    if (!end_slot) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int qi = min(slot * ROWS + (wv * QB + qb) * 32 + col, row_stride - 1);
            qw[qb][0] = reinterpret_cast<const uint4*>(Q)[2 * qi];
            qw[qb][1] = reinterpret_cast<const uint4*>(Q)[2 * qi + 1];
        }
    }
    const int na = n1[b], nb = n2[b];
    const int nq = dir == 0 ? na : nb;
    const int nt_all = dir == 0 ? nb : na;
    const int seg_len = (((nt_all + nseg - 1) / nseg) + MF_TILE - 1) & ~(MF_TILE - 1);
    const int j0 = min(seg * seg_len, nt_all);
    const int nt = min(j0 + seg_len, nt_all);
    if (claim_init && seg == 0 && dir == dir0)  // (by SLOT: rows 0 .. row_stride - 1 exactly once per frame, whichever tile the slot scans)
        for (int c = slot * ROWS + tid; c < min((slot + 1) * ROWS, row_stride); c += MF_BLOCK) claim_init[frame_off + c] = 0xFFFFFFFFu;
    int tile = slot;
    if (remap) {
        const int last = min(nq / ROWS, tiles - 1);
        if (end_slot) tile = last;
        else if (slot >= last) return;  // workgroup-uniform
    }
    const int q_base = tile * ROWS;
    if (q_base >= nq) return;  // workgroup-uniform
    const uint32_t* __restrict__ T = reinterpret_cast<const uint32_t*>((dir == 0 ? d2 : d1) + frame_off * STVO_DESC_BYTES);
    uint2* __restrict__ out = (dir == 0 ? knn12 : knn21) + (size_t)seg * B * row_stride + frame_off;

    // A tile of at most ROWS / 2 rows (workgroup-uniform; under the remap only an end slot's) is scanned with ONE block per wave,
    // rows q_base + 32 wv + col: all four waves work instead of two of them holding their registers idle through the scan.
    const bool one_block = QB == 2 && nq - q_base <= ROWS / 2;
    auto block_row = [&](int qb) { return q_base + (one_block ? wv : wv * QB + qb) * 32 + col; };
    // query fragments: block qb of this wave, kept for the whole scan
    const bool wave_active = block_row(0) - col < nq;
    v4i qf[QB][KSTEPS];
    auto query_row = [&](int qb) {  // recomputed for the final store rather than kept live across the scan
        const int q = block_row(qb);
        return q < nq ? q : nq - 1;  // tail lanes scan a valid row and discard the result
    };
    if (end_slot || one_block) {  // (the early fetch of a one-block tile outside the remap took the two-block rows)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int qi = query_row(qb);
            qw[qb][0] = reinterpret_cast<const uint4*>(Q)[2 * qi];
            qw[qb][1] = reinterpret_cast<const uint4*>(Q)[2 * qi + 1];
        }
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const uint32_t w[8] = {qw[qb][0].x, qw[qb][0].y, qw[qb][0].z, qw[qb][0].w, qw[qb][1].x, qw[qb][1].y, qw[qb][1].z, qw[qb][1].w};
        // K step kk covers words 2 kk and 2 kk + 1: the lower wave half takes the first, the upper the second
        const bool up = hf != 0;  // (selects, not an indexed array: that one went through scratch)
        qf[qb][0] = expand_fp4(~(up ? w[1] : w[0]));
        qf[qb][1] = expand_fp4(~(up ? w[3] : w[2]));
        qf[qb][2] = expand_fp4(~(up ? w[5] : w[4]));
        qf[qb][3] = expand_fp4(~(up ? w[7] : w[6]));
    }
    // The train index enters through the C operand of the first matrix instruction of a tile: accumulator register r of
    // this lane belongs to tile row (r & 3) + 8 (r >> 2) + 4 hf.  Keys are therefore relative to the first row of their PAIR
    // of tiles (the second tile of a pair takes cidx + 32) and the running (best, second) are rebased by -64 per pair: 1 VALU
    // op per tile and query block instead of a ninth matrix instruction per block (16 more registers: 168, the cap of three
    // waves per SIMD, no scratch).
    acc_t cidx;
#pragma unroll
    for (int r = 0; r < 16; ++r) cidx[r] = (key_t)((r & 3) + 8 * (r >> 2) + 4 * hf);
    acc_t cidx2 = cidx + (key_t)MF_TILE;  // the second tile of a pair

    const key_t no_key = MF_NO_KEY_F;
    key_t best[QB], second[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) best[qb] = second[qb] = no_key;

    // staging role of this thread: word xk of train row xr of the tile
    const int xr = tid & 31, xk = tid >> 5;
    const int ntiles = (nt - j0 + MF_TILE - 1) / MF_TILE;
    // A thread's word of tile t lies t KB behind its word of tile 0: a 32-bit byte offset against the frame's (scalar) base, one
    // addition per fetch; only the segment's last tile can hold rows past its end, and only there a lane tests its row.
    const uint32_t voff0 = (uint32_t)((j0 + xr) * 8 + xk) * 4u;
    const int nfull = (nt - j0) / MF_TILE;
    auto fetch = [&](int t) -> uint32_t {
        const int j = j0 + t * MF_TILE + xr;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(T) + (voff0 + (uint32_t)t * (MF_TILE * STVO_DESC_BYTES)));
        if (t < nfull) return *p;
        return j < nt ? *p : 0u;
    };
    auto stage = [&](int t, uint32_t w) {
        s_tile[t & (NBUF - 1)][xk * 32 + xr] = expand_fp4_lshl_or(w);  // word xk = K step xk / 2, wave half xk & 1
    };
#pragma unroll
    for (int i = 0; i < MF_TPB; ++i)
        if (i < ntiles) stage(i, fetch(i));
    __syncthreads();
    // Software pipeline, depth one tile: step t issues the matrix instructions of tile t and, in their shadow, folds the
    // accumulators of tile t - 1 into (best, second) — a v_mfma occupies the matrix pipe for 8 passes while the wave's
    // VALU slots stay free.  Only the last tile of a segment can be ragged and it is folded after the loop (masked).
    auto rebase = [&](int nb) {  // (best, second) relative to the next PAIR of tiles; the no-key sentinel stays far above any key
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
            if (qb < nb) {
                best[qb] -= (key_t)(2 * MF_TILE);
                second[qb] -= (key_t)(2 * MF_TILE);
            }
    };
    auto fold = [&](int qb, key_t key) {
        second[qb] = med3_f32(best[qb], second[qb], key);
        best[qb] = min_f32(best[qb], key);
    };
    auto mma = [&](const v4i& tf, const v4i& q, const acc_t& c) -> acc_t {
        const v8i a8 = {tf.x, tf.y, tf.z, tf.w, 0, 0, 0, 0}, b8 = {q.x, q.y, q.z, q.w, 0, 0, 0, 0};  // (FP4 reads four dwords)
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, MF_SCALE_2_4, 0, MF_SCALE_2_4);
    };
    // NB blocks of this wave take part: QB, or 1 in the one-block form of a small tile — a compile-time constant per copy of the
    // scan (below), so that either copy is straight-line code for the instruction groups at the end of a K step.
    // FOLD: 0 = the first tile of a scan (nothing to fold yet), 1 = the tile behind it, 2 = every later tile.
    // ODD: the second tile of a pair — its keys are relative to the pair's first row (C operand cidx + 32), and in front of its folds,
    // which take the pair's first tile, (best, second) move from the previous pair's frame to this one.
    // KNOWN: the caller has tested wave_active already (the steady loop: once, in front of the loop).
    auto mma_fold = [&](auto known_c, auto nb_c, auto fold_c, auto odd_c, acc_t (&cur)[QB], acc_t (&prev)[QB], int t) {
        constexpr int NB = decltype(nb_c)::value, FOLD = decltype(fold_c)::value;
        constexpr bool ODD = decltype(odd_c)::value, KNOWN = decltype(known_c)::value;
        constexpr bool fold_prev = FOLD > 0;  // tile t - 1 is a full tile here
        if (KNOWN || wave_active) {
            const v4i* frag = s_tile[t & (NBUF - 1)];
            if (ODD && FOLD == 2) rebase(NB);  // (in the first pair they hold no key yet)
            key_t node[NB][5];
            v4i tf = frag[lane];
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                v4i tf_ahead = tf;
                if (kk < KSTEPS - 1) tf_ahead = frag[(kk + 1) * 64 + lane];  // one K step ahead of its use
#pragma unroll
                for (int qb = 0; qb < NB; ++qb) cur[qb] = mma(tf, qf[qb][kk], kk == 0 ? (ODD ? cidx2 : cidx) : cur[qb]);
                if (fold_prev) {
                    // The fold as a TOURNAMENT of three-input nodes (round 5, last change).  The 16 keys of the previous tile and the
                    // running best are the 17 leaves of a tree of eight nodes; a node forms the smallest of its three inputs (v_min3,
                    // passed up) and their median (v_med3).  The root's minimum is the new best, and the new second is the smallest of
                    // the old second and the eight medians: a median is the minimum of a subtree that does not hold the overall
                    // minimum, so none is below the true second; and the true second — the smallest key that lost DIRECTLY to the
                    // winner, or the old second — is among them.  16 + 4 operations per block and tile instead of the 27 of merging
                    // three keys at a time into the pair (5 per 3 keys); the kernel is bound by vector + matrix ISSUE (rocprofv3:
                    // SQ_ACTIVE_INST_ANY of the three waves of a SIMD = 1.08 of a wave's life) and the fold is most of its vector work.
                    // The previous tile's 16 accumulator registers per block are complete, so their order is free: five operations
                    // behind each of the four matrix instructions of a block.
                    // HAZARD (tools/mfma_hazard_check.py, run by tests/test_isa_mfma_hazard.py on every build): these reads
                    // are inline asm, so the compiler inserts none of the 12 wait states an 8-pass XDL write needs before a vector read
                    // of its destination.  With QB >= 2 the distance is structural — behind the last matrix instruction of a block's
                    // previous tile come its share of the fold, the other blocks' matrix instructions and folds, the rebasing and this
                    // tile's first matrix instruction (>= 14 counted conservatively; the ISA check fails the CPU suite below 12).  With one
                    // block per wave (the one-block form of a small tile, and the developer switch) only five fold operations and the
                    // rebasing lie between: an explicit fence, tied to the registers, as in the reverse kernel.  The same fence stands in
                    // the SECOND tile of a scan: the first one folds nothing, its matrix instructions stand back to back.
                    if ((NB == 1 || FOLD == 1) && kk == 0) {
                        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 2" : "+v"(prev[0]));
#pragma unroll
                        for (int qb = 1; qb < NB; ++qb) asm volatile("" : "+v"(prev[qb]));  // (behind the fence: volatile asm keeps its order)
                    }
                    // In the steady loop two tiles share a basic block, and nothing but data keeps this tile's folds behind its first
                    // matrix instruction, which the structural distance above counts on (without the tie the scheduler drew five of
                    // them in front of it: 12 wait states, no margin).  Tie the previous tile's registers to that instruction's
                    // result: no instruction, no register (21 wait states).
                    if (KNOWN && kk == 0) {
#pragma unroll
                        for (int qb = 0; qb < NB; ++qb) asm("" : "+v"(prev[qb]) : "v"(cur[0]));
                    }
#pragma unroll
                    for (int qb = 0; qb < NB; ++qb) {
                        const acc_t& p = prev[qb];
                        key_t(&a)[5] = node[qb];
                        if (kk == 0) {
                            a[0] = min3_f32(p[0], p[1], p[2]);
                            a[1] = min3_f32(p[3], p[4], p[5]);
                            second[qb] = min3_f32(second[qb], med3_f32(p[0], p[1], p[2]), med3_f32(p[3], p[4], p[5]));
                        } else if (kk == 1) {
                            a[2] = min3_f32(p[6], p[7], p[8]);
                            a[3] = min3_f32(p[9], p[10], p[11]);
                            second[qb] = min3_f32(second[qb], med3_f32(p[6], p[7], p[8]), med3_f32(p[9], p[10], p[11]));
                        } else if (kk == 2) {
                            a[4] = min3_f32(p[12], p[13], p[14]);
                            const key_t b0 = min3_f32(a[0], a[1], a[2]);
                            second[qb] = min3_f32(second[qb], med3_f32(p[12], p[13], p[14]), med3_f32(a[0], a[1], a[2]));
                            a[0] = b0;
                        } else {
                            const key_t b1 = min3_f32(a[3], a[4], p[15]), n1 = med3_f32(a[3], a[4], p[15]);
                            second[qb] = min3_f32(second[qb], n1, med3_f32(a[0], b1, best[qb]));
                            best[qb] = min3_f32(a[0], b1, best[qb]);
                        }
                    }
                }
                if (kk < KSTEPS - 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // 1 LDS read (the next step's fragment)
#pragma unroll
                for (int qb = 0; qb < NB; ++qb) {  // (one instruction, then its share of the fold: with FP4 operands a matrix instruction
                                                   //  lasts about as long as the 8 fold operations of one block take to issue — 0.418 ->
                                                   //  0.401 ms per 1024 frames against QB instructions followed by all of the fold)
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         // one matrix instruction
                    __builtin_amdgcn_sched_group_barrier(0x002, MF_FOLD_SLOTS, 0);             // its shadow: a block's share of the fold (20 ops + rebasing)
                }
                tf = tf_ahead;
            }
            // A tile is a scheduling region of its own: the instruction groups above hold only as long as no fold of the NEXT tile (an
            // inline-asm read of the accumulators written just above) can be drawn into this tile's slots when two tiles share a basic block.
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    acc_t accA[QB], accB[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int r = 0; r < 16; ++r) accA[qb][r] = accB[qb][r] = 0;
    // MF_TPB tiles per workgroup barrier: while tiles t .. t + MF_TPB - 1 are multiplied (2 MF_TPB LDS buffers), the next MF_TPB are
    // fetched and staged.  With FP4 operands a tile is short (4 matrix instructions per block) and the four waves of a workgroup
    // met at a barrier every ~400 cycles: two tiles per barrier 0.402 -> 0.364 ms per 1024 frames.
    static_assert(MF_TPB % 2 == 0, "the accumulator sets alternate tile by tile");
    int t = 0;
    // the train words travel TWO barrier groups ahead of their tiles (registers only: the LDS buffers are staged as before; round 5:
    // 0.3256 -> 0.3227 ms per 1024 frames).  What else round 5 measured on this loop, all without effect or worse: LDS reads truly one K
    // step ahead (lgkmcnt(1) instead of (0) in front of every pair of matrix instructions): no change; no barrier: no change; no fetch /
    // stage / barrier at all: 0.289; (almost) no fold: 0.273 — the matrix pipe's own 0.17 is not within reach of this skeleton; workgroups
    // persistent over the query tiles of a frame, next tile's rows requested under the drain: 0.40 (168 VGPRs, address reloads in the loop),
    // and as slow with ONE tile per workgroup, i.e. the per-workgroup prologue is not what is missing either.
    uint32_t w_near[MF_TPB];
#pragma unroll
    for (int i = 0; i < MF_TPB; ++i) {
        w_near[i] = 0;
        if (MF_TPB + i < ntiles) w_near[i] = fetch(MF_TPB + i);
    }
    // The scan exists twice, chosen per workgroup: QB blocks per wave, and ONE block per wave for a tile of at most ROWS / 2 rows.
    // Both copies carry the same state through the loop (the one-block copy leaves the second block's registers alone).
    auto scan = [&](auto nb_c) {
        constexpr int NB = decltype(nb_c)::value;
        auto group = [&](auto first_c) {  // MF_TPB tiles between two workgroup barriers; `first`: tiles 0 .. MF_TPB - 1
            constexpr bool FIRST = decltype(first_c)::value;
            uint32_t w_far[MF_TPB];
#pragma unroll
            for (int i = 0; i < MF_TPB; ++i) {
                w_far[i] = 0;
                if (t + 2 * MF_TPB + i < ntiles) w_far[i] = fetch(t + 2 * MF_TPB + i);
            }
            static_assert(MF_TPB == 2, "the accumulator sets alternate tile by tile, two tiles per group");
            mma_fold(std::false_type{}, nb_c, std::integral_constant<int, (FIRST ? 0 : 2)>{}, std::false_type{}, accA, accB, t);
            mma_fold(std::false_type{}, nb_c, std::integral_constant<int, (FIRST ? 1 : 2)>{}, std::true_type{}, accB, accA, t + 1);
#pragma unroll
            for (int i = 0; i < MF_TPB; ++i) {
                if (t + MF_TPB + i < ntiles) stage(t + MF_TPB + i, w_near[i]);
                w_near[i] = w_far[i];
            }
            __syncthreads();
            t += MF_TPB;
        };
        // The STEADY group: tiles t .. t + 3 MF_TPB - 1 are all full tiles of the segment, so the fetch two groups ahead and the
        // staging one group ahead are unconditional and no lane tests its row: the conditions of the general group are false only
        // in a segment's last groups, yet cost it ~45 scalar and branch instructions every time (1647 train rows: 22 of the 26
        // groups run here; K1m 988 -> 941 us at 3072 frames, profiles/k1m_codes_ab.json).  `near` / `far` trade places from one
        // group to the next — the loop holds two groups, no move carries the words.  Only a wave that multiplies comes here
        // (tested once, in front of the loop); an idle wave of a two-block tile stays with the general group, which stages the
        // same tiles and meets the others at the same barrier, one per group.
        auto steady_group = [&](uint32_t (&near)[MF_TPB], uint32_t (&far)[MF_TPB]) {
#pragma unroll
            for (int i = 0; i < MF_TPB; ++i)
                far[i] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(T) +
                                                            (voff0 + (uint32_t)(t + 2 * MF_TPB + i) * (MF_TILE * STVO_DESC_BYTES)));
            mma_fold(std::true_type{}, nb_c, std::integral_constant<int, 2>{}, std::false_type{}, accA, accB, t);
            mma_fold(std::true_type{}, nb_c, std::integral_constant<int, 2>{}, std::true_type{}, accB, accA, t + 1);
#pragma unroll
            for (int i = 0; i < MF_TPB; ++i) stage(t + MF_TPB + i, near[i]);
            __syncthreads();
            t += MF_TPB;
        };
        if (MF_TPB <= ntiles) group(std::true_type{});
        // (the one-block form of a small tile keeps the general group only; wave_active is wave-uniform and constant over the scan)
        if (NB == QB && wave_active) {
            uint32_t w_other[MF_TPB];
            while (t + 4 * MF_TPB <= nfull) {  // two groups per turn: the second one fetches tiles t + 3 MF_TPB .. t + 4 MF_TPB - 1
                steady_group(w_near, w_other);
                steady_group(w_other, w_near);
            }
        }
        while (t + MF_TPB <= ntiles) group(std::false_type{});  // the segment's last two or three groups
        if (t < ntiles) {  // its tile is staged already (t is even here)
            if (t == 0) mma_fold(std::false_type{}, nb_c, std::integral_constant<int, 0>{}, std::false_type{}, accA, accB, t);
            else mma_fold(std::false_type{}, nb_c, std::integral_constant<int, 2>{}, std::false_type{}, accA, accB, t);
        }
        if (wave_active && ntiles > 0) {  // drain: the last tile, rows past the segment end carry no key
            const int jt = j0 + (ntiles - 1) * MF_TILE;
            const acc_t(&last)[QB] = (ntiles & 1) ? accA : accB;
            if (ntiles & 1) rebase(NB);  // (the last tile opens a pair of its own)
#pragma unroll
            for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int jr = jt + (r & 3) + 8 * (r >> 2) + 4 * hf;
                    fold(qb, jr < nt ? last[qb][r] : no_key);
                }
        }
    };
    if (one_block) scan(std::integral_constant<int, 1>{});
    else scan(std::integral_constant<int, QB>{});
    if (!wave_active) return;
    // the two wave halves hold the same query columns over different train rows: merge, lower half writes
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        // (the f32 keys are exact integers below 2^23: from here on as int)
        const int bi = best[qb] >= MF_NO_KEY_MIN_F ? MF_NO_KEY : (int)best[qb];
        const int si = second[qb] >= MF_NO_KEY_MIN_F ? MF_NO_KEY : (int)second[qb];
        const int ob = __shfl_xor(bi, 32), os = __shfl_xor(si, 32);
        const int hi = max(bi, ob);
        const int sec = min(min(si, os), hi);
        const int bst = min(bi, ob);
        const int q = block_row(qb);
        const int base = j0 + ((ntiles - 1) & ~1) * MF_TILE;  // the frame of the last rebasing: the first row of the last pair of tiles
        if (hf == 0 && q < nq && (qb == 0 || !one_block)) out[query_row(qb)] = make_uint2(key_to_knn(bst, base), key_to_knn(sec, base));
    }
}

// ---- the reverse check of the claimed columns (match_kernels.hip: forward_plan_kernel) in ONE launch -------------------------------
// Two lists per frame pair: the LIGHT columns, to be compared with the rows of S (tsel), and the HEAVY columns (back of the list), to
// be compared with ALL prev rows.  A list's train side is cut into rev_segments(rows) segments of at most ~256 rows; a UNIT of work is
// (list, segment): its train rows are made RESIDENT — requested in one go (eight words per thread in flight behind their list entries),
// expanded into LDS once, ONE barrier — and then every wave runs ITS column blocks (32 columns each) against the resident tiles without
// meeting the others again: the next block's rows are requested (list entries two blocks ahead, rows one block ahead) while the
// current block is multiplied.  The general scan above, used for this in rounds 3 - 4 (one launch per list), pays one global fetch per
// barrier and per two tiles and ran at the latency of that fetch (round 5, 512 clustered frames: 97 heavy columns per frame took
// 113 us as one 2000-row scan per frame, the 1340 light ones 48 us against |S| = 178 rows; 0.186 ms for the whole check).
// `slots` workgroups per frame pair share the units: column group g (4 blocks, one per wave) of segment seg belongs to slot
// (g + seg) mod slots — the groups of a long light list spread over the slots, and so do the segments of a short heavy list.  A frame
// whose plan left nothing to scan (i.i.d. rows: S is empty) costs `slots` workgroups that read four counters and leave.
// A segment longer than a chunk (more than 2048 train rows) takes several chunks, one after the other.
// Result: m12[claimant] = -1 for every listed column whose claim some other row blocks (each train range decides for itself: the
// question is a union over ranges; forward_plan_kernel wrote m12[claimant] = column before) — no top-2 array leaves the kernel.
constexpr int REV_CHUNK_TILES = 8, REV_CHUNK = REV_CHUNK_TILES * MF_TILE;
constexpr int REV_MAX_SEG = 8;
__host__ __device__ inline int rev_segments(int train_rows) {  // train segments of a column list with this many train rows
    const int s = (train_rows + 255) / 256;
    return s < 1 ? 1 : (s > REV_MAX_SEG ? REV_MAX_SEG : s);
}

__global__ __launch_bounds__(MF_BLOCK, 4) void hamming_knn2_mfma_reverse_kernel(int B, int slots, int row_stride, const uint8_t* __restrict__ d1,
                                                                                const int32_t* __restrict__ n1, const uint8_t* __restrict__ d2,
                                                                                const int32_t* __restrict__ qsel, const int32_t* __restrict__ nsel,
                                                                                const int32_t* __restrict__ tsel, const uint32_t* __restrict__ claim,
                                                                                float nnr, int32_t* __restrict__ m12) {
    constexpr int KSTEPS = 4;
    using key_t = float;
    using acc_t = v16f;
    __shared__ v4i s_tile[REV_CHUNK_TILES][KSTEPS * 2 * 32];  // 32 KB: every tile of the chunk
    __shared__ uint16_t s_thr[257];                           // block_threshold(d0), d0 = 0 .. 256: the largest distance that still blocks a claim at d0
    const int L = blockIdx.x;
    const int xcd = L & 7, k = L >> 3;
    const int b = (k / slots) * 8 + xcd, slot = k % slots;
    if (b >= B) return;
    const int na = n1[b];
    const int nl = nsel[(size_t)B + b], nh = nsel[2 * (size_t)B + b], ns = nsel[3 * (size_t)B + b];
    if ((ns == 0 || nl == 0) && nh == 0) return;  // (an empty S: nothing can block a light column any more)
    {   // block_threshold (match_scratch.h) for every d0, its loop written out: calling the function here changes the register
        // allocation of this whole kernel
        const float f0 = (float)threadIdx.x;
        uint32_t thr = threadIdx.x;
        while (thr < 256u && !(f0 < (float)(thr + 1u) * nnr)) ++thr;
        s_thr[threadIdx.x] = (uint16_t)thr;
        if (threadIdx.x == 0) s_thr[256] = 256;  // (a claim at distance 256 — possible with nnr > 1 only — is blocked by any other row: nothing is farther)
    }   // (read after the first barrier below)
    const size_t frame_off = (size_t)b * row_stride;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, hf = lane >> 5;
    const int xr = tid & 31, xk = tid >> 5;  // staging role: word xk of train row xr of a tile
    const uint32_t* __restrict__ Q = reinterpret_cast<const uint32_t*>(d2 + frame_off * STVO_DESC_BYTES);  // the columns: curr rows
    const uint32_t* __restrict__ T = reinterpret_cast<const uint32_t*>(d1 + frame_off * STVO_DESC_BYTES);  // against prev rows
    acc_t cidx;
#pragma unroll
    for (int r = 0; r < 16; ++r) cidx[r] = (key_t)((r & 3) + 8 * (r >> 2) + 4 * hf);
    auto mma = [&](const v4i& tf, const v4i& q, const acc_t& c) -> acc_t {
        const v8i a8 = {tf.x, tf.y, tf.z, tf.w, 0, 0, 0, 0}, b8 = {q.x, q.y, q.z, q.w, 0, 0, 0, 0};
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, MF_SCALE_2_4, 0, MF_SCALE_2_4);
    };

    for (int list = 0; list < 2; ++list) {
        const bool light = list == 0;
        const int nq = light ? (ns > 0 ? nl : 0) : nh, nt_all = light ? ns : na;
        if (nq == 0) continue;
        const int nseg = rev_segments(nt_all);
        const int n_groups = (nq + 127) / 128;  // 4 blocks of 32 columns, one per wave
        const int seg_len = (((nt_all + nseg - 1) / nseg) + MF_TILE - 1) & ~(MF_TILE - 1);
        auto column_of = [&](int g) -> int {  // this lane's column (a position in the list) of group g; tail lanes take a valid one
            const int q = (g * 4 + wv) * 32 + col;
            return q < nq ? q : nq - 1;
        };
        auto list_entry = [&](int g) -> int { return qsel[frame_off + (light ? column_of(g) : row_stride - 1 - column_of(g))]; };
        for (int seg = 0; seg < nseg; ++seg) {
            // this workgroup's groups of the unit: g = g_first, g_first + slots, ...
            const int g_first = ((slot - seg) % slots + slots) % slots;
            if (g_first >= n_groups) continue;  // (workgroup-uniform)
            const int j0 = min(seg * seg_len, nt_all), nt = min(j0 + seg_len, nt_all);
            for (int c0 = j0; c0 < nt || c0 == j0; c0 += REV_CHUNK) {  // (an empty segment still writes "no key" for its columns)
                // ---- the chunk's train rows -> LDS
                uint32_t w[REV_CHUNK_TILES];
#pragma unroll
                for (int t = 0; t < REV_CHUNK_TILES; ++t) {
                    const int j = c0 + t * MF_TILE + xr;
                    uint32_t v = 0u;
                    if (j < nt) v = T[(size_t)(light ? tsel[frame_off + j] : j) * 8 + xk];
                    w[t] = v;
                }
                // (the first two groups' list entries travel with them)
                int e_cur = list_entry(g_first);
                int e_next = g_first + slots < n_groups ? list_entry(g_first + slots) : 0;
                const int ntc = min((nt - c0 + MF_TILE - 1) / MF_TILE, REV_CHUNK_TILES);
#pragma unroll
                for (int t = 0; t < REV_CHUNK_TILES; ++t)
                    if (t < ntc) s_tile[t][xk * 32 + xr] = expand_fp4(w[t]);
                uint4 qw0 = reinterpret_cast<const uint4*>(Q)[2 * e_cur], qw1 = reinterpret_cast<const uint4*>(Q)[2 * e_cur + 1];
                uint32_t cw = claim[frame_off + e_cur];  // (d0 << 16) | claimant of the lane's column
                __syncthreads();
                // ---- every wave: its blocks against the resident tiles
                for (int g = g_first; g < n_groups; g += slots) {
                    const bool up = hf != 0;
                    v4i qf[KSTEPS];
                    qf[0] = expand_fp4(~(up ? qw0.y : qw0.x));
                    qf[1] = expand_fp4(~(up ? qw0.w : qw0.z));
                    qf[2] = expand_fp4(~(up ? qw1.y : qw1.x));
                    qf[3] = expand_fp4(~(up ? qw1.w : qw1.z));
                    const uint32_t c_claim = cw;
                    const bool block_active = (g * 4 + wv) * 32 < nq;
                    // requests one block ahead (rows) and two ahead (list entry): under way while this block is multiplied
                    if (g + slots < n_groups) {
                        qw0 = reinterpret_cast<const uint4*>(Q)[2 * e_next];
                        qw1 = reinterpret_cast<const uint4*>(Q)[2 * e_next + 1];
                        cw = claim[frame_off + e_next];
                        e_cur = e_next;
                        if (g + 2 * slots < n_groups) e_next = list_entry(g + 2 * slots);
                    }
                    if (!block_active) continue;
                    key_t best = MF_NO_KEY_F, second = MF_NO_KEY_F;
                    auto fold = [&](key_t key) {
                        second = med3_f32(best, second, key);
                        best = min_f32(best, key);
                    };
                    int last_base = c0;
                    if (ntc > 0) {
                        // software pipeline, depth one tile (as the general scan): tile t's matrix instructions are issued, tile t - 1's
                        // keys are folded in their shadow; the chunk's last tile is folded after the loop
                        auto do_tile = [&](acc_t& cur, acc_t& prev, int t) {
                            key_t nd[5];
                            const v4i* frag = s_tile[t];
                            const bool fold_prev = t > 0;
                            if (fold_prev) {
                                best -= (key_t)MF_TILE;
                                second -= (key_t)MF_TILE;
                            }
                            v4i tf = frag[lane];
#pragma unroll
                            for (int kk = 0; kk < KSTEPS; ++kk) {
                                v4i tf_ahead = tf;
                                if (kk < KSTEPS - 1) tf_ahead = frag[(kk + 1) * 64 + lane];
                                cur = mma(tf, qf[kk], kk == 0 ? cidx : cur);
                                if (fold_prev) {
                                    if (kk == 0) {
                                        // The folds read tile t - 1's accumulators through inline asm (v_min3 / v_med3 without
                                        // canonicalisation), which the compiler's hazard recogniser does not cover: nothing stops it from
                                        // scheduling them right behind the matrix instruction that writes them, and the hardware does not
                                        // interlock that read (round 5: one wrong top-2 in the adversarial test with a single instruction
                                        // between the two).  The wait states of a 16-pass XDL write -> VALU read (19), tied to the
                                        // registers, in the shadow of this tile's first matrix instruction.
                                        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 2" : "+v"(prev));
                                        // (the fold as a tournament of v_min3 / v_med3 nodes, as in the forward scan above)
                                        nd[0] = min3_f32(prev[0], prev[1], prev[2]);
                                        nd[1] = min3_f32(prev[3], prev[4], prev[5]);
                                        second = min3_f32(second, med3_f32(prev[0], prev[1], prev[2]), med3_f32(prev[3], prev[4], prev[5]));
                                    } else if (kk == 1) {
                                        nd[2] = min3_f32(prev[6], prev[7], prev[8]);
                                        nd[3] = min3_f32(prev[9], prev[10], prev[11]);
                                        second = min3_f32(second, med3_f32(prev[6], prev[7], prev[8]), med3_f32(prev[9], prev[10], prev[11]));
                                    } else if (kk == 2) {
                                        nd[4] = min3_f32(prev[12], prev[13], prev[14]);
                                        const key_t b0 = min3_f32(nd[0], nd[1], nd[2]);
                                        second = min3_f32(second, med3_f32(prev[12], prev[13], prev[14]), med3_f32(nd[0], nd[1], nd[2]));
                                        nd[0] = b0;
                                    } else {
                                        const key_t b1 = min3_f32(nd[3], nd[4], prev[15]), n1 = med3_f32(nd[3], nd[4], prev[15]);
                                        second = min3_f32(second, n1, med3_f32(nd[0], b1, best));
                                        best = min3_f32(nd[0], b1, best);
                                    }
                                }
                                if (kk < KSTEPS - 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                                __builtin_amdgcn_sched_group_barrier(0x002, MF_FOLD_SLOTS, 0);
                                tf = tf_ahead;
                            }
                        };
                        acc_t accA, accB;
#pragma unroll
                        for (int r = 0; r < 16; ++r) accA[r] = accB[r] = 0;
                        int t = 0;
                        for (; t + 2 <= ntc; t += 2) {
                            do_tile(accA, accB, t);
                            do_tile(accB, accA, t + 1);
                        }
                        if (t < ntc) do_tile(accA, accB, t);
                        acc_t& last = (ntc & 1) ? accA : accB;
                        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 2" : "+v"(last));  // (as above: read by asm folds)
                        best -= (key_t)MF_TILE;
                        second -= (key_t)MF_TILE;
                        last_base = c0 + (ntc - 1) * MF_TILE;  // first train row of the tile the keys are relative to
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int jr = last_base + (r & 3) + 8 * (r >> 2) + 4 * hf;
                            fold(jr < nt ? last[r] : MF_NO_KEY_F);
                        }
                    }
                    // the two wave halves hold the same columns over different train rows: merge, lower half writes
                    const int bi = best >= MF_NO_KEY_MIN_F ? MF_NO_KEY : (int)best;
                    const int si = second >= MF_NO_KEY_MIN_F ? MF_NO_KEY : (int)second;
                    const int ob = __shfl_xor(bi, 32), os = __shfl_xor(si, 32);
                    const int hi = max(bi, ob);
                    const int sec = min(min(si, os), hi);
                    const int bst = min(bi, ob);
                    // The verdict of this train range: the claim (row i*, distance d0) on the column is BLOCKED iff some other row lies within
                    // T = block_threshold(d0) — a union over segments and chunks, so every range decides for itself from its own top-2
                    // (the nearest row if it is not the claimant, else the second) and the claimant of a blocked column loses its match; writers only store -1.
                    if (hf == 0 && (g * 4 + wv) * 32 + col < nq) {
                        const uint32_t x = key_to_knn(bst, last_base), y = key_to_knn(sec, last_base);
                        if (x != 0xFFFFFFFFu) {
                            const uint32_t T = s_thr[c_claim >> 16], istar = c_claim & 0xFFFFu;
                            bool blk = false;
                            if ((x >> 16) <= T) {  // (else nothing of the range is within T)
                                const uint32_t pos = x & 0xFFFFu;
                                const uint32_t row = light ? (uint32_t)tsel[frame_off + pos] : pos;
                                blk = row != istar || (y != 0xFFFFFFFFu && (y >> 16) <= T);
                            }
                            if (blk) m12[frame_off + istar] = -1;
                        }
                    }
                }
                __syncthreads();  // the tile buffers are staged again (next chunk, next unit)
            }
        }
    }
}

void launch_hamming_knn2_mfma_reverse(hipStream_t s, const MatchProblem& p, const MatchViews& v, int32_t* m12, int slots) {
    if (p.B <= 0 || p.row_stride <= 0) return;
    const dim3 grid((unsigned)(((p.B + 7) / 8) * 8 * slots));
    hipLaunchKernelGGL(hamming_knn2_mfma_reverse_kernel, grid, dim3(MF_BLOCK), 0, s, p.B, slots, p.row_stride, p.d1, p.n1, p.d2, v.qsel, v.nsel, v.tsel,
                       v.claim, p.nnr, m12);
}

template <int QB>
static void launch_mf(hipStream_t s, const KnnScan& a) {
    const MatchProblem& p = a.p;
    constexpr int rows = 4 * QB * 32;  // query rows per workgroup
    const int tiles = (p.row_stride + rows - 1) / rows, ndir = a.both_directions ? 2 : 1;
    const int groups = (p.B + 7) / 8;
    const dim3 grid((unsigned)(groups * 8 * tiles * ndir * a.nseg));
    // dir0, the first direction of the launch, stays a kernel argument although it is always the forward one: as a constant it
    // takes an instruction out of the scan, and this kernel's instruction stream is held fixed
    const int first_direction = 0;
    hipLaunchKernelGGL((hamming_knn2_mfma_kernel<QB, 0>), grid, dim3(MF_BLOCK), 0, s, p.B, tiles, ndir, first_direction, a.nseg, p.row_stride, p.d1, p.n1, p.d2, p.n2,
                       a.knn12, a.knn21, a.claim_init);
}

void launch_hamming_knn2_mfma(hipStream_t s, const KnnScan& a, int qb) {
    if (a.p.B <= 0 || a.p.row_stride <= 0) return;
    if (qb == 1) launch_mf<1>(s, a);
    else if (qb == 2) launch_mf<2>(s, a);
    else launch_mf<4>(s, a);
}

}  // namespace stvo
