// rectify_bank.hip — one rectifier for mixed cameras (stvo_rectify_bank_*): a different map set and image size for every pair of ONE
// launch, over K resident stvo_rectify objects whose maps the bank borrows.  Source and destination are slot-shaped
// ([n][slot_rows][slot_cols][channels]); image b is the top-left cols_k x rows_k of its slot at the slot's row pitch, the layout
// stvo_orb_set_image_sizes reads.  Per pair the crop of the destination is bit for bit what rectifier k alone writes for the crop of the
// source (rectify_px.h states the arithmetic, from which every primitive here is drawn: (X + 512) >> 10 per channel, a tap outside the IMAGE reads 0 —
// also where it lies inside the slot — and cvtColor's integer weights behind the 8-bit rounding); nothing outside the crop is written.
//
//   rectify_bank_kernel<CH, GRAY>  one workgroup = one item of the plan (rectify_bank_plan.h: calibration, 256 quads, a list of pairs),
//                                  blockIdx.y = side.  What the uniform kernels keep cheap is kept: a quad's maps are loaded once (one
//                                  16-B and one 8-B load) and held in registers over the item's pairs, the inside flag of map2 selects
//                                  the path without per-tap tests (the branch stands outside the loop over the quad's pixels: 16 loads
//                                  issued together), and a quad whose 4 pixels lie in one row is stored by dwords.  New against them:
//                                  the quad's pixel index is split into (row, column) of the image once per thread, since the row
//                                  pitch is the slot's — which also makes a run's address dword-aligned in some rows only, so runs are
//                                  stored as unaligned dwords; the calibration's record, the item and the pair list are
//                                  workgroup-uniform and read with scalar loads.  dist = 0 calibrations have no maps: their items copy
//                                  the crop (GRAY: convert it), reading exactly the pixels they write, COPY_BATCH pairs in flight.
//
// The assignment (which calibration a pair takes) is known to the host: stvo_rectify_bank_assign splits the work there
// (plan_rectify_bank) into pinned staging and sends the table on the context's stream, behind the launches that read the previous one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "ctx_internal.h"
#include "rectify_bank_plan.h"
#include "rectify_internal.h"

namespace {

using stvo::RBANK_BLOCK;
using stvo::RectBankItem;
constexpr int COPY_BATCH = 8;  // pairs a copying thread has in flight

// one calibration as the kernel reads it (workgroup-uniform: scalar loads)
struct BankCalib {
    const int4* map1q[2];   // [side] the rectifier's resident maps, nullptr with dist = 0
    const uint2* map2q[2];
    int32_t cols, rows, nquads, dist;
};
static_assert(sizeof(BankCalib) == 48, "four pointers and four words");

// The quad's 4 pixels of CH bytes each into the slot at D (pixel k at byte D + at[k]): CH dwords where the quad is one run of a row,
// else the pixels that exist by bytes.  The slot's pitch is not the image's width, so the run's address is dword-aligned only in some
// rows (pitch 1242: every other row); the dwords are stored at whatever alignment the run has, as load_px reads its 4-channel pixels
// (global memory takes unaligned dwords; a run never leaves its row, so nothing beyond the crop is touched).
template <int CH>
__device__ __forceinline__ void store_quad(uint8_t* __restrict__ D, const uint32_t (&at)[4], bool one_run, const bool (&live)[4],
                                           const uint32_t (&v)[4][CH]) {
    if (one_run) {
        uint32_t o[CH];
        pack_quad<CH>(v, o);
        __builtin_memcpy(D + at[0], o, 4 * CH);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (live[k]) {
#pragma unroll
                for (int c = 0; c < CH; ++c) D[at[k] + c] = (uint8_t)v[k][c];
            }
    }
}

// The quad's 4 pixels read as one run of a row (dist = 0: a calibration that copies): CH dwords at whatever alignment the run has.
template <int CH>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ s, uint32_t (&wd)[CH]) {
#pragma unroll
    for (int c = 0; c < CH; ++c) __builtin_memcpy(&wd[c], s + 4 * c, 4);
}

template <int CH>
__device__ __forceinline__ void store_run(uint8_t* __restrict__ d, const uint32_t (&wd)[CH]) {
#pragma unroll
    for (int c = 0; c < CH; ++c) __builtin_memcpy(d + 4 * c, &wd[c], 4);
}

// An empty asm over loaded dwords keeps them dwords: left alone, the compiler narrows a dword that is only ever taken apart into byte
// loads again.  Placed behind ALL the loads of a batch, so that none of them is waited for before the last is issued.
template <int CH>
__device__ __forceinline__ void keep_dwords(uint32_t (&wd)[CH]) {
#pragma unroll
    for (int c = 0; c < CH; ++c) asm volatile("" : "+v"(wd[c]));
}

template <int CH, int NC>
__device__ __forceinline__ void unpack_run(const uint32_t (&wd)[CH], uint32_t (&v)[4][NC]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = k * CH + c;
            v[k][c] = (wd[j >> 2] >> ((j & 3) * 8)) & 0xffu;
        }
}

// The plan's table is written before the launch and by nothing in it: read through the constant address space it is a scalar load.
// (Read as global memory the compiler cannot rule out the kernel's own stores, and makes it a vector load with a wait for every
// memory operation in flight in front of each pair.)
__device__ __forceinline__ int32_t table_word(const int32_t* p) {
    return *(const __attribute__((address_space(4))) int32_t*)(p);
}

// src / dst: this side's first slot.  GRAY = false: dst holds CH-channel slots, dstb unused.  GRAY = true: dst is plane A, dstb plane B
// or NULL (both sides), one byte per pixel.  n: pairs of the call (the pairs of the plan at or beyond n are passed over).
template <int CH, bool GRAY>
__global__ void __launch_bounds__(RBANK_BLOCK) rectify_bank_kernel(const BankCalib* __restrict__ calibs, const int32_t* __restrict__ pairs,
                                                                   const RectBankItem* __restrict__ items,
                                                                   const uint8_t* __restrict__ src_l, const uint8_t* __restrict__ src_r,
                                                                   uint8_t* __restrict__ dst_l, uint8_t* __restrict__ dst_r,
                                                                   uint8_t* __restrict__ dstb_l, uint8_t* __restrict__ dstb_r, int n,
                                                                   int slot_cols, int slot_rows, GrayWeights w) {
    constexpr int NC = GRAY ? 3 : CH;   // channels computed: the grey planes never read alpha
    constexpr int DCH = GRAY ? 1 : CH;  // bytes per pixel of the destination
    const RectBankItem it = items[blockIdx.x];
    const BankCalib& cal = calibs[it.calib];
    const int q = it.qblock * RBANK_BLOCK + (int)threadIdx.x;
    if (q >= cal.nquads) return;
    const bool right = blockIdx.y != 0;
    const int dist = cal.dist;
    const uint8_t* src = right ? src_r : src_l;
    uint8_t* dst = right ? dst_r : dst_l;
    uint8_t* dstb = right ? dstb_r : dstb_l;
    const int cols = cal.cols, rows = cal.rows;
    // Offsets inside a slot are 32-bit: a slot holds at most 32767 x 32767 pixels of 4 bytes, below 2^32 bytes.
    const uint32_t npx = (uint32_t)cols * (uint32_t)rows;
    const size_t slot_px = (size_t)slot_cols * slot_rows;
    const uint32_t pitch_b = (uint32_t)slot_cols * CH;
    const uint32_t p0 = (uint32_t)q * 4u;
    // the quad's pixels in the image: (row, column) of each, where it lands in the slot, and whether it exists
    uint32_t dpx[4];  // offset in PIXELS of the slot
    bool live[4];
    const uint32_t y0 = p0 / (uint32_t)cols, x0 = p0 - y0 * (uint32_t)cols;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t x = x0 + k, y = y0;
#pragma unroll
        for (int wrap = 0; wrap < 3; ++wrap)  // (an image narrower than a quad wraps up to three times)
            if (x >= (uint32_t)cols) { x -= (uint32_t)cols; ++y; }
        live[k] = p0 + k < npx;
        dpx[k] = y * (uint32_t)slot_cols + x;
    }
    const bool one_run = x0 + 3u < (uint32_t)cols;  // 4 pixels of one row: all exist
    uint32_t dbytes[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dbytes[k] = dpx[k] * DCH;

    // the quad's maps, loaded once and held over the item's pairs (dist = 0: none)
    int4 m1 = make_int4(0, 0, 0, 0);
    uint2 m2v = make_uint2(0u, 0u);
    if (dist) {
        m1 = (right ? cal.map1q[1] : cal.map1q[0])[q];
        m2v = (right ? cal.map2q[1] : cal.map2q[0])[q];
    }
    const int m1s[4] = {m1.x, m1.y, m1.z, m1.w};
    const uint32_t m2s[4] = {m2v.x & 0xffffu, m2v.x >> 16, m2v.y & 0xffffu, m2v.y >> 16};
    int mx[4], my[4];
    uint32_t soff[4];  // source offset in bytes of the top-left tap (dist = 0: of the pixel itself); read only where the pixel is inside
    bool all_inside = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        map_tap(m1s[k], mx[k], my[k]);
        soff[k] = dist ? (uint32_t)my[k] * pitch_b + (uint32_t)mx[k] * CH : dpx[k] * CH;
        all_inside = all_inside && (m2s[k] & INSIDE);
    }

    // the pixels of pair b are in v: weigh them (GRAY) and store
    auto emit = [&](int b, const uint32_t (&v)[4][NC]) {
        if constexpr (GRAY) {
            uint32_t ga[4][1];
#pragma unroll
            for (int k = 0; k < 4; ++k) ga[k][0] = weigh(v[k][0], v[k][1], v[k][2], w.w0, w.w1, w.w2, w);
            store_quad<1>(dst + (size_t)b * slot_px, dbytes, one_run, live, ga);
            if (dstb) {
                uint32_t gb[4][1];
#pragma unroll
                for (int k = 0; k < 4; ++k) gb[k][0] = weigh(v[k][0], v[k][1], v[k][2], w.w2, w.w1, w.w0, w);
                store_quad<1>(dstb + (size_t)b * slot_px, dbytes, one_run, live, gb);
            }
        } else {
            store_quad<DCH>(dst + (size_t)b * slot_px * DCH, dbytes, one_run, live, v);
        }
    };

    // a calibration's pairs are listed in ascending order: the first one at or beyond n ends the item
    const int32_t* list = pairs + it.pair_begin;
    const int b_first = table_word(list);
    if (b_first >= n) return;
    if (!dist) {
        // The reference copies: the pixels themselves, only where they exist.  A copy has one load per quad and pair, so the pairs are
        // taken COPY_BATCH at a time with their loads issued together (a pair beyond the item's or the call's loads the first pair's quad
        // again and stores nothing): the bytes in flight per lane are what a copy kernel's 16-byte loads would hold.
        if (one_run) {
            for (int j = 0; j < it.pair_count; j += COPY_BATCH) {
                int bs[COPY_BATCH];
                bool valid[COPY_BATCH];
                uint32_t wd[COPY_BATCH][CH];
#pragma unroll
                for (int u = 0; u < COPY_BATCH; ++u) {
                    const int b = j + u < it.pair_count ? table_word(list + j + u) : n;
                    valid[u] = b < n;
                    bs[u] = valid[u] ? b : b_first;
                    load_run<CH>(src + (size_t)bs[u] * slot_px * CH + soff[0], wd[u]);
                }
                if constexpr (GRAY) {
#pragma unroll
                    for (int u = 0; u < COPY_BATCH; ++u) keep_dwords<CH>(wd[u]);
                }
#pragma unroll
                for (int u = 0; u < COPY_BATCH; ++u) {
                    if (!valid[u]) continue;
                    if constexpr (GRAY) {
                        uint32_t v[4][NC];
                        unpack_run<CH, NC>(wd[u], v);
                        emit(bs[u], v);
                    } else {
                        store_run<CH>(dst + (size_t)bs[u] * slot_px * CH + dbytes[0], wd[u]);
                    }
                }
                if (!valid[COPY_BATCH - 1]) break;
            }
        } else {  // the quad straddles two rows or runs past the image's end
            for (int j = 0; j < it.pair_count; ++j) {
                const int b = table_word(list + j);
                if (b >= n) break;
                const uint8_t* S = src + (size_t)b * slot_px * CH;
                uint32_t v[4][NC];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (live[k]) {
                        load_px<CH, NC>(S + soff[k], v[k]);
                    } else {
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[k][c] = 0u;
                    }
                }
                emit(b, v);
            }
        }
        return;
    }
    auto at = [&](int x, int y) { return (size_t)y * (size_t)pitch_b + (size_t)x * CH; };  // a pixel's offset in its slot
    for (int j = 0; j < it.pair_count; ++j) {
        const int b = table_word(list + j);
        if (b >= n) break;
        const uint8_t* S = src + (size_t)b * slot_px * CH;
        uint32_t v[4][NC];
        if (all_inside) {  // (the branch outside the loop over the pixels, as in the one-channel uniform kernel: one run of 16 loads)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t t00[NC], t01[NC], t10[NC], t11[NC];
                const uint8_t* s = S + soff[k];
                load_px<CH, NC>(s, t00);
                load_px<CH, NC>(s + CH, t01);
                load_px<CH, NC>(s + pitch_b, t10);
                load_px<CH, NC>(s + pitch_b + CH, t11);
#pragma unroll
                for (int c = 0; c < NC; ++c) v[k][c] = blend(t00[c], t01[c], t10[c], t11[c], m2s[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t t00[NC], t01[NC], t10[NC], t11[NC];
                tap_px<CH, NC>(S, mx[k], my[k], cols, rows, at, t00);
                tap_px<CH, NC>(S, mx[k] + 1, my[k], cols, rows, at, t01);
                tap_px<CH, NC>(S, mx[k], my[k] + 1, cols, rows, at, t10);
                tap_px<CH, NC>(S, mx[k] + 1, my[k] + 1, cols, rows, at, t11);
#pragma unroll
                for (int c = 0; c < NC; ++c) v[k][c] = blend(t00[c], t01[c], t10[c], t11[c], m2s[k]);
            }
        }
        emit(b, v);
    }
}

}  // namespace

struct stvo_rectify_bank {
    stvo_ctx* ctx = nullptr;
    int B = 0, K = 0, slot_cols = 0, slot_rows = 0;
    std::vector<stvo_rectify*> rects;      // borrowed: the rectifiers outlive the bank
    std::vector<int32_t> cols, rows;       // [K] their sizes, as the plan takes them
    std::vector<int32_t> calib_of_pair;    // [B] the assignment in force
    size_t max_items = 0;
    int n_items = 0;                       // items of the table in force = workgroups per side of the next launch
    // one device block: [K] BankCalib, then the table of the assignment in force (rectify_bank_plan.h).  The table is copied on the
    // context's stream; two pinned staging blocks are used alternately, each with the event of the copy that last read it.
    char* dev = nullptr;
    BankCalib* d_calibs = nullptr;
    char* d_table = nullptr;
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int next = 0;
    const int32_t* d_pairs() const { return reinterpret_cast<const int32_t*>(d_table); }
    const RectBankItem* d_items() const { return reinterpret_cast<const RectBankItem*>(d_table + stvo::rbank_items_offset(B)); }
};

namespace {

// Validated before anything changes.  The table is formed on the host in a pinned block and copied on the context's stream, so it
// arrives behind the launches already enqueued (which read the previous table) and in front of the next one; nothing waits for it.  A
// pinned block is written again only after the copy that last read it (two calls ago) has completed.
int bank_assign(stvo_rectify_bank* k, const int32_t* calib_of_pair) {
    for (int b = 0; b < k->B; ++b)
        if (calib_of_pair[b] < 0 || calib_of_pair[b] >= k->K) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = k->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int hb = k->next;
    if (k->busy[hb]) {
        HIP_TRY(ctx, hipEventSynchronize(k->ev[hb]));
        k->busy[hb] = false;
    }
    char* tab = k->stage[hb];
    const int n_items = stvo::plan_rectify_bank(k->B, k->K, calib_of_pair, k->cols.data(), k->rows.data(), reinterpret_cast<int32_t*>(tab),
                                                reinterpret_cast<RectBankItem*>(tab + stvo::rbank_items_offset(k->B)), k->max_items);
    if (n_items <= 0) return STVO_ERR_CAPACITY;  // (never: max_items is the bound of every assignment, and B >= 1 pairs make an item)
    HIP_TRY(ctx, hipMemcpyAsync(k->d_table, tab, stvo::rbank_table_bytes(k->B, (size_t)n_items), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(k->ev[hb], ctx->stream));
    k->busy[hb] = true;
    k->next = hb ^ 1;
    k->n_items = n_items;
    std::memcpy(k->calib_of_pair.data(), calib_of_pair, (size_t)k->B * sizeof(int32_t));
    return STVO_OK;
}

template <int CH, bool GRAY>
void launch_bank(stvo_rectify_bank* k, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r, uint8_t* dstb_l,
                 uint8_t* dstb_r, const GrayWeights& w) {
    hipLaunchKernelGGL((rectify_bank_kernel<CH, GRAY>), dim3((unsigned)k->n_items, 2), dim3(RBANK_BLOCK), 0, k->ctx->stream, k->d_calibs,
                       k->d_pairs(), k->d_items(), src_l, src_r, dst_l, dst_r, dstb_l, dstb_r, n, k->slot_cols, k->slot_rows, w);
}

}  // namespace

extern "C" {

int stvo_rectify_bank_destroy(stvo_rectify_bank* k) {
    if (!k) return STVO_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    if (k->dev) (void)hipFree(k->dev);
    if (k->stage[0]) (void)hipHostFree(k->stage[0]);  // (one allocation for both blocks)
    for (hipEvent_t e : k->ev)
        if (e) (void)hipEventDestroy(e);
    delete k;
    return STVO_OK;
}

int stvo_rectify_bank_create(stvo_ctx* ctx, int B, int slot_cols, int slot_rows, stvo_rectify* const* rects, int K, stvo_rectify_bank** out) {
    if (!ctx || !rects || !out || B <= 0 || K <= 0 || slot_cols <= 0 || slot_rows <= 0 || slot_cols > 32767 || slot_rows > 32767)
        return STVO_ERR_INVALID_ARG;
    for (int i = 0; i < K; ++i) {
        const stvo_rectify* r = rects[i];
        if (!r || r->ctx != ctx || r->cols <= 0 || r->rows <= 0 || r->cols > slot_cols || r->rows > slot_rows) return STVO_ERR_INVALID_ARG;
        if (r->cam.dist && !r->dev) return STVO_ERR_INVALID_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_rectify_bank* k = new (std::nothrow) stvo_rectify_bank();
    if (!k) return STVO_ERR_HIP;
    k->ctx = ctx;
    k->B = B; k->K = K; k->slot_cols = slot_cols; k->slot_rows = slot_rows;
    k->rects.assign(rects, rects + K);
    k->calib_of_pair.assign((size_t)B, 0);
    std::vector<BankCalib> host((size_t)K);
    for (int i = 0; i < K; ++i) {
        const stvo_rectify* r = rects[i];
        k->cols.push_back(r->cols);
        k->rows.push_back(r->rows);
        BankCalib& c = host[(size_t)i];
        const bool dist = r->cam.dist != 0;
        for (int side = 0; side < 2; ++side) {
            c.map1q[side] = dist ? r->map1q(side) : nullptr;
            c.map2q[side] = dist ? r->map2q(side) : nullptr;
        }
        c.cols = r->cols; c.rows = r->rows; c.nquads = r->nquads; c.dist = dist ? 1 : 0;
    }
    k->max_items = stvo::rbank_max_items(B, K, slot_cols, slot_rows);
    const size_t calib_bytes = ((size_t)K * sizeof(BankCalib) + 255) & ~size_t(255);
    const size_t span = (stvo::rbank_table_bytes(B, k->max_items) + 255) & ~size_t(255);
    bool ok = hip_ok(ctx, hipMalloc((void**)&k->dev, calib_bytes + span), "hipMalloc rectify bank") &&
              hip_ok(ctx, hipHostMalloc((void**)&k->stage[0], 2 * span, hipHostMallocDefault), "hipHostMalloc rectify bank");
    for (auto& e : k->ev) ok = ok && hip_ok(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate rectify bank");
    if (ok) {
        k->stage[1] = k->stage[0] + span;
        k->d_calibs = reinterpret_cast<BankCalib*>(k->dev);
        k->d_table = k->dev + calib_bytes;
        ok = upload_now(ctx, k->d_calibs, host.data(), (size_t)K * sizeof(BankCalib), "hipMemcpy rectify bank");
    }
    // every pair starts on calibration 0
    if (!ok || bank_assign(k, k->calib_of_pair.data()) != STVO_OK) {
        stvo_rectify_bank_destroy(k);
        return STVO_ERR_HIP;
    }
    *out = k;
    return STVO_OK;
}

int stvo_rectify_bank_camera(const stvo_rectify_bank* k, int calib, stvo_rect_camera* out) {
    if (!k || calib < 0 || calib >= k->K) return STVO_ERR_INVALID_ARG;
    return stvo_rectify_camera(k->rects[(size_t)calib], out);
}

int stvo_rectify_bank_assign(stvo_rectify_bank* k, const int32_t* calib_of_pair_host) {
    if (!k || !calib_of_pair_host) return STVO_ERR_INVALID_ARG;
    return bank_assign(k, calib_of_pair_host);
}

int stvo_rectify_bank_images_dev(stvo_rectify_bank* k, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                                 uint8_t* dst_r) {
    if (!k || !src_l || !src_r || !dst_l || !dst_r || n <= 0 || n > k->B || (channels != 1 && channels != 3 && channels != 4))
        return STVO_ERR_INVALID_ARG;
    const size_t bytes = (size_t)n * k->slot_cols * k->slot_rows * channels;
    if (!stereo_ranges_ok(dst_l, dst_r, src_l, src_r, bytes)) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = k->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const GrayWeights none{};
    if (channels == 1)
        launch_bank<1, false>(k, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    else if (channels == 3)
        launch_bank<3, false>(k, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    else
        launch_bank<4, false>(k, n, src_l, src_r, dst_l, dst_r, nullptr, nullptr, none);
    return check_launch(ctx);
}

int stvo_rectify_bank_color_to_gray_dev(stvo_rectify_bank* k, int n, int channels, int order, int weights, const uint8_t* src_l,
                                        const uint8_t* src_r, uint8_t* gray_l, uint8_t* gray_r, uint8_t* swapped_l, uint8_t* swapped_r) {
    GrayWeights w;
    if (!k || !src_l || !src_r || !gray_l || !gray_r || n <= 0 || n > k->B || (channels != 3 && channels != 4) ||
        (swapped_l == nullptr) != (swapped_r == nullptr) || !gray_weights(order, weights, &w))
        return STVO_ERR_INVALID_ARG;
    const size_t px = (size_t)n * k->slot_cols * k->slot_rows, sb = px * channels;
    const uint8_t* planes[4] = {gray_l, gray_r, swapped_l, swapped_r};
    if (!gray_planes_ok(planes, swapped_l ? 4 : 2, px, src_l, src_r, sb)) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = k->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (channels == 3)
        launch_bank<3, true>(k, n, src_l, src_r, gray_l, gray_r, swapped_l, swapped_r, w);
    else
        launch_bank<4, true>(k, n, src_l, src_r, gray_l, gray_r, swapped_l, swapped_r, w);
    return check_launch(ctx);
}

}  // extern "C"
