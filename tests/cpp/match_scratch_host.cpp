// The matcher's scratch views and shared rules (stvo-pl_amd/csrc/match_scratch.h) behind a flat C interface — TEST INFRASTRUCTURE
// ONLY.  tests/test_match_scratch_host.py holds them against the arithmetic the launch code carried before the header existed.  Built
// by g++ alone: the header includes nothing of HIP on the host.  With MATCH_SCRATCH_HOST_MAIN it is a stand-alone program that
// allocates the arrays of a table of shapes for real and writes every view end to end (the sanitizer build).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stvo-pl_amd/csrc/match_scratch.h"

namespace {
long long at(const void* p) { return (long long)reinterpret_cast<uintptr_t>(p); }
}  // namespace

extern "C" {

// The six arrays at the addresses base[0..5] (knn12, knn21, cand, claim, qsel, nsel).  out: knn12 segments 0 and 1, claim, cand, qsel,
// nsel rows 0 .. 4, blocked, tsel (12 addresses), then `per`.
int msh_views(int B, int row_stride, long long knn_capacity, const long long* base, long long* out) {
    stvo::MatchScratch w;
    w.knn12 = reinterpret_cast<uint2*>((uintptr_t)base[0]);
    w.knn21 = reinterpret_cast<uint2*>((uintptr_t)base[1]);
    w.cand = reinterpret_cast<int32_t*>((uintptr_t)base[2]);
    w.claim = reinterpret_cast<uint32_t*>((uintptr_t)base[3]);
    w.qsel = reinterpret_cast<int32_t*>((uintptr_t)base[4]);
    w.nsel = reinterpret_cast<int32_t*>((uintptr_t)base[5]);
    w.knn_capacity = (size_t)knn_capacity;
    const stvo::MatchViews v = stvo::match_views(w, B, row_stride);
    int n = 0;
    out[n++] = at(v.knn12_seg(0)); out[n++] = at(v.knn12_seg(1));
    out[n++] = at(v.claim); out[n++] = at(v.cand); out[n++] = at(v.qsel);
    for (int k = 0; k < 5; ++k) out[n++] = at(v.nsel_row(k));
    out[n++] = at(v.blocked); out[n++] = at(v.tsel);
    out[n++] = (long long)v.per;
    return n;
}
int msh_fits(int B, int row_stride, long long knn_capacity) { return stvo::match_scratch_fits(B, row_stride, (size_t)knn_capacity) ? 1 : 0; }
int msh_pick_nseg(int B, int max_n, long long knn_capacity, int forced) { return stvo::knn_pick_nseg(B, max_n, (size_t)knn_capacity, forced); }
int msh_block_threshold(int d0, float nnr) { return (int)stvo::block_threshold((uint32_t)d0, nnr); }
int msh_nseg_limits(int* lo, int* hi) { *lo = stvo::KNN_MIN_NSEG; *hi = stvo::KNN_MAX_NSEG; return 0; }
}

#ifdef MATCH_SCRATCH_HOST_MAIN
// arrays sized as their owner sizes them; every view a launch would use is written from its first to its last element
static bool walk(int B, int row_stride, size_t cap, size_t rows_cap, int batch_cap) {
    if (!stvo::match_scratch_fits(B, row_stride, cap)) return false;
    std::vector<uint2> knn12(cap), knn21(cap);
    std::vector<int32_t> cand(rows_cap), qsel(rows_cap), nsel((size_t)batch_cap * 5);
    std::vector<uint32_t> claim(rows_cap);
    const stvo::MatchScratch w{knn12.data(), knn21.data(), cand.data(), claim.data(), qsel.data(), nsel.data(), cap};
    const stvo::MatchViews v = stvo::match_views(w, B, row_stride);
    const int picked = stvo::knn_pick_nseg(B, row_stride, cap, 0);
    int most = (int)(cap / (v.per ? v.per : 1));
    if (most > stvo::KNN_MAX_NSEG) most = stvo::KNN_MAX_NSEG;
    for (int nseg : {picked, most})
        for (int s = 0; s < nseg; ++s) std::memset(v.knn12_seg(s), 0x11, v.per * sizeof(uint2));
    std::memset(v.claim, 0xFF, v.per * 4);
    std::memset(v.cand, 0x22, v.per * 4);
    std::memset(v.qsel, 0x33, v.per * 4);
    for (int k = 0; k < 5; ++k) std::memset(v.nsel_row(k), 0x44, (size_t)B * 4);
    std::memset(v.blocked, 0, v.per * 4);
    std::memset(v.tsel, 0x55, v.per * 4);
    // tsel ends where knn21 ends, and lies behind blocked
    return reinterpret_cast<char*>(v.tsel + v.per) == reinterpret_cast<char*>(knn21.data() + cap) && v.tsel >= v.blocked + v.per;
}

int main() {
    int bad = 0, n = 0;
    static const int ctx_cases[][2] = {{1, 1}, {1, 2}, {1, 8192}, {1, 8193}, {1, 65535}, {9, 33}, {64, 4096}};
    for (const auto& c : ctx_cases) {  // stvo_ctx_create(max_rows = row_stride, max_batch = B)
        const int B = c[0], rs = c[1];
        const size_t cap = (size_t)rs * (size_t)(2 * B > stvo::KNN_MAX_NSEG ? 2 * B : stvo::KNN_MAX_NSEG);
        const bool ok = walk(B, rs, cap, (size_t)B * rs, B);
        std::printf("context  B %4d row_stride %5d capacity %9zu: %s\n", B, rs, cap, ok ? "views inside" : "INCONSISTENT");
        bad += !ok; ++n;
    }
    for (int B : {1, 64, 1024})
        for (int M : {64, 128, 512}) {  // the key-line scratch of a pipeline (seq_state.h)
            const size_t cap = (size_t)4 * B * M;
            const bool ok = walk(B, M, cap, (size_t)B * M, B);
            std::printf("pipeline B %4d row_stride %5d capacity %9zu: %s\n", B, M, cap, ok ? "views inside" : "INCONSISTENT");
            bad += !ok; ++n;
        }
    unsigned long long sum = 0;
    for (float nnr : {0.5f, 0.75f, 0.9f, 1.0f})
        for (unsigned d0 = 0; d0 <= 256; ++d0) {
            const unsigned t = stvo::block_threshold(d0, nnr);
            bad += t < d0 || t > 256;
            sum += t;
        }
    std::printf("%d shapes, block_threshold checksum %llu, %d inconsistent\n", n, sum, bad);
    return bad ? 1 : 0;
}
#endif
