// The work split of the rectifier bank (stvo-pl_amd/csrc/rectify_bank_plan.h) behind a flat C interface — TEST INFRASTRUCTURE ONLY.
// tests/test_rectify_bank_plan_host.py runs it over planned assignments and checks the cover.  Built by g++ alone: the header includes
// nothing of HIP.  With RECTIFY_BANK_PLAN_HOST_MAIN it is a stand-alone program that plans into allocations of exactly the sizes the
// header states and walks every item (the sanitizer build).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stvo-pl_amd/csrc/rectify_bank_plan.h"

extern "C" {

int rbp_block() { return stvo::RBANK_BLOCK; }
long long rbp_max_items(int B, int K, int slot_cols, int slot_rows) { return (long long)stvo::rbank_max_items(B, K, slot_cols, slot_rows); }
long long rbp_items_offset(int B) { return (long long)stvo::rbank_items_offset(B); }
long long rbp_table_bytes(int B, long long n_items) { return (long long)stvo::rbank_table_bytes(B, (size_t)n_items); }
int rbp_nquads(int cols, int rows) { return stvo::rbank_nquads(cols, rows); }

// pairs [B], items [max_items][4] = calib, qblock, pair_begin, pair_count; returns the number of items (-1: they did not fit)
int rbp_plan(int B, int K, const int32_t* calib_of_pair, const int32_t* cols, const int32_t* rows, int32_t* pairs, int32_t* items,
             long long max_items) {
    static_assert(sizeof(stvo::RectBankItem) == 4 * sizeof(int32_t), "an item is four words");
    return stvo::plan_rectify_bank(B, K, calib_of_pair, cols, rows, pairs, reinterpret_cast<stvo::RectBankItem*>(items), (size_t)max_items);
}
}

#ifdef RECTIFY_BANK_PLAN_HOST_MAIN
// the table planned into an allocation of exactly rbank_table_bytes(B, rbank_max_items(...)); every (pair, quad) counted once
static bool walk(int B, int K, const std::vector<int32_t>& assign, const std::vector<int32_t>& cols, const std::vector<int32_t>& rows, int sc, int sr) {
    const size_t max_items = stvo::rbank_max_items(B, K, sc, sr);
    std::vector<unsigned char> table(stvo::rbank_table_bytes(B, max_items));
    int32_t* pairs = reinterpret_cast<int32_t*>(table.data());
    stvo::RectBankItem* items = reinterpret_cast<stvo::RectBankItem*>(table.data() + stvo::rbank_items_offset(B));
    const int n = stvo::plan_rectify_bank(B, K, assign.data(), cols.data(), rows.data(), pairs, items, max_items);
    if (n < 0 || (size_t)n > max_items) return false;
    std::vector<std::vector<int>> seen((size_t)B);
    for (int b = 0; b < B; ++b) seen[(size_t)b].assign((size_t)stvo::rbank_nquads(cols[(size_t)assign[(size_t)b]], rows[(size_t)assign[(size_t)b]]), 0);
    for (int i = 0; i < n; ++i) {
        const stvo::RectBankItem& it = items[i];
        if (it.calib < 0 || it.calib >= K || it.pair_count < 1 || it.pair_begin < 0 || it.pair_begin + it.pair_count > B) return false;
        const int nq = stvo::rbank_nquads(cols[(size_t)it.calib], rows[(size_t)it.calib]);
        for (int j = 0; j < it.pair_count; ++j) {
            const int b = pairs[it.pair_begin + j];
            if (b < 0 || b >= B || assign[(size_t)b] != it.calib) return false;
            for (int t = 0; t < stvo::RBANK_BLOCK; ++t) {
                const int q = it.qblock * stvo::RBANK_BLOCK + t;
                if (q < nq) ++seen[(size_t)b][(size_t)q];
            }
        }
    }
    for (const auto& s : seen)
        for (int c : s)
            if (c != 1) return false;
    return true;
}

int main() {
    struct Case { int B, sc, sr; std::vector<int32_t> cols, rows, assign; };
    const std::vector<Case> cases = {
        {7, 53, 21, {53, 50, 7, 3, 1, 40}, {21, 19, 5, 2, 1, 16}, {0, 1, 1, 2, 3, 4, 5}},
        {7, 53, 21, {53, 50, 7, 3, 1, 40}, {21, 19, 5, 2, 1, 16}, {4, 4, 4, 4, 4, 4, 4}},
        {1, 1, 1, {1}, {1}, {0}},
        {256, 1242, 480, {1241, 1242, 752}, {376, 375, 480}, std::vector<int32_t>(256, 2)},
        {257, 640, 480, {640, 1}, {480, 1}, std::vector<int32_t>(257, 1)},
    };
    int bad = 0;
    for (const Case& c : cases) {
        const bool ok = walk(c.B, (int)c.cols.size(), c.assign, c.cols, c.rows, c.sc, c.sr);
        std::printf("B %3d K %d slot %4d x %3d: %s\n", c.B, (int)c.cols.size(), c.sc, c.sr, ok ? "every quad once, inside the table" : "INCONSISTENT");
        bad += !ok;
    }
    std::printf("%d cases, %d inconsistent\n", (int)cases.size(), bad);
    return bad ? 1 : 0;
}
#endif
