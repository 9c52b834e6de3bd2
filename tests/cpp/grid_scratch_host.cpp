// The scratch of the stereo grid matchers (stvo-pl_amd/csrc/grid_scratch.h) behind a flat C interface — TEST INFRASTRUCTURE ONLY.
// tests/test_grid_scratch_host.py holds it against a plain statement of the sizes.  Built by g++ alone: the header includes nothing of
// HIP on the host.  With GRID_SCRATCH_HOST_MAIN it is a stand-alone program that cuts the arrays of a table of shapes from a real
// allocation and writes every one end to end (the sanitizer build).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stvo-pl_amd/csrc/grid_scratch.h"

namespace {
const uintptr_t kBase = (uintptr_t)1 << 40;  // a base no offset reaches: a null pointer is told from the buffer at offset 0
long long rel(const void* p) { return p ? (long long)(reinterpret_cast<uintptr_t>(p) - kBase) : -1; }
const unsigned char kUntouched = 0x5A;
}  // namespace

extern "C" {

// out: elements of cover, top2, owner2, elig, elig_cnt, ovf
int gsh_counts(int B, int rows1, int rows2, int with_bit_matrix, int with_misfit, long long* out) {
    const stvo::GridScratchCounts n = stvo::grid_scratch_counts(B, rows1, rows2, with_bit_matrix != 0, with_misfit != 0);
    const size_t v[6] = {n.cover, n.top2, n.owner2, n.elig, n.elig_cnt, n.ovf};
    for (int i = 0; i < 6; ++i) out[i] = (long long)v[i];
    return 6;
}

// out: words64, n1p, words of one frame's matrix
int gsh_dims(int rows1, int rows2, long long* out) {
    const stvo::GridMatrixDims d = stvo::grid_matrix_dims(rows1, rows2);
    out[0] = d.words64; out[1] = d.n1p; out[2] = (long long)d.words();
    return 3;
}

long long gsh_route_words(int B) { return (long long)stvo::grid_route_words(B); }
int gsh_elig_slots() { return stvo::GRID_ELIG; }

// One carve, or the two halves one after the other (parts = 1 then 2, 2 then 1: `first`), on a carver that has `lead` bytes cut already.
// out: byte offsets of cover, top2, owner2, elig, elig_cnt, ovf, misfit (-1: null), then the carver's offset behind the carve; a pointer
// a half must leave alone is reported as -2 when it was touched.
int gsh_carve(int B, int rows1, int rows2, int with_bit_matrix, int with_misfit, int first, long long lead, long long* out) {
    stvo::Carver c(reinterpret_cast<const void*>(kBase));
    c.off = (size_t)lead;
    stvo::GridScratch g;
    std::memset(&g, kUntouched, sizeof(g));
    stvo::GridScratch untouched = g;
    const bool bm = with_bit_matrix != 0, mf = with_misfit != 0;
    bool left_alone = true;
    if (first == stvo::GRID_SCRATCH_ALL) {
        stvo::carve_grid_scratch(c, g, B, rows1, rows2, bm, mf);
    } else {
        stvo::carve_grid_scratch(c, g, B, rows1, rows2, bm, mf, first);
        if (first == stvo::GRID_SCRATCH_ELIG)
            left_alone = g.cover == untouched.cover && g.top2 == untouched.top2 && g.owner2 == untouched.owner2;
        else
            left_alone = g.elig == untouched.elig && g.elig_cnt == untouched.elig_cnt && g.ovf == untouched.ovf && g.misfit == untouched.misfit;
        stvo::carve_grid_scratch(c, g, B, rows1, rows2, bm, mf, stvo::GRID_SCRATCH_ALL & ~first);
    }
    const void* p[7] = {g.cover, g.top2, g.owner2, g.elig, g.elig_cnt, g.ovf, g.misfit};
    for (int i = 0; i < 7; ++i) out[i] = left_alone ? rel(p[i]) : -2;
    out[7] = (long long)c.off;
    return 8;
}
}

#ifdef GRID_SCRATCH_HOST_MAIN
// the arrays cut from an allocation of exactly the size the null-base run gives; every array written from its first to its last element
static bool walk(int B, int rows1, int rows2, bool bm, bool mf) {
    stvo::GridScratch g;
    stvo::Carver sizing(nullptr);
    stvo::carve_grid_scratch(sizing, g, B, rows1, rows2, bm, mf);
    std::vector<unsigned char> mem(sizing.off + 256);
    unsigned char* base = mem.data() + ((256 - reinterpret_cast<uintptr_t>(mem.data()) % 256) % 256);
    stvo::Carver c(base);
    stvo::carve_grid_scratch(c, g, B, rows1, rows2, bm, mf);
    const stvo::GridScratchCounts n = stvo::grid_scratch_counts(B, rows1, rows2, bm, mf);
    const stvo::GridMatrixDims d = stvo::grid_matrix_dims(rows1, rows2);
    if (bm) std::memset(g.cover, 0x11, (size_t)B * d.words() * 8);
    std::memset(g.top2, 0x22, (size_t)B * rows1 * 8);
    std::memset(g.owner2, 0x33, (size_t)B * rows2 * 4);
    std::memset(g.elig, 0x44, (size_t)B * stvo::GRID_ELIG * rows2 * 4);
    std::memset(g.elig_cnt, 0x55, (size_t)B * rows2 * 4);
    std::memset(g.ovf, 0x66, (size_t)B * 4);
    if (mf) std::memset(g.misfit, 0x77, (size_t)B * 4);
    bool ok = c.off == sizing.off && (bm ? g.cover != nullptr && n.cover == (size_t)B * d.words() : g.cover == nullptr && n.cover == 0);
    ok = ok && (mf ? g.misfit == g.ovf + B && n.ovf == stvo::grid_route_words(B) : g.misfit == nullptr && n.ovf == (size_t)B);
    // what was written last of each neighbour is still there: nothing overlapped
    ok = ok && *reinterpret_cast<unsigned char*>(g.top2) == 0x22 && *reinterpret_cast<unsigned char*>(g.owner2) == 0x33 &&
         *reinterpret_cast<unsigned char*>(g.elig) == 0x44 && *reinterpret_cast<unsigned char*>(g.elig_cnt) == 0x55 &&
         *reinterpret_cast<unsigned char*>(g.ovf) == 0x66 && (!bm || *reinterpret_cast<unsigned char*>(g.cover) == 0x11) &&
         (!mf || *reinterpret_cast<unsigned char*>(g.ovf + B - 1) == 0x66);
    return ok;
}

int main() {
    static const int shapes[][3] = {{1, 1, 1},      {1, 1, 65},      {1, 1, 2048},  {1, 64, 64},   {1, 128, 128}, {1, 2048, 2048}, {1, 2112, 2112},
                                    {3, 64, 2112},  {3, 2112, 128},  {16, 2048, 2048}, {3072, 64, 64}, {3072, 128, 64}};
    int bad = 0, n = 0;
    for (const auto& sh : shapes)
        for (int bm = 0; bm < 2; ++bm)
            for (int mf = 0; mf < 2; ++mf) {
                const bool ok = walk(sh[0], sh[1], sh[2], bm != 0, mf != 0);
                std::printf("B %4d rows %4d x %4d matrix %d misfit %d: %s\n", sh[0], sh[1], sh[2], bm, mf, ok ? "arrays inside" : "INCONSISTENT");
                bad += !ok; ++n;
            }
    std::printf("%d shapes, %d inconsistent\n", n, bad);
    return bad ? 1 : 0;
}
#endif
