// The host-side decisions of the rectify / colour entry points (stvo-pl_amd/csrc/rectify_bank_plan.h: the chunking rule;
// rectify_internal.h: the grey weight sets and the range checks), run without a device — TEST INFRASTRUCTURE ONLY.  A stand-alone
// program: tests/test_rectify_host_decisions.py builds it with g++ (rectify_internal.h includes the HIP headers; g++ reads them in host
// mode and nothing of the runtime is called or linked) under AddressSanitizer and UBSan and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../stvo-pl_amd/csrc/rectify_bank_plan.h"
#include "../../stvo-pl_amd/csrc/rectify_internal.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            if (++failures <= 20) {       \
                std::printf("FAILED %s: ", #cond); \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

// The uniform launch's grid as it was written in launch_remap and launch_rect_ch before they called rbank_chunks.
static void uniform_formula(int bx, int n, int* gy, int* per_chunk) {
    const int want = std::max(1, (256 * 8 + 2 * bx - 1) / (2 * bx));
    const int chunks = std::max(1, std::min(want, (n + 3) / 4));
    *per_chunk = (n + chunks - 1) / chunks;
    *gy = (n + *per_chunk - 1) / *per_chunk;
}

static void chunking() {
    for (int bx = 1; bx <= 2048; ++bx)
        for (int n = 1; n <= 600; ++n) {
            int gy = 0, per = 0, per_shared = 0;
            uniform_formula(bx, n, &gy, &per);
            const int gy_shared = stvo::rbank_chunks(bx, n, &per_shared);
            EXPECT(gy_shared == gy && per_shared == per, "bx %d n %d: (%d, %d) against (%d, %d)", bx, n, gy_shared, per_shared, gy, per);
            EXPECT(per >= 1 && (long long)gy * per >= n && (long long)(gy - 1) * per < n, "bx %d n %d: the chunks do not cover", bx, n);
        }
}

static void weights() {
    struct Want { int order, set; uint32_t w0, w1, w2, rnd, shift; };
    const Want want[4] = {{STVO_ORDER_BGR, STVO_GRAY_Q14, 1868u, 9617u, 4899u, 1u << 13, 14u},
                          {STVO_ORDER_RGB, STVO_GRAY_Q14, 4899u, 9617u, 1868u, 1u << 13, 14u},
                          {STVO_ORDER_BGR, STVO_GRAY_Q15, 3735u, 19235u, 9798u, 1u << 14, 15u},
                          {STVO_ORDER_RGB, STVO_GRAY_Q15, 9798u, 19235u, 3735u, 1u << 14, 15u}};
    for (int order = -2; order <= 3; ++order)
        for (int set = -2; set <= 3; ++set) {
            stvo_detail::GrayWeights w{7u, 7u, 7u, 7u, 7u};
            const bool ok = stvo_detail::gray_weights(order, set, &w);
            const Want* m = nullptr;
            for (const Want& k : want)
                if (k.order == order && k.set == set) m = &k;
            EXPECT(ok == (m != nullptr), "order %d set %d: %s", order, set, ok ? "accepted" : "refused");
            if (ok && m) {
                EXPECT(w.w0 == m->w0 && w.w1 == m->w1 && w.w2 == m->w2 && w.rnd == m->rnd && w.shift == m->shift, "order %d set %d", order, set);
                EXPECT(w.w0 + w.w1 + w.w2 == 1u << w.shift, "order %d set %d: the weights do not sum to one", order, set);
            }
        }
}

// Ranges inside one real allocation, so that every address compared exists.
static void ranges() {
    using stvo_detail::gray_planes_ok;
    using stvo_detail::stereo_ranges_ok;
    unsigned char* base = static_cast<unsigned char*>(std::malloc(4096));
    const size_t n = 100;
    // offsets of dst_l, dst_r, src_l, src_r ([o, o + 100) each); accepted
    struct Four { size_t dl, dr, sl, sr; bool ok; };
    const Four four[] = {
        {0, 100, 200, 300, true},      // touching, in order
        {300, 200, 100, 0, true},      // touching, reversed
        {0, 1000, 2000, 3000, true},   // disjoint
        {0, 100, 200, 250, true},      // the sources overlap each other: nothing is written there
        {0, 101, 200, 300, false},     // dst_r reaches one byte into src_l
        {0, 100, 199, 300, false},     // the first byte of src_l is the last of dst_r
        {99, 200, 0, 300, false},      // the first byte of dst_l is the last of src_l
        {0, 99, 200, 300, false},      // the first byte of dst_r is the last of dst_l
        {100, 200, 300, 1, false},     // the first byte of dst_l is the last of src_r
        {200, 0, 300, 99, false},      // the last byte of dst_r is the first of src_r
        {0, 0, 200, 300, false},       // the same destination twice
        {200, 300, 200, 400, false},   // in place
    };
    for (const Four& f : four)
        EXPECT(stereo_ranges_ok(base + f.dl, base + f.dr, base + f.sl, base + f.sr, n) == f.ok, "dst %zu %zu src %zu %zu", f.dl, f.dr, f.sl, f.sr);
    EXPECT(stereo_ranges_ok(base, base + 1, base + 2, base + 3, 1), "one byte each, touching");
    EXPECT(!stereo_ranges_ok(base, base + 1, base + 1, base + 3, 1), "one byte each, dst_r on src_l");

    // planes of px bytes, sources of sb bytes
    const size_t px = 100, sb = 300;
    struct Planes { size_t p[4]; int np; size_t sl, sr; bool ok; };
    const Planes planes[] = {
        {{0, 100, 200, 300}, 4, 400, 700, true},     // all touching
        {{0, 100, 0, 0}, 2, 200, 500, true},         // two planes: the other two entries are not read
        {{1000, 2000, 3000, 3500}, 4, 0, 400, true}, // disjoint
        {{0, 100, 200, 300}, 4, 399, 700, false},    // the last byte of plane 3 is the first of src_l
        {{300, 100, 200, 0}, 4, 400, 700, true},     // any order
        {{699, 100, 200, 300}, 4, 400, 800, false},  // the first byte of plane 0 is the last of src_l
        {{0, 99, 200, 300}, 4, 400, 700, false},     // plane 1 over the last byte of plane 0
        {{0, 100, 200, 299}, 4, 400, 700, false},    // plane 3 over the last byte of plane 2
        {{0, 100, 200, 299}, 2, 400, 700, true},     // ... which two planes do not read
        {{500, 100, 200, 300}, 4, 400, 700, false},  // plane 0 nested in src_l
        {{0, 100, 200, 300}, 4, 400, 1, false},      // src_r [1, 301) over three planes
        {{0, 0, 200, 300}, 4, 400, 700, false},      // the same plane twice
    };
    for (const Planes& c : planes) {
        const uint8_t* p[4] = {base + c.p[0], base + c.p[1], base + c.p[2], base + c.p[3]};
        EXPECT(gray_planes_ok(p, c.np, px, base + c.sl, base + c.sr, sb) == c.ok, "planes %zu %zu %zu %zu (%d) src %zu %zu", c.p[0], c.p[1], c.p[2],
               c.p[3], c.np, c.sl, c.sr);
    }
    std::free(base);
}

int main() {
    chunking();
    weights();
    ranges();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
