// Writes what csrc/orb_pattern.h derives, for tests/test_orb_wta_host.py to hold against the numpy statement (tests/np_orb_wta.py):
//   pattern <wta_k> <P> <n_points> <2048 hex digits>     the effective pattern of every wta_k 2 .. 4 and patch size 2 .. 63
//   geometry <P> <half patch> <reach> <umax[0 .. half patch]>
//   verdict <wta_k> <P> <verdict>                            settings outside the built range, and pools a tuple cannot be drawn from
// The pool of patch size 31 is the seeded stand-in.  A stand-alone program: it is built with the host compiler (once more with
// -fsanitize=address,undefined) and run as a process of its own.
#include <cstdio>

#include "../../stvo-pl_amd/csrc/orb_pattern.h"

int main() {
    for (int wta = 2; wta <= 4; ++wta)
        for (int P = 2; P <= 63; ++P) {
            int8_t out[1024];
            for (int i = 0; i < 1024; ++i) out[i] = 99;
            int n = -1;
            const int v = stvo::orb_effective_pattern(wta, P, nullptr, out, &n);
            if (v != stvo::ORB_PATTERN_OK) {
                std::printf("failed %d %d %d\n", wta, P, v);
                return 1;
            }
            std::printf("pattern %d %d %d ", wta, P, n);
            for (int i = 0; i < 1024; ++i) std::printf("%02x", (unsigned)(uint8_t)out[i]);
            std::printf("\n");
        }
    for (int P = 2; P <= 63; ++P) {
        int u[stvo::ORB_MAX_HALF_PATCH + 2];
        const int h = stvo::orb_half_patch(P);
        stvo::orb_umax(h, u);
        std::printf("geometry %d %d %d", P, h, stvo::orb_reach(P));
        for (int v = 0; v <= h; ++v) std::printf(" %d", u[v]);
        std::printf("\n");
    }
    const int bad[][2] = {{1, 31}, {5, 31}, {0, 31}, {-2, 31}, {2, 1}, {2, 0}, {3, -7}, {4, 64}, {2, 64}, {3, 1000}, {5, 64}, {1, 1}};
    for (const auto& b : bad) {
        int8_t out[1024];
        for (int i = 0; i < 1024; ++i) out[i] = 99;
        int n = -1;
        const int v = stvo::orb_effective_pattern(b[0], b[1], nullptr, out, &n);
        bool untouched = n == -1;
        for (int i = 0; i < 1024; ++i) untouched = untouched && out[i] == 99;
        std::printf("verdict %d %d %d %d\n", b[0], b[1], v, (int)untouched);
    }
    {   // pools of patch size 31: out of range; one, two and three different points under wta_k 2, 3, 4
        int8_t pool[1024], out[1024];
        for (int i = 0; i < 1024; ++i) pool[i] = 0;
        pool[7] = 14;
        std::printf("pool range %d\n", stvo::orb_effective_pattern(2, 31, pool, out, nullptr));
        for (int distinct = 1; distinct <= 4; ++distinct) {
            for (int i = 0; i < 512; ++i) {
                pool[2 * i] = (int8_t)(i % distinct);
                pool[2 * i + 1] = (int8_t)(-(i % distinct));
            }
            for (int wta = 2; wta <= 4; ++wta) std::printf("pool distinct %d %d %d\n", distinct, wta, stvo::orb_effective_pattern(wta, 31, pool, out, nullptr));
        }
    }
    return 0;
}
