// track_host_main.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the product's track_update.h on seeded random cases
// against an ascending loop written out here, with buffers sized exactly to the counts — built with -fsanitize=address,undefined by
// tests/test_tracks_host.py, so that a read or write outside rows [0, n) ends the program.  Exit status 0: every case agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "track_host.cpp"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

static int run_case(int n_prev, int n_cur, int mode, int new_kf, int lanes, bool saturate) {
    std::vector<int32_t> m12((size_t)n_prev), inl((size_t)n_prev);
    std::vector<stvo_track> prev((size_t)n_prev), rec((size_t)n_cur), next((size_t)n_cur), want((size_t)n_cur), want_next((size_t)n_cur);
    for (int i = 0; i < n_prev; ++i) {
        // about half of the previous features matched, into a third of the current ones: duplicates are the rule
        m12[i] = (n_cur > 0 && (rnd() & 1)) ? (int32_t)(rnd() % (unsigned)((n_cur + 2) / 3)) : -1;
        inl[i] = (int32_t)(rnd() % 3) - 1;
        prev[i].idx = (int32_t)(rnd() % 5000);
        prev[i].age = saturate ? (uint16_t)(65533 + rnd() % 3) : (uint16_t)(rnd() % 100);
        prev[i].kf = (uint8_t)(rnd() & 1);
        prev[i].inlier = (int8_t)((int)(rnd() % 3) - 1);
    }
    for (int i = 0; i < n_cur; ++i) {
        want[i].idx = i; want[i].age = 0; want[i].kf = mode == trk::MODE_INIT ? 1 : 0; want[i].inlier = -1;
    }
    if (mode == trk::MODE_RUN)
        for (int i1 = 0; i1 < n_prev; ++i1) {
            const int i2 = m12[i1];
            if (i2 < 0 || i2 >= n_cur) continue;
            want[i2].idx = prev[i1].idx;
            want[i2].age = prev[i1].age == 65535 ? 65535 : (uint16_t)(prev[i1].age + 1);
            want[i2].kf = prev[i1].kf;
            want[i2].inlier = (int8_t)inl[i1];
        }
    const bool reset = mode == trk::MODE_INIT || (mode == trk::MODE_RUN && new_kf == 1);
    for (int i = 0; i < n_cur; ++i) {
        want_next[i] = want[i];
        if (reset) { want_next[i].idx = i; want_next[i].age = 0; want_next[i].kf = 1; }
    }
    const int got_reset = tkh_step(n_prev, m12.data(), inl.data(), prev.data(), n_cur, mode, new_kf, rec.data(), next.data(), lanes);
    if (got_reset != (reset ? 1 : 0)) return 1;
    if (n_cur && (std::memcmp(rec.data(), want.data(), (size_t)n_cur * sizeof(stvo_track)) || std::memcmp(next.data(), want_next.data(), (size_t)n_cur * sizeof(stvo_track))))
        return 1;
    return 0;
}

int main() {
    const int counts[] = {0, 1, 63, 64, 65, 300, 512, 2048};
    int bad = 0, cases = 0;
    for (int np : counts)
        for (int nc : counts)
            for (int mode = 0; mode < 3; ++mode)
                for (int new_kf = 0; new_kf < 2; ++new_kf) {
                    bad += run_case(np, nc, mode, new_kf, (cases % 3 == 0) ? 1 : ((cases % 3 == 1) ? 64 : 256), (cases & 7) == 0);
                    ++cases;
                }
    std::printf("track_host_main: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
