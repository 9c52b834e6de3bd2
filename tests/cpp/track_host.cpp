// track_host.cpp — TEST INFRASTRUCTURE ONLY: exposes the product's track_update.h (the text the track kernel runs per stream) to the CPU
// test-suite and to tools/bench_tracks.py's host leg.  Not part of the product library.
#include <cstddef>
#include <vector>

#include "../../stvo-pl_amd/csrc/track_update.h"

extern "C" {
void tkh_sizes(int* out2) {
    out2[0] = (int)sizeof(stvo_track);
    out2[1] = (int)sizeof(stvo_kf_header);
}
// One stream, one feature kind, the three phases as `lanes` lanes would run them (lane after lane, phase after phase).  prev / m12 / inl:
// n_prev rows; rec / next: rows [0, n_cur) are written.  mode: trk::MODE_*; returns whether the frame resets the numbering.
int tkh_step(int n_prev, const int32_t* m12, const int32_t* inl, const stvo_track* prev, int n_cur, int mode, int new_kf, stvo_track* rec,
             stvo_track* next, int lanes) {
    typedef unsigned long long u64;
    std::vector<int> win((size_t)(n_cur > 0 ? n_cur : 1), 12345);
    const bool reset = trk::track_resets(mode, new_kf);
    if (mode == trk::MODE_RUN) {
        for (int l = 0; l < lanes; ++l) trk::track_clear(win.data(), n_cur, l, lanes);
        for (int l = 0; l < lanes; ++l) trk::track_vote(win.data(), m12, n_prev, n_cur, l, lanes);
    }
    for (int l = 0; l < lanes; ++l)
        trk::track_write(win.data(), inl, reinterpret_cast<const u64*>(prev), n_cur, mode, reset, reinterpret_cast<u64*>(rec),
                         reinterpret_cast<u64*>(next), l, lanes);
    return reset ? 1 : 0;
}
// B streams of capacity `cap` one after the other on one core: the host alternative the benchmark times
void tkh_step_batch(int B, int cap, const int32_t* n_prev, const int32_t* m12, const int32_t* inl, const stvo_track* prev, const int32_t* n_cur,
                    stvo_track* rec, stvo_track* next) {
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * cap;
        tkh_step(n_prev[b], m12 + o, inl + o, prev + o, n_cur[b], trk::MODE_RUN, 0, rec + o, next + o, 1);
    }
}
}
