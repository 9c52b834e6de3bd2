// track_update.h — one stream's feature identities advanced by one step: the chain that says "feature 17 of this frame is an observation
// of feature 5 of the last key-frame".  matchF2FPoints / matchF2FLines hand idx from the previous frame's feature to the current one
// (the reference's src/stereoFrameHandler.cpp:151,178), the stereo association numbers new features by position
// (src/stereoFrame.cpp:151,165,350,384) and currFrameIsKF renumbers at a key-frame (:1190-1218).  One text for the kernel
// (track_kernel.hip: a workgroup per stream, lane `first` of `stride`) and the host (tests/cpp/track_host.cpp: first = 0, stride = 1);
// points and key-lines run the same three phases on their own rows.
//   1  track_clear      win[i2] = -1 for the current features
//   2  track_vote       win[m12[i1]] = max(.., i1): the reference's ascending loop lets the LAST i1 that names an i2 win
//   3  track_write      the step's record of every current feature, and the state the next step propagates from
// The caller puts a barrier between the phases (the device) or runs them one after the other (the host).
#pragma once

#include <cstdint>

#include "../../include/stvo_types.h"

#if defined(__HIPCC__)
#define TRK_HD __host__ __device__ __forceinline__
#else
#define TRK_HD inline
#endif

namespace trk {

// what the step is for the stream: a tracked frame, the first frame of a sequence (`initialize`, also RESTART), or a parked frame
enum { MODE_RUN = 0, MODE_INIT = 1, MODE_PARK = 2 };

// a record as the one 8-byte word it is stored as (little endian: idx, age, kf, inlier)
TRK_HD unsigned long long track_pack(int32_t idx, uint32_t age, uint32_t kf, int32_t inlier) {
    return (unsigned long long)(uint32_t)idx | ((unsigned long long)(age & 0xFFFFu) << 32) | ((unsigned long long)(kf & 0xFFu) << 48) |
           ((unsigned long long)((uint32_t)inlier & 0xFFu) << 56);
}

TRK_HD void track_clear(int* win, int n_cur, int first, int stride) {
    for (int i = first; i < n_cur; i += stride) win[i] = -1;
}

TRK_HD void track_vote(int* win, const int32_t* m12, int n_prev, int n_cur, int first, int stride) {
    for (int i1 = first; i1 < n_prev; i1 += stride) {
        const int i2 = m12[i1];
        if (i2 < 0 || i2 >= n_cur) continue;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicMax(&win[i2], i1);  // LDS
#else
        if (i1 > win[i2]) win[i2] = i1;
#endif
    }
}

// mode != MODE_RUN: win is not read (nothing was voted).  reset: the frame is a key-frame (or a sequence's first frame) — the state carried
// on is numbered by position again, the record keeps the values from before.  inl may be null when mode != MODE_RUN.
// prev / rec / next: the stream's rows as 8-byte words; prev and next must not overlap.
TRK_HD void track_write(const int* win, const int32_t* inl, const unsigned long long* prev, int n_cur, int mode, bool reset,
                        unsigned long long* rec, unsigned long long* next, int first, int stride) {
    for (int i2 = first; i2 < n_cur; i2 += stride) {
        unsigned long long r;
        const int w = mode == MODE_RUN ? win[i2] : -1;
        if (w >= 0) {
            const unsigned long long p = prev[w];
            const uint32_t age = (uint32_t)(p >> 32) & 0xFFFFu;
            r = track_pack((int32_t)(uint32_t)p, age < 65535u ? age + 1u : 65535u, (uint32_t)(p >> 48) & 0xFFu, inl[w]);
        } else {
            r = track_pack(i2, 0u, mode == MODE_INIT ? 1u : 0u, -1);
        }
        rec[i2] = r;
        next[i2] = reset ? track_pack(i2, 0u, 1u, (int32_t)(int8_t)(r >> 56)) : r;
    }
}

// does the frame start a new numbering?  new_kf: the stream's trajectory record of this step (0 without the trajectory)
TRK_HD bool track_resets(int mode, int new_kf) { return mode == MODE_INIT || (mode == MODE_RUN && new_kf == 1); }

}  // namespace trk
