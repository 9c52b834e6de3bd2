// pose_scratch.h — the route of a pose launch and the record arena of the batch kernels, stated ONCE: which kernel a launch of B frame
// pairs takes, with how many waves per pair, which in-kernel ordering devices it honours, and how many bytes of arena it works in.
// launch_pose (pose_kernel.hip) and the step's fact gathering (seq_pipeline.hip) both ask pose_route; the owner of the arena (the
// context: ctx_internal.h) sizes its block by the same answer.  Host-pure: g++ alone compiles it; tests/cpp/pose_scratch_host.cpp runs
// everything here without a device.
#pragma once

#include <cstddef>

#include "../../include/stvo_hip.h"
#include "debug_switches.h"

namespace stvo {

constexpr int POSE_LATENCY_MAX_B = 256;      // the latency kernel has a CU per frame pair up to here
constexpr int POSE_INLINE_SYNC_MAX_B = 16;   // few workgroups: the kernels an in-kernel wait is for always find CUs

// The arena of the batch kernels (pose_kernel2p.hip), in 16-byte words per frame pair: seven parts per key-line, and three per stereo
// point when the points come as doubles (compact records stay on chip).  A thread's records are planes [ordinal][part][thread] of a
// whole workgroup, so the count is LPT * 7 * BLOCK + PPT * 3 * BLOCK — the same for two and four waves per pair.
constexpr size_t POSE_ARENA_WORD_BYTES = 16;
constexpr size_t pose_arena_pair_words(bool compact) {
    return (size_t)7 * STVO_POSE_MAX_LINES + (compact ? (size_t)0 : (size_t)3 * STVO_POSE_MAX_POINTS);
}

struct PoseRoute {
    bool batch;          // pose_kernel2p.hip (pose2c_kernel on compact records, pose2p_kernel on doubles); false: the latency kernel
    int waves;           // per frame pair of the batch kernel, 2 or 4; 0 on the latency route
    bool inline_sync;    // PoseSync::wait_flag / fetch_* may be used (the latency kernel honours them)
    bool start_flag;     // PoseSync::start_flag is honoured (pose2c_kernel only)
    size_t arena_bytes;  // what the launch needs of its arena; 0 on the latency route
};

// The latency kernel up to 256 frame pairs and for single evaluations, the batch kernel beyond; STVO_POSE_KERNEL = 1 / 4 force either
// for every batch size.
inline bool pose_takes_batch_kernel(int B, bool eval, const DebugSwitches& sw) {
    return !eval && (sw.pose_kernel == 4 || (sw.pose_kernel != 1 && B > POSE_LATENCY_MAX_B));
}

// compact: the stereo points come as compact records; eval: a single evaluation; cus: CUs of the device (read on the batch route only).
// Waves per frame pair: two (four pairs per CU) once the batch holds more than two pairs per CU, four (two pairs per CU, half as many
// records per thread) below that — with 512 pairs on 256 CUs the two-wave variant leaves half of every CU's wave slots empty (configs[3]
// leg, 512 streams: 701 k vs 774 k frame pairs/s).  STVO_POSE2P_NW overrides (developer).
inline PoseRoute pose_route(int B, bool compact, bool eval, int cus, const DebugSwitches& sw) {
    PoseRoute r;
    r.batch = pose_takes_batch_kernel(B, eval, sw);
    r.waves = !r.batch ? 0 : sw.pose2p_nw > 0 ? (sw.pose2p_nw >= 4 ? 4 : 2) : (B > 2 * cus ? 2 : 4);
    r.inline_sync = B >= 1 && B <= POSE_INLINE_SYNC_MAX_B && sw.pose_kernel != 4;
    r.start_flag = B > 0 && compact && r.batch;
    r.arena_bytes = r.batch && B > 0 ? (size_t)B * pose_arena_pair_words(compact) * POSE_ARENA_WORD_BYTES : 0;
    return r;
}

}  // namespace stvo
