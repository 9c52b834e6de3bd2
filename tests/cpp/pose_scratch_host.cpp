// The route of a pose launch and the arena of the batch kernels (stvo-pl_amd/csrc/pose_scratch.h) behind a flat C interface — TEST
// INFRASTRUCTURE ONLY.  tests/test_pose_scratch_host.py holds it against a plain statement of the route and the sizes.  Built by g++
// alone: the header includes nothing of HIP.
#include <climits>
#include <cstring>

#include "../../stvo-pl_amd/csrc/pose_scratch.h"

extern "C" {

int psh_unset() { return stvo::DBG_UNSET; }

// out: batch, waves, inline_sync, start_flag, arena_bytes.  Every switch but the two the route reads is left unset.
int psh_route(int B, int compact, int eval, int cus, int pose_kernel, int pose2p_nw, long long* out) {
    stvo::DebugSwitches sw;
    int* w = reinterpret_cast<int*>(&sw);
    for (size_t i = 0; i < sizeof(sw) / sizeof(int); ++i) w[i] = stvo::DBG_UNSET;
    sw.pose_kernel = pose_kernel;
    sw.pose2p_nw = pose2p_nw;
    const stvo::PoseRoute r = stvo::pose_route(B, compact != 0, eval != 0, cus, sw);
    out[0] = r.batch; out[1] = r.waves; out[2] = r.inline_sync; out[3] = r.start_flag; out[4] = (long long)r.arena_bytes;
    return 5;
}

// 16-byte words of arena per frame pair; the bytes of a word
long long psh_pair_words(int compact) { return (long long)stvo::pose_arena_pair_words(compact != 0); }
int psh_word_bytes() { return (int)stvo::POSE_ARENA_WORD_BYTES; }
int psh_max_points() { return STVO_POSE_MAX_POINTS; }
int psh_max_lines() { return STVO_POSE_MAX_LINES; }
}
