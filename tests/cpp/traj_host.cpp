// traj_host.cpp — TEST INFRASTRUCTURE ONLY: exposes the product's traj_update.h (the text the trajectory kernel runs per stream)
// to the CPU test-suite and to tools/bench_trajectory.py's host leg.  Not part of the product library.
#include "../../stvo-pl_amd/csrc/traj_update.h"

extern "C" {
void trh_sizes(int* out3) {
    out3[0] = (int)sizeof(stvo_traj_params);
    out3[1] = (int)sizeof(stvo_traj_state);
    out3[2] = (int)sizeof(stvo_traj_record);
}
void trh_init(int B, stvo_traj_state* state) {
    for (int b = 0; b < B; ++b) pm::traj_init(state[b]);
}
// one update of B streams, stream after stream: what the kernel does with one lane each
void trh_update(int B, const stvo_pose_result* results, const stvo_traj_params* prm, stvo_traj_state* state, stvo_traj_record* records) {
    for (int b = 0; b < B; ++b) pm::traj_update(state[b], results[b].T, results[b].cov, results[b].status, *prm, records ? records + b : nullptr);
}
}
