// pose_args.h — between pose_kernel.hip and pose_kernel2p.hip only: the ONE flat by-value argument of the pose kernels.  The host
// surface is in parts (kernels.h: PoseProblem, PosePoints, PoseOptions); launch_pose copies them in here once per launch.  Fields,
// order and type name are what the kernels were compiled against: pose2c_kernel reads its arguments from the kernel-argument segment
// by offset, a nested struct would move every kernel by a few instructions, and traces match the mangled names.
#pragma once

#include "kernels.h"

namespace stvo {

struct PoseArgs {
    int B, max_pts, max_lines;
    const int32_t* n_prev_pts;
    const double* prev_P;
    const double* prev_s2p;
    const double* curr_pl;
    const int32_t* m12p;
    const int32_t* init_inl_p;
    const int32_t* n_prev_lines;
    const double* prev_sP;
    const double* prev_eP;
    const double* prev_spl;
    const double* prev_epl;
    const double* prev_s2l;
    const double* curr_le;
    const int32_t* m12l;
    const int32_t* init_inl_l;
    const double* init_T;
    double* next_T;
    stvo_cam cam;
    const stvo_cam* cams;
    stvo_opt_params prm;
    stvo_pose_result* results;
    int32_t* inl_p_out;
    int32_t* inl_l_out;
    int eval_only;  // 1: PoseOptions::eval_out is present
    int eval_robust;
    double* eval_out;
    long long* prof_out;
    const float4* prev_rc;
    const float4* curr_rc;
    const double* q_tab;
    double level_scale;
    const unsigned* wait_flag;
    unsigned wait_value;
    int lazy_eig;
    // != 0 (launch_pose's own decision for the latency kernel; STVO_POSE_LOS=0 clears it): frame pairs with at most 64 LPT key-lines
    // have them evaluated by the solver wave (pose_kernel.hip)
    int lines_on_solver;
    const uint4* fetch_src;
    uint4* fetch_dst;
    unsigned fetch_n16;
    unsigned* fetch_flag;
    unsigned fetch_value;
    unsigned* start_flag;
    unsigned start_value;
};

// pose_kernel2p.hip: thread-private records, `waves` (2 or 4) per frame pair; arena: B * pose_arena_pair_words 16-byte words
int launch_pose2p(hipStream_t s, const PoseArgs& a, int waves, double2* arena);

}  // namespace stvo
