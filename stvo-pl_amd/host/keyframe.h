// keyframe.h — the key-frame decision of StVO::StereoFrameHandler (the "slam functions" of
// /root/reference/src/stereoFrameHandler.cpp:1134-1218, used by PL-SLAM on top of PL-StVO), as plain host
// code with no GPU dependency: state (include/stereoFrameHandler.h:81-85) + needNewKF + currFrameIsKF.
// SURVEY.md §8f rank 2.  The handler mirror forwards to these; tests/test_pose_math_host.py checks them
// against a numpy model without a GPU.
#pragma once

#include <cmath>
#include <iostream>

#include "../csrc/traj_update.h"
#include "stvo_compat.h"

namespace StVO {

struct KeyFrameState {
    bool prev_f_iskf = true;                       // stereoFrameHandler.cpp:50
    double entropy_first_prevKF = 0.0;
    Matrix4d T_prevKF = Matrix4d::Identity();      // :48
    Matrix6d cov_prevKF_currF = Matrix6d::Zero();  // :49
    int N_prevKF_currF = 0;                        // :51
};

// needNewKF (:1136-1188).  Tfw, DT, DT_cov are curr_frame's fields.  Returns true when a new key-frame is needed;
// otherwise counts the frame (N_prevKF_currF++).  The accumulated covariance is updated in both cases, like the original.
// The rule itself is pm::kf_decide (csrc/traj_update.h), the text the device runs per stream.
inline bool kf_need_new(KeyFrameState& k, const Matrix4d& Tfw, const Matrix4d& DT, const Matrix6d& DT_cov,
                        double min_entropy_ratio, double max_kf_t_dist, double max_kf_r_dist, bool verbose = true) {
    int32_t iskf = k.prev_f_iskf ? 1 : 0, N = k.N_prevKF_currF;
    pm::KfTerms o;
    const bool need = pm::kf_decide(iskf, k.entropy_first_prevKF, k.T_prevKF.m, k.cov_prevKF_currF.m, N, Tfw.m, DT.m, DT_cov.m,
                                    min_entropy_ratio, max_kf_t_dist, max_kf_r_dist, o);
    k.prev_f_iskf = iskf != 0;
    if (verbose) {
        if (need)
            std::cout << std::endl << "Entropy ratio: " << o.entropy_ratio << "\t" << o.t << " " << o.r << " " << k.N_prevKF_currF << std::endl;
        else
            std::cout << std::endl << "No new KF needed: " << o.entropy_ratio << "\t" << o.entropy_curr << " " << k.entropy_first_prevKF << " "
                      << o.det_acc << "\t" << o.t << " " << o.r << " " << k.N_prevKF_currF << std::endl << std::endl;
    }
    k.N_prevKF_currF = N;
    return need;
}

// the state part of currFrameIsKF (:1209-1216); the caller resets the feature indices and the frame pose
inline void kf_reset(KeyFrameState& k, const Matrix4d& Tfw_of_new_kf) {
    int32_t iskf, N;
    pm::kf_restart(iskf, k.T_prevKF.m, k.cov_prevKF_currF.m, N, Tfw_of_new_kf.m);
    k.prev_f_iskf = iskf != 0;
    k.N_prevKF_currF = N;
}

}  // namespace StVO
