// traj_update.h — one stream's trajectory state advanced by one pose result: the "set estimated pose" block of optimizePose
// (the reference's src/stereoFrameHandler.cpp:372-391: Tfw, Tfw_cov) followed by the key-frame decision PL-SLAM drives on top of the
// odometry (needNewKF / currFrameIsKF, :1136-1218).  One text for the host mirror (host/keyframe.h forwards to kf_decide), the CPU
// tests (tests/cpp/traj_host.cpp) and the device (traj_kernel.hip, one lane per stream): the operations and their order are the same,
// what differs between the two builds is FMA contraction and the device's sin / cos / log / acos.
#pragma once

#include "pose_math.h"

namespace pm {

// what the decision compared, for the record and the host mirror's console line
struct KfTerms {
    double entropy_ratio, entropy_curr, det_acc, t, r;
};

PM_HD void identity6(double* C) {
#pragma unroll
    for (int i = 0; i < 36; ++i) C[i] = (i % 7 == 0) ? 1.0 : 0.0;
}

// the state as `initialize` leaves the handler (:35-51)
PM_HD void traj_init(stvo_traj_state& s) {
    identity4(s.Tfw);
    identity6(s.Tfw_cov);
    s.entropy_first_prevKF = 0.0;
    identity4(s.T_prevKF);
#pragma unroll
    for (int i = 0; i < 36; ++i) s.cov_prevKF_currF[i] = 0.0;
    s.prev_f_iskf = 1;
    s.N_prevKF_currF = 0;
    s.n_frames = 0;
    s.n_keyframes = 0;
}

// needNewKF (:1136-1188).  Tfw, DT, DT_cov are curr_frame's fields.  Returns true when a new key-frame is needed; otherwise counts
// the frame (N_prevKF_currF++).  The accumulated covariance is updated in both cases, like the original.
PM_HD bool kf_decide(int32_t& prev_f_iskf, double& entropy_first_prevKF, const double* T_prevKF, double* cov_prevKF_currF,
                     int32_t& N_prevKF_currF, const double* Tfw, const double* DT, const double* DT_cov, double min_entropy_ratio,
                     double max_kf_t_dist, double max_kf_r_dist, KfTerms& o) {
    const double kPi = 3.1415926535897932384626433832795;  // CV_PI
    const double two_pi_term = 3.0 * (1.0 + log(2.0 * acos(-1.0)));
    if (prev_f_iskf) {  // :1140-1153 — first frame after a key-frame fixes the reference entropy
        const double det = det6(DT_cov);
        entropy_first_prevKF = (det != 0.0) ? two_pi_term + 0.5 * log(det) : -999999999.99;
        prev_f_iskf = 0;
    }
    // geometric distance from the previous key-frame (:1156-1159)
    double Ti[16], D[16], dX[6];
    inverse_se3(Tfw, Ti);
    mat4_mul(Ti, T_prevKF, D);
    logmap_se3(D, dX);
    o.t = sqrt(dX[0] * dX[0] + dX[1] * dX[1] + dX[2] * dX[2]);
    o.r = sqrt(dX[3] * dX[3] + dX[4] * dX[4] + dX[5] * dX[5]) * 180.f / kPi;
    // accumulated covariance from the previous key-frame (:1162-1166)
    double A[36], cinv[36], tmp[36];
    adjoint_se3(T_prevKF, A);
    uncTinv_se3(DT, DT_cov, cinv);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) s += A[i * 6 + q] * cinv[q * 6 + j];
            tmp[i * 6 + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) s += tmp[i * 6 + q] * A[j * 6 + q];
            cov_prevKF_currF[i * 6 + j] += s;
        }
    o.det_acc = det6(cov_prevKF_currF);
    o.entropy_curr = two_pi_term + 0.5 * log(o.det_acc);
    o.entropy_ratio = o.entropy_curr / entropy_first_prevKF;
    bool zero_cov = true, ident = true;
#pragma unroll
    for (int i = 0; i < 36; ++i) zero_cov = zero_cov && DT_cov[i] == 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) ident = ident && DT[i] == ((i % 5 == 0) ? 1.0 : 0.0);
    // :1173-1175
    if (o.entropy_ratio < min_entropy_ratio || __builtin_isnan(o.entropy_ratio) || __builtin_isinf(o.entropy_ratio) ||
        (zero_cov && ident) || o.t > max_kf_t_dist || o.r > max_kf_r_dist || N_prevKF_currF > 10)
        return true;
    N_prevKF_currF++;
    return false;
}

// the state part of currFrameIsKF (:1209-1216) for a key-frame whose pose is Tfw_of_new_kf
PM_HD void kf_restart(int32_t& prev_f_iskf, double* T_prevKF, double* cov_prevKF_currF, int32_t& N_prevKF_currF, const double* Tfw_of_new_kf) {
#pragma unroll
    for (int i = 0; i < 16; ++i) T_prevKF[i] = Tfw_of_new_kf[i];
#pragma unroll
    for (int i = 0; i < 36; ++i) cov_prevKF_currF[i] = 0.0;
    prev_f_iskf = 1;
    N_prevKF_currF = 0;
}

// One frame: publishPose's pose block (host/stereoFrameHandler.cpp), the record the app writes, then — with prm.keyframes — needNewKF
// and, when it says so, currFrameIsKF: the map frame restarts at this frame (Tfw = I, Tfw_cov = I) for the frames that follow.
// T / cov / status are the fields of the stream's stvo_pose_result; rec may be null.
PM_HD void traj_update(stvo_traj_state& s, const double* T, const double* cov, int32_t status, const stvo_traj_params& prm,
                       stvo_traj_record* rec) {
    double DT[16], DT_cov[36];
    if (status == STVO_POSE_OK) {  // :372-381
#pragma unroll
        for (int i = 0; i < 16; ++i) DT[i] = T[i];
#pragma unroll
        for (int i = 0; i < 36; ++i) DT_cov[i] = cov[i];
        double prod[16], x[6], Tn[16], Cn[36];
        mat4_mul(s.Tfw, DT, prod);
        logmap_se3(prod, x);
        expmap_se3(x, Tn);  // :377
        unccomp_se3(s.Tfw, s.Tfw_cov, DT_cov, Cn);
#pragma unroll
        for (int i = 0; i < 16; ++i) s.Tfw[i] = Tn[i];
#pragma unroll
        for (int i = 0; i < 36; ++i) s.Tfw_cov[i] = Cn[i];
    } else {  // :382-391 — DT = I, DT_cov = 0, the pose of the previous frame carried over
        identity4(DT);
#pragma unroll
        for (int i = 0; i < 36; ++i) DT_cov[i] = 0.0;
    }
    s.n_frames++;
    if (rec) {  // the pose of this frame, before any reset
#pragma unroll
        for (int i = 0; i < 16; ++i) rec->Tfw[i] = s.Tfw[i];
#pragma unroll
        for (int i = 0; i < 36; ++i) rec->Tfw_cov[i] = s.Tfw_cov[i];
    }
    KfTerms k{0.0, 0.0, 0.0, 0.0, 0.0};
    int32_t new_kf = 0;
    if (prm.keyframes) {
        new_kf = kf_decide(s.prev_f_iskf, s.entropy_first_prevKF, s.T_prevKF, s.cov_prevKF_currF, s.N_prevKF_currF, s.Tfw, DT, DT_cov,
                           prm.min_entropy_ratio, prm.max_kf_t_dist, prm.max_kf_r_dist, k)
                     ? 1 : 0;
        if (new_kf) {
            identity4(s.Tfw);
            identity6(s.Tfw_cov);
            kf_restart(s.prev_f_iskf, s.T_prevKF, s.cov_prevKF_currF, s.N_prevKF_currF, s.Tfw);
            s.n_keyframes++;
        }
    }
    if (rec) {
        rec->entropy_ratio = k.entropy_ratio;
        rec->t = k.t;
        rec->r = k.r;
        rec->new_kf = new_kf;
        rec->frame = s.n_frames;
    }
}

}  // namespace pm
