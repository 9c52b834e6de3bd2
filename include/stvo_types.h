/*
 * stvo_types.h — plain-C data records shared by the C-ABI (stvo_hip.h), the host-side
 * mirror of the reference classes, and the test oracle.  POD only: no torch, no C++.
 *
 * Conventions (all follow the reference, /root/reference):
 *   - 4x4 / 6x6 matrices are row-major doubles.
 *   - se(3) twists are ordered (t, w): head(3) translation, tail(3) rotation
 *     (src/auxiliar.cpp:124-141).
 *   - Binary descriptors are N x 32 bytes, contiguous (ORB 256 bit, LBD 256 bit;
 *     src/stereoFrame.cpp:112-115, 3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:639).
 *   - The stereo bucketing grid is 64 columns x 48 rows (include/stereoFrame.h:51-52).
 */
#ifndef STVO_TYPES_H
#define STVO_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STVO_DESC_BYTES 32
#define STVO_GRID_COLS 64 /* include/stereoFrame.h:52 */
#define STVO_GRID_ROWS 48 /* include/stereoFrame.h:51 */
#define STVO_GRID_CELLS (STVO_GRID_COLS * STVO_GRID_ROWS)

/* Pinhole stereo camera scalars read by the path (src/pinholeStereoCamera.cpp:221-237). */
typedef struct stvo_cam {
    double fx, fy, cx, cy, b;
} stvo_cam;

/* GridWindow (include/gridStructure.h:37-39): cells [x-w_lo .. x+w_hi] x [y-h_lo .. y+h_hi]. */
typedef struct stvo_grid_window {
    int32_t w_lo, w_hi, h_lo, h_hi;
} stvo_grid_window;

/* Optimizer parameters = the Config scalars optimizePose reads (src/config.cpp:80-86,
 * include/config.h:39-105).  `mode` is the local constant of stereoFrameHandler.cpp:329
 * (0 GN, 1 robust GN, 2 LM) exposed as a parameter; the reference hard-codes 0. */
typedef struct stvo_opt_params {
    int32_t mode;
    int32_t has_points;
    int32_t has_lines;
    int32_t min_features;
    int32_t max_iters;
    int32_t max_iters_ref;
    int32_t reserved0;
    int32_t reserved1;
    double homog_th;
    double min_error;
    double min_error_change;
    double inlier_k;
} stvo_opt_params;

/* Matching / stereo-association parameters (src/config.cpp:49-69,91). */
typedef struct stvo_match_params {
    int32_t best_lr_matches;
    int32_t matching_s_ws;
    float   min_ratio_12_p; /* passed as float to match() (src/matching.cpp:63) */
    float   min_ratio_12_l;
    double  max_dist_epip;
    double  min_disp;
    double  line_sim_th;
    double  stereo_overlap_th;
    double  line_horiz_th;
    double  ls_min_disp_ratio;
    double  orb_scale_factor;
    double  lsd_scale;
    /* Config::minRatio12P() as the DOUBLE both matchGrid overloads compare with (src/matching.cpp:160,241), used by the
     * stereo stage of the stvo_seq_* pipeline; 0 = (double)min_ratio_12_p.  (match() takes the ratio as float,
     * src/matching.cpp:63, so the f2f stage keeps the float fields above.) */
    double  min_ratio_12_p_d;
} stvo_match_params;

/* Status of one optimizePose call (the in-band failure modes of
 * src/stereoFrameHandler.cpp:332-391). */
enum {
    STVO_POSE_OK = 0,                  /* committed: good solution and DT != I           (:372-381) */
    STVO_POSE_FEW_INLIERS_BEFORE = 1,  /* n_inliers < minFeatures before optimisation    (:364-368) */
    STVO_POSE_FEW_INLIERS_AFTER = 2,   /* n_inliers < minFeatures after removeOutliers   (:351-355) */
    STVO_POSE_REJECTED = 3,            /* isGoodSolution false or DT == I at commit      (:382-391) */
    STVO_POSE_INTERNAL = 4             /* device-side failure: the single-stream pose kernel waited ~2 s for the key-line stream's
                                          signal and did not get it (a failed launch there); pose held, no by-products published */
};

/* Flags describing the path taken through the state machine. */
enum {
    STVO_PATH_STAGE1_GOOD = 1,  /* isGoodSolution after stage 1 (:341)       */
    STVO_PATH_ROBUST_FALLBACK = 2, /* gaussNewtonOptimizationRobust ran (:359) */
    STVO_PATH_REFINED = 4       /* stage 2 ran (:345-350)                    */
};

/* Output of optimizePose.  `T` is what the reference stores in curr_frame->DT, i.e.
 * expmap(logmap(inverse(DT_opt))) (:374); identity when rejected (:385).            */
typedef struct stvo_pose_result {
    double T[16];
    double cov[36];
    double cov_eig[6];
    double err;        /* curr_frame->err_norm; -1 when rejected (:387) */
    double T_opt[16];  /* raw optimiser variable DT before the commit step */
    double err_opt;    /* raw err of the last optimiser call */
    int32_t status;    /* STVO_POSE_* */
    int32_t path;      /* STVO_PATH_* flags */
    int32_t iters[2];  /* optimizeFunctions evaluations in stage 1 / stage 2 (or fallback) */
    int32_t n_matched_pt, n_matched_ls;
    int32_t n_inliers_pt, n_inliers_ls;
} stvo_pose_result;

/* Correspondence records handed to optimizePose: the live fields of matched_pt / matched_ls
 * (include/stereoFeatures.h:30-121).  Host pointers for the host-buffer
 * entry points.  `inlier_*` are in/out (1 = inlier). */
typedef struct stvo_matched {
    int32_t np;
    const double* P;       /* [np][3]  PointFeature::P                                   */
    const double* pl_obs;  /* [np][2]  PointFeature::pl_obs                              */
    const double* sigma2p; /* [np]     PointFeature::sigma2                              */
    int32_t* inlier_p;     /* [np]                                                       */
    int32_t nl;
    const double* sP;      /* [nl][3]  LineFeature::sP                                   */
    const double* eP;      /* [nl][3]  LineFeature::eP                                   */
    const double* le_obs;  /* [nl][3]  LineFeature::le_obs                               */
    const double* spl;     /* [nl][2]  LineFeature::spl (prev-frame end point, overlap)  */
    const double* epl;     /* [nl][2]  LineFeature::epl                                  */
    const double* sigma2l; /* [nl]     LineFeature::sigma2 AFTER safeCopy's re-scaling   */
    int32_t* inlier_l;     /* [nl]                                                       */
} stvo_matched;

/* Extracted features of ONE frame for B independent sequences: what detectStereoPoints / detectStereoLineSegments
 * leave behind before the stereo association (src/stereoFrame.cpp:88-100,191-203).  Host pointers; per-sequence
 * arrays are strided by stride_kp / stride_kl rows.  Key-points are cv::KeyPoint::pt (float x, y) + octave;
 * key-lines are line_descriptor::KeyLine start/end points (float) + octave; descriptors are 32-byte rows. */
typedef struct stvo_frame_features {
    int32_t stride_kp, stride_kl;
    const int32_t* n_kp_l;   /* [B] */
    const int32_t* n_kp_r;   /* [B] */
    const float* kp_l;       /* [B][stride_kp][2] */
    const int32_t* oct_l;    /* [B][stride_kp]    */
    const uint8_t* desc_l;   /* [B][stride_kp][32] */
    const float* kp_r;       /* [B][stride_kp][2] */
    const uint8_t* desc_r;   /* [B][stride_kp][32] */
    const int32_t* n_kl_l;   /* [B] (may be NULL: no lines) */
    const int32_t* n_kl_r;   /* [B] */
    const float* kl_l;       /* [B][stride_kl][4]  sx, sy, ex, ey */
    const int32_t* oct_ll;   /* [B][stride_kl]    */
    const uint8_t* ldesc_l;  /* [B][stride_kl][32] */
    const float* kl_r;       /* [B][stride_kl][4] */
    const uint8_t* ldesc_r;  /* [B][stride_kl][32] */
} stvo_frame_features;

/* Parameters of the ORB point front-end = the cv::ORB::create arguments the reference passes (src/stereoFrame.cpp:112-114)
 * that vary between its configurations.  The ranking, orb_score, is chosen with stvo_orb_set_score_type (default FAST_SCORE); WTA_K and
 * the patch size, orb_wta_k / orb_patch_size, with stvo_orb_set_descriptor (default 2 and 31; built: 2 / 3 / 4 and 2 .. 63, a patch size
 * other than 31 under the border rule edge_threshold >= ceil((patch_size / 2) sqrt 2); patch sizes above 63 are not built). */
#define STVO_ORB_MAX_LEVELS 8
#define STVO_ORB_SCORE_HARRIS 0 /* cv::ORB::HARRIS_SCORE */
#define STVO_ORB_SCORE_FAST 1   /* cv::ORB::FAST_SCORE   */
typedef struct stvo_orb_params {
    int32_t nfeatures;       /* Config::orbNFeatures()  (2000 in config_kitti.yaml)                     */
    int32_t fast_threshold;  /* Config::orbFastTh() or the handler's adaptive orb_fast_th (1 .. 254)     */
    int32_t edge_threshold;  /* Config::orbEdgeTh()  (19; must be >= 19: patch radius 15, pattern reach) */
    int32_t nlevels;         /* Config::orbNLevels()  (1 in config_kitti.yaml, 4 in config_euroc.yaml:61 and src/config.cpp:97);
                                0 is read as 1; at most STVO_ORB_MAX_LEVELS */
    double scale_factor;     /* Config::orbScaleFactor()  (1.2; > 1; ignored for one level) */
} stvo_orb_params;

/* The adaptive FAST threshold rule of StereoFrameHandler::updateFrame (src/stereoFrameHandler.cpp:66-86) = Config::fastMinTh /
 * fastMaxTh / fastIncTh / fastFeatTh / fastErrTh (config_kitti.yaml: 7, 30, 5, 50, 0.5; the other shipped files: 5, 50, 5, 50, 0.5).
 * err_th is a float as in the reference (:72): err_norm is compared with its value widened to double. */
typedef struct stvo_fast_adapt {
    int32_t min_th, max_th, inc_th, feat_th;
    float err_th;
} stvo_fast_adapt;

/* Trajectory and key-frame decision per stream (StereoFrameHandler's public state the odometry leaves behind: curr_frame->Tfw /
 * Tfw_cov of optimizePose's "set estimated pose" block, src/stereoFrameHandler.cpp:372-391, and the "slam functions" needNewKF /
 * currFrameIsKF, :1136-1218).  The thresholds are Config::minEntropyRatio / maxKFTDist / maxKFRDist (0.85, 5.0, 15.0 in every
 * shipped configuration).  keyframes = 0: the pose is composed and never reset. */
typedef struct stvo_traj_params {
    int32_t keyframes;
    int32_t reserved;
    double min_entropy_ratio, max_kf_t_dist, max_kf_r_dist;
} stvo_traj_params;

/* One stream's state: the pose of the last frame in the map frame, and the five members the key-frame decision keeps
 * (include/stereoFrameHandler.h:81-85).  Initial (stvo_traj_init_dev; src/stereoFrameHandler.cpp:35-51): Tfw = I, Tfw_cov = I,
 * prev_f_iskf = 1, entropy_first_prevKF = 0, T_prevKF = I, cov_prevKF_currF = 0, counters 0. */
typedef struct stvo_traj_state {
    double Tfw[16];
    double Tfw_cov[36];
    double entropy_first_prevKF;
    double T_prevKF[16];
    double cov_prevKF_currF[36];
    int32_t prev_f_iskf;
    int32_t N_prevKF_currF;
    int32_t n_frames;    /* pose results taken in */
    int32_t n_keyframes; /* resets among them */
} stvo_traj_state;

/* What one update leaves for the caller (448 bytes): the frame's pose BEFORE a key-frame reset, the three quantities the decision
 * compared (0 with keyframes off), the decision, and the number of the frame in its stream (the first tracked frame is 1). */
typedef struct stvo_traj_record {
    double Tfw[16];
    double Tfw_cov[36];
    double entropy_ratio, t, r;
    int32_t new_kf;
    int32_t frame;
} stvo_traj_record;

/* One feature of a stream's current stereo set as the handler's lists know it (stvo_seq_set_tracks), 8 bytes:
 *   idx     PointFeature::idx / LineFeature::idx: handed from the previous frame's feature by the f2f match
 *           (src/stereoFrameHandler.cpp:151,178), the feature's own position when nothing matched it (src/stereoFrame.cpp:151,165,350,384),
 *           and the position again behind a key-frame (currFrameIsKF, :1190-1218);
 *   age     f2f matches in a row that led to this feature since it was last numbered by position (saturates at 65535);
 *   kf      1: idx names a feature of the stream's last key-frame (an observation of it), 0: a feature first seen after it;
 *   inlier  the pose kernel's flag of the match that led here (1 / 0), -1 for a feature nothing matched. */
typedef struct stvo_track {
    int32_t idx;
    uint16_t age;
    uint8_t kf;
    int8_t inlier;
} stvo_track;

/* What goes with a stream's key-frame set: the rows of the set that are valid, the pipeline step (0 = the first) whose stereo set
 * it is, and the number of the key-frame in its sequence (the first frame is 1).  serial == 0: no key-frame set yet. */
typedef struct stvo_kf_header {
    int32_t n_pts, n_lines, frame, serial;
} stvo_kf_header;

/* A key-line as the LBD descriptor consumes it: the line_descriptor::KeyLine fields BinaryDescriptor::computeImpl copies into its
 * OctaveSingleLine (3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:592-609), octave 0.
 * Domain of the descriptor: every sample coordinate of the support region (63 rows across, (short) num_pixels along) inside
 * +-32767 before it is clamped into the image, and angle inside [-2 pi, 2 pi].  Beyond that the source's (short) cast of the rounded
 * coordinate is undefined and no result is promised.  Of the end points only the mid-point is used; num_pixels is taken through a
 * (short) cast as the source takes it (32768 walks nothing, 65537 walks one step), and a walk of no step gives a NaN descriptor. */
typedef struct stvo_keyline {
    float sx, sy, ex, ey;  /* sPointInOctaveX / Y, ePointInOctaveX / Y */
    float angle;           /* KeyLine::angle = atan2(ey - sy, ex - sx), radians */
    int32_t num_pixels;    /* KeyLine::numOfPixels (cv::LineIterator count): the length of the line support region */
} stvo_keyline;

/* Stereo calibration as the reference's YAML constructor reads it (src/pinholeStereoCamera.cpp:30-125), before rectification.
 * form STVO_RECT_FORM_KITTI: cam_fx / cam_fy / cam_cx / cam_cy and cam_d0..d3 (fx, fy, cx, cy, d).  STVO_RECT_FORM_RADTAN and
 * STVO_RECT_FORM_FISHEYE: Kl / Kr = (fx, fy, cx, cy), Dl / Dr (n_dist = 4, 5 or 8 rad-tan coefficients; 4 equidistant ones for
 * the fisheye form, which the reference selects with a `dtype` key), R row-major, t.  b = cam_bl in every form (never derived
 * from t).  Rl / Rr of the YAML are not read (the reference ignores them). */
enum { STVO_RECT_FORM_KITTI = 0, STVO_RECT_FORM_RADTAN = 1, STVO_RECT_FORM_FISHEYE = 2 };
typedef struct stvo_rect_calib {
    int32_t form;
    int32_t width, height;
    int32_t n_dist;
    double b;
    double fx, fy, cx, cy, d[4];
    double Kl[4], Kr[4];
    double Dl[8], Dr[8];
    double R[9], t[3];
} stvo_rect_calib;

/* The rectified stereo camera: R1 / R2 (3 x 3) and P1 / P2 (3 x 4) row-major as stereoRectify returns them (form KITTI: R = I and
 * P = [fx 0 cx 0; 0 fx cy 0; 0 0 1 0] in float, src/pinholeStereoCamera.cpp:114), cam = the camera the pipeline works with
 * (fx = P1(0,0), fy = P1(1,1), cx = P1(0,2), cy = P1(1,2), b = cam_bl; form KITTI: the intrinsics as read), dist = whether
 * rectifyImagesLR remaps (0: it copies, :198-207). */
typedef struct stvo_rect_camera {
    int32_t dist, width, height, reserved;
    double R1[9], R2[9], P1[12], P2[12];
    stvo_cam cam;
} stvo_rect_camera;

/* Error codes of the C-ABI (0 ok, <0 error; never throws). */
enum {
    STVO_OK = 0,
    STVO_ERR_INVALID_ARG = -1,   /* contract violations the reference throws on (matching.cpp:50,113,184) */
    STVO_ERR_HIP = -2,           /* a HIP runtime call failed */
    STVO_ERR_NO_DEVICE = -3,     /* no gfx950 device visible: the product never falls back to CPU */
    STVO_ERR_CAPACITY = -4,      /* problem larger than the context was created for */
    STVO_ERR_UNSUPPORTED = -5
};

#ifdef __cplusplus
}
#endif
#endif /* STVO_TYPES_H */
