/*
 * stvo_hip.h — C-ABI of the MI355X-native PL-StVO hot path (libstvo_hip.so, gfx950 only).
 *
 * The reference (/root/reference) has NO plugin / FFI interface: its boundary is the C++ class API
 * consumed by app/imagesStVO.cpp:86-124.  This header declares the `extern "C"` seams a maintainer
 * binds in place of the reference's inner functions (see INTEGRATION.md for the stubs); every
 * entry point cites the reference interface it replaces.  Plain pointers and sizes only.
 *
 *   - returns 0 (STVO_OK) or a negative STVO_ERR_* code; never throws, never aborts
 *   - there is NO CPU fallback: without a gfx950 device stvo_ctx_create fails with
 *     STVO_ERR_NO_DEVICE and nothing else can be called
 *   - host-buffer entry points copy in/out through pinned staging and synchronise before returning
 *   - *_dev entry points take DEVICE pointers, enqueue on the context's stream and do not
 *     synchronise (use stvo_ctx_synchronize / your own events)
 *   - descriptors: N x 32 bytes, contiguous; matrices row-major FP64; twists (t, w)
 */
#ifndef STVO_HIP_H
#define STVO_HIP_H

#include "stvo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STVO_ABI_VERSION 3
#define STVO_MAX_ROWS_LIMIT 65535 /* packed (distance << 16 | index) keys */
#define STVO_POSE_MAX_POINTS 2048 /* per frame pair: points owned per worker thread x worker threads of the pose kernel */
#define STVO_POSE_MAX_LINES 512

typedef struct stvo_ctx stvo_ctx;

/* ---- library / context ------------------------------------------------------------------- */
const char* stvo_backend_name(void); /* "hip-gfx950" */
int stvo_abi_version(void);
const char* stvo_error_string(int code);
/* Last HIP error text recorded on this context ("" if none). */
const char* stvo_ctx_last_error(const stvo_ctx* ctx);

/* One context per sequence / host thread (the reference's StereoFrameHandler is not re-entrant
 * either).  Owns device scratch sized for `max_rows` descriptors per set and
 * `max_batch` problems per launch, pinned staging buffers and (unless set_stream is used) a stream. */
int stvo_ctx_create(int device_id, int max_rows, int max_batch, stvo_ctx** out);
int stvo_ctx_destroy(stvo_ctx* ctx);
/* Borrow an existing hipStream_t (e.g. the caller's / torch's current stream); NULL = default. */
int stvo_ctx_set_stream(stvo_ctx* ctx, void* hip_stream);
int stvo_ctx_synchronize(stvo_ctx* ctx);
/* Throughput option for the batched path.  enable = 1: stvo_track_batched_dev enqueues the pose kernel
 * on a second (context-owned) stream behind an event, so that the NEXT call's matching kernels run
 * concurrently with this call's latency-bound pose kernel (worth ~7 % with the VALU matcher, which is then
 * launched with an occupancy cap, ~1-2 % with the matrix-core matcher).  Results of a call are complete after stvo_ctx_synchronize (or a
 * device synchronise); hazards between consecutive calls on the same buffers are handled with events.
 * enable = 0 (default): strict stream order on the context's stream. */
int stvo_ctx_set_overlap(stvo_ctx* ctx, int enable);

/* ---- matching: host-buffer seams ------------------------------------------------------------ */

/* Replaces  int StVO::match(const cv::Mat&, const cv::Mat&, float nnr, std::vector<int>&)
 * (include/matching.h:52, src/matching.cpp:63-91; with mutual == 0: matchNNR, :41-61).
 * m12[i] = matched row of d2 or -1;  *n_matches = return value of the reference function.
 * n2 < 2 yields no matches (the reference reads out of bounds there, src/matching.cpp:54). */
int stvo_match_nnr_mutual(stvo_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, float nnr, int mutual,
                          int32_t* m12, int32_t* n_matches);

/* Replaces  int StVO::matchGrid(const std::vector<point_2d>&, const cv::Mat&, const GridStructure&,
 *                               const cv::Mat&, const GridWindow&, std::vector<int>&)
 * (include/matching.h:57, src/matching.cpp:111-177).  The GridStructure (64x48 std::list buckets,
 * src/gridStructure.cpp:43-83) is passed as CSR: cell c = y*64 + x owns
 * cell_items[cell_start[c] .. cell_start[c+1]).  `ratio` = Config::minRatio12P() (double test, :160),
 * `mutual` = Config::bestLRMatches(). */
int stvo_match_grid_points(stvo_ctx* ctx, const int32_t* cell_xy1 /*[n1][2]*/, const uint8_t* d1, int n1,
                           const int32_t* cell_start /*[3073]*/, const int32_t* cell_items, const uint8_t* d2, int n2,
                           const stvo_grid_window* w, double ratio, int mutual, int32_t* m12, int32_t* n_matches);

/* Replaces the line overload of StVO::matchGrid (include/matching.h:60, src/matching.cpp:179-258).
 * cell_xy1 = [n1][4] (sx, sy, ex, ey) integer cells of the left end points; dir2 = [n2][2] unit
 * directions of the right lines in grid space (src/stereoFrame.cpp:331-333). */
int stvo_match_grid_lines(stvo_ctx* ctx, const int32_t* cell_xy1 /*[n1][4]*/, const uint8_t* d1, int n1,
                          const int32_t* cell_start /*[3073]*/, const int32_t* cell_items, const uint8_t* d2, int n2,
                          const double* dir2 /*[n2][2]*/, const stvo_grid_window* w, double ratio, double line_sim_th,
                          int mutual, int32_t* m12, int32_t* n_matches);

/* ---- optimizer: host-buffer seams ----------------------------------------------------------- */

/* Replaces the private  void StereoFrameHandler::optimizeFunctions(Matrix4d, Matrix6d&, Vector6d&, double&)
 * and optimizeFunctionsRobust (include/stereoFrameHandler.h:97-98, src/stereoFrameHandler.cpp:549-962):
 * one evaluation of H (6x6), g (6), e at pose T over the inlier records. *n_used = N_p + N_l. */
int stvo_normal_eq(stvo_ctx* ctx, const double T[16], const stvo_cam* cam, const stvo_opt_params* params,
                   const stvo_matched* m, int robust, double H[36], double g[6], double* e, int32_t* n_used);

/* Replaces  void StereoFrameHandler::optimizePose()  (include/stereoFrameHandler.h:54,
 * src/stereoFrameHandler.cpp:307-392) minus the Tfw composition (:377-378, done by the caller):
 * GN / robust GN / LM, removeOutliers (:988-1067), isGoodSolution (:292-305) and the commit rule.
 * init_T = the DT chosen at :317-326.  m->inlier_* are updated in place. */
int stvo_optimize_pose(stvo_ctx* ctx, const double init_T[16], const stvo_cam* cam, const stvo_opt_params* params,
                       stvo_matched* m, stvo_pose_result* out);

/* ---- batched, device-resident path (throughput mode; B independent frame pairs) --------------- */

/* All pointers are DEVICE pointers.  Per-frame arrays are strided by max_pts / max_lines rows.
 * Replaces, per frame pair, f2fTracking() + optimizePose() (src/stereoFrameHandler.cpp:106-180,
 * 307-392): brute-force mutual NNR matching of prev->pdesc_l vs curr->pdesc_l (and ldesc_l),
 * gathering of the matched records, and the full pose optimisation. */
typedef struct stvo_track_batch_dev {
    int32_t B, max_pts, max_lines, reserved;
    /* prev frame: stereo points / lines that survived stereo association */
    const int32_t* n_prev_pts;   /* [B] */
    const uint8_t* prev_pdesc;   /* [B][max_pts][32] */
    const double* prev_P;        /* [B][max_pts][3] */
    const double* prev_sigma2p;  /* [B][max_pts] */
    const int32_t* n_curr_pts;   /* [B] */
    const uint8_t* curr_pdesc;   /* [B][max_pts][32] */
    const double* curr_pl;       /* [B][max_pts][2]  -> pl_obs of the matched prev point */
    const int32_t* n_prev_lines; /* [B]  (may be NULL when max_lines == 0) */
    const uint8_t* prev_ldesc;   /* [B][max_lines][32] */
    const double* prev_sP;       /* [B][max_lines][3] */
    const double* prev_eP;       /* [B][max_lines][3] */
    const double* prev_spl;      /* [B][max_lines][2] */
    const double* prev_epl;      /* [B][max_lines][2] */
    const double* prev_sigma2l;  /* [B][max_lines]  (after safeCopy's re-scaling) */
    const int32_t* n_curr_lines; /* [B] */
    const uint8_t* curr_ldesc;   /* [B][max_lines][32] */
    const double* curr_le;       /* [B][max_lines][3] -> le_obs of the matched prev line */
    const double* init_T;        /* [B][16] or NULL = identity */
    /* outputs */
    int32_t* m12_pts;            /* [B][max_pts]   */
    int32_t* m12_lines;          /* [B][max_lines] */
    int32_t* inlier_pts;         /* [B][max_pts]   -1 unmatched, 0 outlier, 1 inlier */
    int32_t* inlier_lines;       /* [B][max_lines] */
    stvo_pose_result* results;   /* [B] */
} stvo_track_batch_dev;

int stvo_track_batched_dev(stvo_ctx* ctx, const stvo_track_batch_dev* batch, const stvo_cam* cam,
                           const stvo_opt_params* params, float nnr_points, float nnr_lines, int mutual);

/* The matching stage alone (forward scan + mutual check) on device-resident descriptor sets: m12[b][i]. */
int stvo_match_nnr_mutual_batched_dev(stvo_ctx* ctx, int B, int row_stride, const uint8_t* d1, const int32_t* n1,
                                      const uint8_t* d2, const int32_t* n2, float nnr, int mutual, int32_t* m12);

/* The optimizer stage alone on device-resident, already associated records (m12 = identity). */
int stvo_optimize_pose_batched_dev(stvo_ctx* ctx, const stvo_track_batch_dev* batch, const stvo_cam* cam,
                                   const stvo_opt_params* params);

/* ---- device-resident per-frame pipeline ------------------------------------ */

/* B independent stereo sequences advancing in lock-step; all per-frame state (stereo point / line sets of the
 * previous frame, grids, matches) lives in HBM.  Replaces, per pushed frame and per sequence,
 * StereoFrameHandler::initialize / insertStereoPair + optimizePose + updateFrame minus feature detection
 * (src/stereoFrameHandler.cpp:35-60, 307-392, 89-100): stereo association on the 64x48 grid
 * (src/stereoFrame.cpp:120-173, 309-415), f2f tracking, pose optimisation.  The Tfw composition (:377-378) stays
 * with the caller; the adaptive FAST threshold (:66-86, a front-end knob) is stvo_seq_adapt_fast_dev below.  init_T is the identity
 * (use_motion_model = false, as in every shipped configuration) unless stvo_seq_set_motion_model turns the motion model on. */
typedef struct stvo_seq stvo_seq;
int stvo_seq_create(stvo_ctx* ctx, int B, int max_keypoints, int max_keylines, int img_cols, int img_rows,
                    const stvo_cam* cam, const stvo_match_params* mp, const stvo_opt_params* op, stvo_seq** out);
/* As stvo_seq_create with one calibration and image size PER SEQUENCE: cams[B], img_cols[B], img_rows[B] (host arrays).
 * BASELINE configs[4] runs KITTI sequences 00-07 side by side and the reference builds one PinholeStereoCamera per
 * dataset (app/imagesStVO.cpp:66): config/dataset_params/kitti00-02.yaml, kitti03.yaml and kitti04-10.yaml differ in
 * focal length, principal point, baseline and image size (1241x376, 1242x375, 1226x370), i.e. in the grid scale
 * 64 / cols, 48 / rows of src/stereoFrame.cpp:47-48 as well. */
int stvo_seq_create_multi(stvo_ctx* ctx, int B, int max_keypoints, int max_keylines, const int32_t* img_cols,
                          const int32_t* img_rows, const stvo_cam* cams, const stvo_match_params* mp,
                          const stvo_opt_params* op, stvo_seq** out);
int stvo_seq_destroy(stvo_seq* seq);
/* Config::useMotionModel() for every sequence of the pipeline (src/stereoFrameHandler.cpp:317-324): the initial DT of a frame pair is
 * prev_frame->DT (the increment COMMITTED for the previous pair, i.e. after :374's inverse) unless !isGoodSolution(prev_frame->DT,
 * prev_frame->DT_cov, prev_frame->err_norm), then the identity.  The decision is taken on the device by the previous step's commit —
 * the result never leaves HBM.  Enabling (again) restarts every sequence from prev_frame->DT = I (:45); synchronises. */
int stvo_seq_set_motion_model(stvo_seq* seq, int enable);
/* Number of raw frame slots (2 .. STVO_SEQ_MAX_SLOTS; 2 after create).  A throughput caller uploads several consecutive
 * frames of every sequence once (stvo_seq_upload) and rotates stvo_seq_step_dev through the slots. */
#define STVO_SEQ_MAX_SLOTS 16
int stvo_seq_set_slots(stvo_seq* seq, int n_slots);
/* One upload, one synchronisation, one small download per frame.  results: [B] (zeroed for the first frame, which
 * only builds the stereo sets); counts: optional [B][4] = stereo points, stereo lines, matched points, matched
 * lines of this frame. */
int stvo_seq_push(stvo_seq* seq, const stvo_frame_features* frame, stvo_pose_result* results, int32_t* counts);
/* The three halves of stvo_seq_push, for callers that keep frames resident in HBM (throughput mode): upload one
 * frame's features into device slot 0 / 1 (asynchronous), run the pipeline on a resident slot (asynchronous, no
 * host transfer), fetch the results of the last step (synchronises). */
int stvo_seq_upload(stvo_seq* seq, int slot, const stvo_frame_features* frame);
/* stvo_seq_upload for features that already live in DEVICE memory — every pointer of `frame`, the count arrays included; oct_l /
 * oct_ll may be NULL (octave 0, e.g. the one-level ORB front-end below).  Asynchronous on the context's stream; counts are
 * clamped to the capacities on the device.  Together with stvo_orb_detect_dev: images in, poses out, nothing through the host
 * (replaces detectStereoPoints + matchStereoPoints + f2fTracking + optimizePose, src/stereoFrame.cpp:88-173,
 * src/stereoFrameHandler.cpp:106-392). */
int stvo_seq_upload_dev(stvo_seq* seq, int slot, const stvo_frame_features* frame);
int stvo_seq_step_dev(stvo_seq* seq, int slot);
int stvo_seq_read(stvo_seq* seq, stvo_pose_result* results, int32_t* counts);

/* By-products for callers that keep the reference's HOST-side feature lists (the StereoFrameHandler mirror):
 * with fetch enabled every step also copies to pinned memory (a) right after the f2f stage — while the pose
 * kernel still runs — the raw stereo matches of the new frame (left key-point / key-line i -> right index or -1,
 * what matchGrid returns at stereoFrame.cpp:145,344, [B][K] / [B][M] with K, M = the capacities rounded up to 64)
 * and the f2f matches (prev stereo feature k -> curr stereo feature or -1, what StVO::match returns at
 * stereoFrameHandler.cpp:141,164), and (b) after the pose kernel the inlier flags of the prev stereo features
 * (-1 unmatched, 0 outlier, 1 inlier; removeOutliers :988-1067).  fetch_matches waits for (a) only; the pointers
 * stay valid until the next step.  fetch_inliers synchronises the stream. */
int stvo_seq_enable_fetch(stvo_seq* seq, int enable);
int stvo_seq_fetch_matches(stvo_seq* seq, const int32_t** m12_stereo_pts, const int32_t** m12_stereo_lines,
                           const int32_t** m12_pts, const int32_t** m12_lines);
int stvo_seq_fetch_inliers(stvo_seq* seq, const int32_t** inl_pts, const int32_t** inl_lines);
/* Row strides of the arrays above. */
int stvo_seq_strides(const stvo_seq* seq, int32_t* stride_pts, int32_t* stride_lines);

/* Live per-stage timing of the pipeline (bench.py): with enable = 1 every stvo_seq_step_dev brackets, with hipEvents on
 * the stream the kernels run on, stage 0 = the whole stereo point stage (cells + grid matcher + tail), 1 = the two
 * grid_scan passes of the point grid matcher alone, 2 = the forward top-2 scan of the point f2f match (K1m), 3 = plan +
 * reverse scans of its mutual check, 4 = the pose kernel.  get synchronises, returns the average milliseconds per stage over
 * the steps measured since the last get / set (n_steps = the largest number of samples any stage has) and resets.
 * enable = 2 ("light"): pairs around stages 1, 2 and 4 only — the three big kernels of the point stream — and the step is otherwise
 * enqueued exactly as an untimed one (key-line stream unmarked, the next frame's grid built ahead on it), so the kernels keep the
 * neighbours they have in the timed region; stages 0 and 3 report 0. */
#define STVO_SEQ_NSTAGE 5
int stvo_seq_set_stage_timing(stvo_seq* seq, int enable);
int stvo_seq_get_stage_timing(stvo_seq* seq, float avg_ms[STVO_SEQ_NSTAGE], int32_t* n_steps);

/* TEST HOOK: the schedule the LAST ENQUEUED step (stvo_seq_step_dev / stvo_seq_push) chose on the host, so that a test of one route
 * can assert that the step took it.  Pure bookkeeping: nothing is launched, awaited or decided by this call.  out[STVO_SCHED_*]:
 * POSE_KERNEL = 0 no pose kernel (first frame), STVO_SCHED_POSE_LATENCY (pose_kernel.hip) or STVO_SCHED_POSE_BATCH (pose_kernel2p.hip);
 * POSE_WAVES = waves per frame pair of the batch kernel (2 or 4; 0 otherwise); the others are 0 / 1: FUSED_CELLS = the grid of a frame
 * is the point matcher's first phase; CELLS_AHEAD = it was built on the key-line stream ahead of the step; LINES_AHEAD = the key-line
 * stage waited for the PREVIOUS step's fork event; GATE = the stream gate was launched in front of it; MID_FORK = the key-line stream
 * forks behind the cells kernel; LINE_FUSED = the key-line association ran as one workgroup per frame.  All 0 before the first step. */
#define STVO_SCHED_POSE_KERNEL 0
#define STVO_SCHED_POSE_WAVES 1
#define STVO_SCHED_FUSED_CELLS 2
#define STVO_SCHED_CELLS_AHEAD 3
#define STVO_SCHED_LINES_AHEAD 4
#define STVO_SCHED_GATE 5
#define STVO_SCHED_MID_FORK 6
#define STVO_SCHED_LINE_FUSED 7
#define STVO_SCHED_POSE_LATENCY 1
#define STVO_SCHED_POSE_BATCH 2
int stvo_seq_last_schedule(const stvo_seq* seq, int32_t out[8]);

/* TEST HOOK: the grid structures the last step built ON THE DEVICE for sequence b (lines = 0: key-points, 1: key-lines):
 * cell_start[3073] / cell_items (cell c = y * 64 + x owns cell_items[cell_start[c] .. cell_start[c+1]); the order inside a
 * cell is unspecified) = GridStructure after src/stereoFrame.cpp:135-139 / :325-338 (lines: every LineIterator cell);
 * cells_left [n_left][2 | 4] = the integer cells of the left features (:129-132, :318-322); cand_off[n_left + 1] / cand =
 * the candidate set GridStructure::get (src/gridStructure.cpp:65-76) yields for every left feature with the stereo window
 * (:141-143, :340-342; lines: the union over both end points, src/matching.cpp:213-215), ascending right ids. */
int stvo_seq_debug_grid(stvo_seq* seq, int b, int lines, int32_t* cell_start, int32_t* cell_items, int32_t cap_items,
                        int32_t* cells_left, int32_t* cand_off, int32_t* cand, int32_t cap_cand, int32_t* n_left);

/* TEST HOOK: the route the stereo point matcher of the last step took for every sequence: out [B][2] = {misfit, ovf}.  misfit = 1: the
 * one-workgroup-per-frame kernel handed the frame to the scan formulation (more keys or wide right key-points than its LDS holds);
 * ovf = 1: the scan formulation met a right key-point with more eligible pairs than its list holds and ran its second scan.  A word
 * that the step's route does not write for a frame is reported as 0 (misfit on the scan route; ovf for a frame the one-workgroup
 * kernel matched itself, and with best_lr_matches off), never as an earlier step left it.  Synchronises, copies, launches nothing
 * and changes no state; call it before stvo_seq_debug_grid, whose own kernels clear ovf.  Before the first step:
 * STVO_ERR_INVALID_ARG. */
int stvo_seq_debug_point_route(stvo_seq* seq, int32_t* out);

/* TEST HOOK: the stereo sets the last step built from its frame for sequence b, i.e. what the tails of the stereo association
 * (src/stereoFrame.cpp:152-172, :351-395) wrote: n_pts stereo points as rc [n_pts][4] = {u, v, disparity, level} (floats) with the kept
 * left descriptor rows desc [n_pts][32]; n_lines stereo lines as spl, epl [n_lines][2], sP, eP, le [n_lines][3], s2l (sigma2 of the
 * LineFeature constructor), s2lm (after LineFeature::safeCopy's re-scaling) [n_lines] and ldesc [n_lines][32].  Synchronises the
 * context's stream and the key-line stream, copies, launches nothing and changes no state.  cap_pts / cap_lines: rows the caller's
 * arrays hold; too few: STVO_ERR_CAPACITY with the counts filled in.  A step of any schedule writes the set it then makes the
 * previous one, so the last step's set is always known; before the first step there is none: STVO_ERR_INVALID_ARG. */
int stvo_seq_debug_stereo(stvo_seq* seq, int b, int32_t cap_pts, int32_t* n_pts, float* rc, uint8_t* desc, int32_t cap_lines,
                          int32_t* n_lines, double* spl, double* epl, double* sP, double* eP, double* le, double* s2l, double* s2lm,
                          uint8_t* ldesc);

/* ---- ORB point front-end ------------------------------------------------------------------ */

/* Replaces  cv::ORB::create(nfeatures, scaleFactor, nlevels, ...)->detectAndCompute(img, Mat(), points, pdesc, false)  as
 * called by StereoFrame::detectPointFeatures (src/stereoFrame.cpp:104-118) for B images of cols x rows bytes at once: the image
 * pyramid (8-bit bilinear resize level by level), per level FAST-9/16 with non-maximum suppression, border filter,
 * retainBest(the level's share of nfeatures) on the FAST response (ties at the cut are kept), intensity-centroid orientation,
 * 7x7 Gaussian blur and the 256-bit rotated BRIEF descriptor; key-points of all levels in level order with their octave and
 * coordinates scaled back to the full image.  Within a level key-points are emitted in row-major order (OpenCV leaves the
 * order to std::nth_element).  When more key-points qualify than max_keypoints holds, the first max_keypoints of that order
 * come back (deterministically) and the uncapped count is reported in n_total.  max_keypoints may not exceed 4096
 * (STVO_ERR_CAPACITY).  OpenCV is third-party code that is not part of the reference tree: the semantics are pinned to
 * oracle/stvo_orb_oracle.c only (parity unpinned). */
typedef struct stvo_orb stvo_orb;
int stvo_orb_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keypoints, const stvo_orb_params* prm, stvo_orb** out);
int stvo_orb_destroy(stvo_orb* orb);
/* The 256 x 4 test pattern (x0, y0, x1, y1 per bit, |coordinate| <= 13).  The default is a seeded table; OpenCV's learned
 * table (bit_pattern_31_ of features2d/src/orb.cpp) is data this repository does not hold — pass it here to reproduce it.
 * It is the pool of patch size 31: under another setting of stvo_orb_set_descriptor the effective pattern is derived from it again
 * (wta_k 3 / 4 refuse a pool with fewer different points than a tuple holds), and at another patch size it is kept but not read. */
int stvo_orb_set_pattern(stvo_orb* orb, const int8_t* pattern /*[1024]*/);
/* The FAST threshold of the following calls: StereoFrameHandler::updateFrame adapts orb_fast_th frame by frame
 * (src/stereoFrameHandler.cpp:66-86) and passes it to detectStereoFeatures (:56 -> src/stereoFrame.cpp:59,104-118). */
int stvo_orb_set_fast_threshold(stvo_orb* orb, int fast_threshold /* 1 .. 254 */);
/* One FAST threshold PER IMAGE for the following calls, at every pyramid level and under either ranking: image i of the B images takes
 * th_dev[i % n_th].  n_th must divide B (else STVO_ERR_INVALID_ARG); n_th = B / 2 is how a stereo detector (B / 2 left images, then
 * B / 2 right ones) shares one threshold between the two images of a pair.  th_dev is a DEVICE array that stays the caller's: the
 * detection kernels read it when they run, in stream order, so a kernel enqueued earlier on the context's stream (stvo_fast_adapt_dev,
 * stvo_seq_adapt_fast_dev) may write it — no host round trip.  What is read is clamped to 1 .. 254 on the device.  th_dev == NULL
 * returns to the scalar of stvo_orb_set_fast_threshold, which keeps its meaning while an array is set but is not read. */
int stvo_orb_set_fast_thresholds_dev(stvo_orb* orb, const int32_t* th_dev, int n_th);
/* The same from a HOST array (every entry 1 .. 254): the detector keeps a device copy of its own, uploaded on the context's stream;
 * synchronises.  th_host == NULL returns to the scalar. */
int stvo_orb_set_fast_thresholds(stvo_orb* orb, const int32_t* th_host, int n_th);
/* One image SIZE per image for the following calls: image i of the B images is sizes_host[i % n] = {cols, rows}; n must divide B, and
 * with n = B / 2 the left image b and the right image B / 2 + b of a stereo detector share an entry.  The image buffer keeps the layout
 * [B][rows][cols] of the size given at creation (the slot): image i occupies the top-left cols_i x rows_i of its slot and keeps the slot's
 * row pitch; the bytes of the slot outside the image influence nothing.  What comes back for image i is, bit for bit, what a detector
 * created at (cols_i, rows_i) returns for that crop — key-points, responses, angles, octaves, descriptors, n_kp, n_total — at every
 * nlevels, under either ranking, every descriptor setting and together with per-image FAST thresholds: level sizes, resize ratios and the
 * rule by which a level yields anything are formed per entry (a level smaller than the border yields nothing for the images of that entry
 * while the other images' level runs).  All four detect entry points; the host-buffer ones take and return slot-shaped buffers as before.
 * STVO_ERR_INVALID_ARG and nothing changes: n <= 0, n > B, B % n != 0, an entry larger than the slot, an entry stvo_orb_create would
 * refuse as an image size (below 64, or 2 * edge_threshold >= a side).  sizes_host is read during the call; the table travels on the
 * context's stream behind the detections already enqueued, through pinned staging that is not reused before its copy has completed: no
 * synchronisation.  The device table is allocated at the first call; sizes_host == NULL: every image fills its slot again, on the very
 * kernels of a detector that was never given a table. */
int stvo_orb_set_image_sizes(stvo_orb* orb, const int32_t* sizes_host /* [n][2] = cols, rows */, int n);
/* The ranking of the following calls, cv::ORB::create's scoreType = Config::orbScore() (src/stereoFrame.cpp:112-114), with OpenCV's
 * values: STVO_ORB_SCORE_FAST (1, the default) as described above; STVO_ORB_SCORE_HARRIS (0): per level retainBest(2 x the level's
 * share) on the FAST response, HarrisResponses (7 x 7 block, k 0.04) of the survivors on the level image, retainBest(the level's
 * share) on that response — ties kept at both cuts, row-major order as above — and `response` is the Harris response.  n_total then
 * counts the key-points that pass the second cut.  Any other value: STVO_ERR_INVALID_ARG.  Applies to all four detect entry points. */
int stvo_orb_set_score_type(stvo_orb* orb, int score_type);
/* The descriptor of the following calls, cv::ORB::create's WTA_K = Config::orbWtaK() and patchSize = Config::orbPatchSize()
 * (src/stereoFrame.cpp:112-114); the default is (2, 31).  Applies to all four detect entry points and to both rankings; FAST, the
 * suppression, the rankings, the level budgets, the blur, the pyramid and the order of the key-points do not depend on either value, and
 * key-points are filtered by edge_threshold alone, as in OpenCV.
 *   patch_size P, 2 .. 63: the intensity-centroid angle is taken on the disc of half patch P / 2 (umax as for 15).  The pool of 512 test
 *     points is the pattern of stvo_orb_set_pattern at P = 31 and OpenCV's makeRandomPattern (RNG(0x34985739), coordinates uniform in
 *     -P / 2 .. P / 2) at every other P, where the learned table plays no part.
 *   wta_k 2: 256 tests on the pool's points in pairs, as before.  wta_k 3 / 4: initializeOrbPattern — 128 tuples of 3 / 4 pairwise
 *     different points drawn from the pool with RNG(0x12345678); the descriptor holds, four tuples per byte, the index of the tuple's
 *     largest blurred intensity (ties go to the earlier point exactly as OpenCV's strict comparisons send them).  Still 32 bytes.
 * Every pixel read lies inside the level image, so for P != 31 the setting needs edge_threshold >= ceil((P / 2) sqrt 2): P <= 27 at the
 * shipped orb_edge_th 19, 44 for P = 63 (P = 31 keeps the reach 19 stvo_orb_create requires).  STVO_ERR_INVALID_ARG: wta_k outside
 * 2 .. 4, patch_size < 2, the border rule; STVO_ERR_UNSUPPORTED: patch_size > 63.  A refused call changes nothing.  Synchronises the
 * context's stream.  Parity with OpenCV itself is unpinned: the algorithm is restated, csrc/orb_pattern.h. */
int stvo_orb_set_descriptor(stvo_orb* orb, int wta_k, int patch_size);
/* HOST ONLY, no context: the effective point list of a setting — out[1024] = n_points (x, y) pairs (512 / 384 / 512 for wta_k 2 / 3 / 4),
 * zero beyond them — and the verdicts of stvo_orb_set_descriptor except the border rule, which needs a detector.  pool: the 1024-byte
 * pattern stvo_orb_set_pattern would be given (NULL: the seeded stand-in); it is read at patch_size 31 only, where a pool outside
 * -13 .. 13, or with fewer different points than a tuple holds, is STVO_ERR_INVALID_ARG.  n_points may be NULL. */
int stvo_orb_pattern(int wta_k, int patch_size, const int8_t* pool /*[1024] or NULL*/, int8_t* out /*[1024]*/, int32_t* n_points);
/* The effective point list of the setting in force (stvo_orb_pattern's `out`): the pattern itself under (2, 31). */
int stvo_orb_get_pattern(const stvo_orb* orb, int8_t* pattern /*[1024]*/);
/* Host buffers in / out, synchronises.  images [B][rows][cols]; kp_xy [B][max_keypoints][2] = cv::KeyPoint::pt; response =
 * cv::KeyPoint::response (FAST score, or the Harris response under STVO_ORB_SCORE_HARRIS); angle in degrees = cv::KeyPoint::angle; desc [B][max_keypoints][32]; n_kp [B]. */
int stvo_orb_detect(stvo_orb* orb, const uint8_t* images, float* kp_xy, float* response, float* angle, uint8_t* desc,
                    int32_t* n_kp);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_orb_detect_dev(stvo_orb* orb, const uint8_t* images, float* kp_xy, float* response, float* angle, uint8_t* desc,
                        int32_t* n_kp);
/* The full forms: octave [B][max_keypoints] = cv::KeyPoint::octave (the pyramid level, what PointFeature's sigma2 is made of,
 * src/stereoFeatures.cpp:41-47) and n_total [B] = the number of key-points that qualified before the max_keypoints cap
 * (n_total > n_kp: the output was truncated).  Either may be NULL. */
int stvo_orb_detect_levels(stvo_orb* orb, const uint8_t* images, float* kp_xy, float* response, float* angle, int32_t* octave,
                           uint8_t* desc, int32_t* n_kp, int32_t* n_total);
int stvo_orb_detect_levels_dev(stvo_orb* orb, const uint8_t* images, float* kp_xy, float* response, float* angle, int32_t* octave,
                               uint8_t* desc, int32_t* n_kp, int32_t* n_total);

/* Replaces the adaptive FAST threshold of  StereoFrameHandler::updateFrame  (src/stereoFrameHandler.cpp:66-86, adaptative_fast: true in
 * five of the six shipped configurations) for B streams at once, on the device: th_dev[b] (in / out) moves by what results_dev[b] says.
 *   lost = T == Matrix4d::Identity() (every element compares equal) || err > (double)err_th       -> 2 steps of inc_th down
 *   else the first row that applies of  n_inliers_pt < feat_th: 2 down; < 2 feat_th: 1 down; > 3 feat_th: 1 up; > 4 feat_th: 2 up
 *   (the last row can never apply, upstream as here); a move down stops at min_th, a move up at max_th, and only on that side.
 * A rejected pose carries T = I and err = -1.  results_dev: device memory or pinned host memory.  Enqueued on the context's stream. */
int stvo_fast_adapt_dev(stvo_ctx* ctx, int B, const stvo_pose_result* results_dev, const stvo_fast_adapt* prm, int32_t* th_dev /* [B] */);
/* The same behind the LAST ENQUEUED step of the pipeline (stvo_seq_step_dev / stvo_seq_push), reading that step's results where the
 * step wrote them, on the stream its pose kernel ran on; th_dev [B] device.  With stvo_orb_set_fast_thresholds_dev(orb, th_dev, B) on a
 * detector of 2 B images of the same context, the next frame's detection takes the adapted thresholds without the host seeing them.
 * The first frame of a sequence has no pose (initialize() calls no updateFrame(), app/imagesStVO.cpp:90-124): nothing is launched for
 * it and th_dev stays.  STVO_ERR_INVALID_ARG before the first step. */
int stvo_seq_adapt_fast_dev(stvo_seq* seq, const stvo_fast_adapt* prm, int32_t* th_dev);

/* ---- trajectory and key-frame decision per stream ------------------------------------------------------------------------ */

/* Replaces, for B streams at once and on the device, what StereoFrameHandler does with a pose result after optimizePose: the "set
 * estimated pose" block (src/stereoFrameHandler.cpp:372-391)
 *   status == STVO_POSE_OK:  Tfw <- expmap_se3(logmap_se3(Tfw * T)),  Tfw_cov <- unccomp_se3(Tfw_old, Tfw_cov_old, cov)
 *   otherwise:               both carried over; the frame counts as DT = I, DT_cov = 0
 * and, with prm->keyframes, needNewKF (:1136-1188) followed by currFrameIsKF (:1190-1218) when it says so: Tfw = I, Tfw_cov = I,
 * T_prevKF = I, cov_prevKF_currF = 0, prev_f_iskf = 1, N_prevKF_currF = 0, n_keyframes + 1.  The record (records_dev [B], may be NULL)
 * holds the pose BEFORE that reset, entropy_ratio / t / r as compared (0 with keyframes off), new_kf and the frame number.
 * state_dev [B] is in / out; stvo_traj_init_dev fills the state `initialize` leaves.  results_dev: device memory or pinned host
 * memory; T, cov and status are read.  Both are enqueued on the context's stream. */
int stvo_traj_init_dev(stvo_ctx* ctx, int B, stvo_traj_state* state_dev /* [B] */);
int stvo_traj_update_dev(stvo_ctx* ctx, int B, const stvo_pose_result* results_dev, const stvo_traj_params* prm,
                         stvo_traj_state* state_dev /* [B] */, stvo_traj_record* records_dev /* [B] or NULL */);
/* The same inside the pipeline.  prm != NULL: the sequence object owns the state [B] and a ring of log_steps (>= 1) x B records, and
 * every step that tracks (every step but a sequence's first) enqueues the update right behind its pose kernel, on the same stream,
 * writing ring row (tracked step) % log_steps.  prm == NULL: off (the default): nothing is allocated, nothing launched.  Only before
 * the first step; a ring above 1 GiB (448 bytes per record) is refused.  STVO_ERR_INVALID_ARG otherwise, and nothing changes.
 * The update is the last launch of stvo_seq_step_dev, behind the step's own bookkeeping: should that launch fail, the call returns
 * the error but the step counts as taken (the frame index has moved on, its results are readable), and so does its ring row. */
int stvo_seq_set_trajectory(stvo_seq* seq, const stvo_traj_params* prm, int log_steps);
/* The records of the last min(n_last, log_steps, tracked steps) steps, oldest first, into records [n_last][B] (host); *n_got = how
 * many steps.  Synchronises the context's stream (after stvo_seq_push / stvo_seq_read it is idle already).  STVO_ERR_INVALID_ARG
 * when the trajectory is off. */
int stvo_seq_read_trajectory(stvo_seq* seq, int n_last, stvo_traj_record* records, int32_t* n_got);
/* The device state [B], for callers that chain their own kernels on the context's stream. */
int stvo_seq_trajectory_state_dev(stvo_seq* seq, stvo_traj_state** state_dev);
/* A host copy of the state [B] behind everything enqueued so far (copied on the context's stream; synchronises). */
int stvo_seq_read_trajectory_state(stvo_seq* seq, stvo_traj_state* state /* [B] host */);

/* ---- restart and park single streams between steps ---------------------------------------------------------------------- */

/* One control word per stream for the NEXT step of the pipeline (stvo_seq_step_dev / stvo_seq_push), then all-RUN again:
 *   RUN      as without a control;
 *   RESTART  the frame in the slot is the first frame of a new sequence — StereoFrameHandler::initialize
 *            (src/stereoFrameHandler.cpp:35-52; the app calls no optimizePose / updateFrame for it): its stereo association runs and
 *            counts[b][0..1] report it; the stream's pose result reads as all-zero bytes (as stvo_seq_read reports a pipeline's very
 *            first frame) and counts[b][2..3] are 0; nothing of the previous sequence reaches a later result; the motion-model seed of
 *            the next step is the identity (:45); with the trajectory on, the stream's state becomes what stvo_traj_init_dev writes
 *            and its ring record of this step is all-zero (frame == 0: no pose in this step), so the next tracked frame is frame 1;
 *            with fetch enabled its f2f match rows and inlier rows are -1, its stereo match rows those of the new frame;
 *   PARK     the stream has no sequence at the moment: the step still builds the stereo set of whatever the slot holds (a following
 *            RUN tracks against it, a following RESTART ignores it); result all-zero, counts[b][2..3] 0, ring record all-zero, seed
 *            identity; trajectory state and key-frame members stay bit for bit (the final pose of a finished sequence stays readable).
 * In the pipeline's own first step nothing is tracked anyway: a control staged for it is consumed without effect.
 * ctl_host [B] is read during the call.  Values outside 0 .. 2: STVO_ERR_INVALID_ARG and nothing changes.  All zero: accepted, nothing
 * is staged (a control staged earlier for the same step is withdrawn).  Otherwise the words travel to the device NOW, on the context's
 * stream, through pinned staging that is not reused before its copy has completed — so that kernels enqueued before the step
 * (stvo_seq_restart_fast_dev) read them.  No synchronisation.  A step that carries a control gives up the key-line stage ahead and the
 * event-free fork of single-stream operation, and adds two small launches; every other step is enqueued exactly as before. */
#define STVO_STREAM_RUN 0
#define STVO_STREAM_RESTART 1
#define STVO_STREAM_PARK 2
int stvo_seq_control_next_step(stvo_seq* seq, const int32_t* ctl_host /* [B] */);
/* th_dev[b] = th0 (1 .. 254) for the streams the STAGED control marks RESTART, enqueued on the context's stream: the FAST threshold is
 * orb_fast_th again before the restart frame is detected (:38 precedes :41-42), so call it before that detection.  Nothing is
 * launched when nothing is staged.  stvo_seq_adapt_fast_dev behind a step that carried a control leaves the thresholds of its RESTART
 * and PARK streams alone (initialize has no updateFrame). */
int stvo_seq_restart_fast_dev(stvo_seq* seq, int32_t* th_dev /* [B] */, int th0);
/* The camera of the sequence a RESTART stream begins: the reference builds one PinholeStereoCamera per dataset (app/imagesStVO.cpp:66), and
 * kitti00-02 / 03 / 04-10 differ in focal length, principal point, baseline and image size (hence in the grid scale 64 / cols, 48 / rows
 * of src/stereoFrame.cpp:47-48).  Call it after stvo_seq_control_next_step for the same step: for every stream the STAGED control marks
 * RESTART, the calibration, the grid scale and the image size of the stream become cams_host[b], img_cols[b], img_rows[b] before that
 * step's first kernel reads them; entries of RUN and PARK streams are not read.  All three arrays [B], read during the call.
 * STVO_ERR_INVALID_ARG and nothing changes: no control staged, no RESTART in it, a size <= 0 for a RESTART stream.  No synchronisation:
 * pinned staging as for the control words, one small launch on the context's stream, device memory of its own.  A snapshot exported
 * afterwards carries the new camera and stvo_seq_import_streams checks a blob against it.  A RESTART without this call keeps the
 * stream's camera.  The cameras are taken when the call is made: a control withdrawn afterwards (an all-RUN
 * stvo_seq_control_next_step) does not bring the old cameras back, and the next step is still ordered behind the update. */
int stvo_seq_restart_cameras(stvo_seq* seq, const stvo_cam* cams_host /* [B] */, const int32_t* img_cols, const int32_t* img_rows);

/* ---- feature tracks and key-frame sets per stream ------------------------------------------------------------------------- */

/* What a consumer of new_kf needs beside the pose: the identity of every feature of a stream's current stereo set (stvo_track:
 * which feature of the last key-frame it observes, since how many frames, whether the pose kernel kept it) and the stereo set of the
 * stream's last key-frame itself, which the pipeline overwrites three steps later.  Off by default: nothing is allocated, nothing
 * launched.  On: every step (the first included) ends with ONE launch on the context's stream, behind the pose kernel, the control
 * kernel and the trajectory update.  Per stream, for key-points and key-lines alike, with i1 over the previous stereo set and
 * i2 = m12[i1] its f2f match (what stvo_seq_fetch_matches reports):
 *   matched i2     idx, kf of i1's record; age + 1 (saturating at 65535); inlier = the pose kernel's flag of i1 (what
 *                  stvo_seq_fetch_inliers reports).  Several i1 naming one i2 (best_lr_matches off): the largest i1 wins;
 *   unmatched i2   idx = i2, age 0, kf 0, inlier -1;
 *   first step of the pipeline and RESTART (StereoFrameHandler::initialize):  idx = i2, age 0, kf 1, inlier -1;
 *   PARK           idx = i2, age 0, kf 0, inlier -1 (the frame belongs to no sequence);
 *   key-frame      the first step, RESTART, and a step whose trajectory record has new_kf = 1 (trajectory on with keyframes): the
 *                  record keeps the values above, the state the NEXT step propagates from becomes idx = i2, age 0, kf 1 — and, with
 *                  keyframe_sets, rows [0, n) of every array of the stream's current stereo set are copied byte for byte into the
 *                  stream's key-frame set, then its header {n_pts, n_lines, frame = the pipeline step (0 = first), serial = the
 *                  key-frame's number in its sequence, 1 for a sequence's first frame}.
 * Without the trajectory there is no key-frame after a sequence's first frame.  Rows at or beyond a stream's count are never written.
 * Memory: (2 + log_steps) x B x (K + M) records of 8 bytes (K, M = stvo_seq_strides; 20 KB per stream and row at 2048 / 512) plus,
 * with keyframe_sets, B x (48 K + 152 M) bytes (about 176 KB per stream at 2048 / 512), zeroed on the context's stream.
 * Only before the first step.  log_steps >= 1: on, the records of the last log_steps steps stay readable; log_steps == 0 (with
 * keyframe_sets 0): off again.  A failed allocation returns STVO_ERR_HIP and leaves the feature off. */
int stvo_seq_set_tracks(stvo_seq* seq, int keyframe_sets /* 0 | 1 */, int log_steps);
/* The records of the last min(n_last, log_steps, steps) steps, oldest first: pts [n_last][B][K], lines [n_last][B][M],
 * counts [n_last][B][2] = {stereo points, stereo lines} (host; each may be NULL); *n_got = how many steps.  Rows [0, count) of a
 * stream are meaningful.  Synchronises the context's stream.  STVO_ERR_INVALID_ARG when the tracks are off. */
int stvo_seq_read_tracks(stvo_seq* seq, int n_last, stvo_track* pts, stvo_track* lines, int32_t* counts, int32_t* n_got);
/* Device pointers of the last step's row ([B][K], [B][M], [B][2]; each may be NULL), for kernels chained on the context's stream. */
int stvo_seq_tracks_dev(stvo_seq* seq, const stvo_track** pts_dev, const stvo_track** lines_dev, const int32_t** counts_dev);
/* The B key-frame headers, and one stream's key-frame set: the arrays and the capacity rule of stvo_seq_debug_stereo (hdr is written
 * even when the set does not fit: STVO_ERR_CAPACITY).  Both synchronise the context's stream.  STVO_ERR_INVALID_ARG unless
 * stvo_seq_set_tracks was called with keyframe_sets = 1. */
int stvo_seq_keyframe_headers(stvo_seq* seq, stvo_kf_header* hdr /* [B] host */);
int stvo_seq_read_keyframe(stvo_seq* seq, int b, stvo_kf_header* hdr, int32_t cap_pts, float* rc, uint8_t* desc, int32_t cap_lines,
                           double* spl, double* epl, double* sP, double* eP, double* le, double* s2l, double* s2lm, uint8_t* ldesc);

/* ---- export and import single streams (snapshots) ------------------------------------------------------------------------- */

/* Everything one stream carries from one step to the next, as ONE position-independent blob (no pointers: it may be written to a file
 * and read by another process, another pipeline, another stream index): rows [0, n) / [0, nl) of every array of the stereo set the last
 * step built and the counts; with the motion model the seed of the next step; with the trajectory its stvo_traj_state (the ring is a log,
 * not state); with the tracks the [K] + [M] records the NEXT step propagates from; with key-frame sets the key-frame header and rows
 * [0, hdr.n_pts) / [0, hdr.n_lines) of the set.  The FAST threshold is the caller's array and travels with the caller.
 * The blob is cut at the EXPORTING pipeline's capacities (K, M = stvo_seq_strides) and feature flags: stvo_seq_snapshot_layout gives the
 * 256-aligned offset of every section (-1: the feature is off, nothing is cut), a function of (K, M, flags) alone.  The header section
 * (256 bytes) holds a magic and a format version, bytes, K, M, flags, n, nl, the key-frame header (its `frame` names a step of the
 * EXPORTING pipeline and is carried verbatim), the stream's stvo_cam and image size, and the pipeline's stvo_match_params and
 * stvo_opt_params byte for byte.  Every byte that is no valid row and no header field is zero: two exports of the same state are
 * byte-identical. */
#define STVO_SNAP_MOTION 1   /* stvo_seq_set_motion_model */
#define STVO_SNAP_TRAJ 2     /* stvo_seq_set_trajectory */
#define STVO_SNAP_TRAJ_KF 4  /* ... with keyframes (needs STVO_SNAP_TRAJ) */
#define STVO_SNAP_TRACKS 8   /* stvo_seq_set_tracks */
#define STVO_SNAP_KF_SETS 16 /* ... with keyframe_sets (needs STVO_SNAP_TRACKS) */
typedef struct stvo_snapshot_layout {
    int64_t bytes; /* of one blob */
    int64_t off_header, off_rc, off_desc, off_spl, off_epl, off_sP, off_eP, off_le, off_s2l, off_s2lm, off_ldesc, off_motion, off_traj,
        off_tracks_p, off_tracks_l, off_kf_rc, off_kf_desc, off_kf_spl, off_kf_epl, off_kf_sP, off_kf_eP, off_kf_le, off_kf_s2l,
        off_kf_s2lm, off_kf_ldesc;
    int32_t K, M, flags, reserved;
} stvo_snapshot_layout;
/* Host only, no device.  K, M <= 0 or an illegal flag set: STVO_ERR_INVALID_ARG. */
int stvo_seq_snapshot_layout(int K, int M, int flags, stvo_snapshot_layout* out);
/* The capacities, the feature flags and the blob size of this pipeline (each pointer may be NULL). */
int stvo_seq_snapshot_info(const stvo_seq* seq, int32_t* K, int32_t* M, int32_t* flags, int64_t* bytes_per_stream);
/* Blob i (at i * bytes_per_stream) = the state of stream streams_host[i].  Reads only; legal whenever no step is half-enqueued, before
 * the first step included (an empty set and initial states).  An index outside [0, B) or a NULL pointer: STVO_ERR_INVALID_ARG; an
 * index named twice is exported twice.  _dev: blobs_dev is device memory, 16-byte aligned; ONE kernel launch on the context's stream,
 * behind the last step's launches and whatever the caller chained there, no host synchronisation (the stream list travels through
 * pinned staging that is not reused before its copy has completed).  The host form copies the blobs out and synchronises. */
int stvo_seq_export_streams_dev(stvo_seq* seq, int n, const int32_t* streams_host, void* blobs_dev);
int stvo_seq_export_streams(stvo_seq* seq, int n, const int32_t* streams_host, void* blobs_host);
/* Stream streams_host[i] holds exactly the state in blob i (at i * blob_stride; a multiple of 16, at least the blob's `bytes`): its
 * next RUN step tracks the frame in the slot against the imported stereo set with the imported seed, trajectory state, track state and
 * key-frame set, as if the stream had lived here all along (n_frames, n_keyframes, serial continue).  Streams not named keep their state
 * bit for bit.  Rows of the target at or beyond the imported counts are not written, except the track state, whose rows beyond the counts
 * become zero.  Every refusal is decided on the host before anything is enqueued and leaves the pipeline unchanged:
 *   bad magic / version / bytes, flags != this pipeline's features, camera or image size != the target stream's, stvo_match_params /
 *   stvo_opt_params != this pipeline's (byte for byte), an index out of range or named twice, blobs of more than four different
 *   (K, M) in one call                                                                                     STVO_ERR_INVALID_ARG
 *   n > K, nl > M, hdr.n_pts > K or hdr.n_lines > M of THIS pipeline (the blob's own K, M may differ)       STVO_ERR_CAPACITY
 * _dev: the n headers are fetched with one small copy, so the call synchronises the context's stream once; then one kernel launch.
 * Before the first step (the restore case; after stvo_seq_set_motion_model / set_trajectory / set_tracks, which stay "only before the
 * first step" and are refused after an import as they are after a step): the pipeline then counts as stepped — its next step tracks,
 * the streams not imported hold an empty stereo set and initial states (what PARK on an empty frame leaves), and the caller starts
 * sequences on them with RESTART.  The step after an import is enqueued as a step with a control is: it gives up the key-line stage and
 * the grid ahead and the event-free fork; a pipeline that never imports enqueues every step exactly as before. */
int stvo_seq_import_streams_dev(stvo_seq* seq, int n, const int32_t* streams_host, const void* blobs_dev, int64_t blob_stride);
int stvo_seq_import_streams(stvo_seq* seq, int n, const int32_t* streams_host, const void* blobs_host, int64_t blob_stride);

/* ---- LBD line descriptor (first half) ------------------------------------------------------- */

/* Replaces  BinaryDescriptor::createBinaryDescriptor()->compute(img, lines, ldesc)  as called by StereoFrame::detectLineFeatures
 * (src/stereoFrame.cpp:213,243,303) for B images of cols x rows bytes with up to max_keylines octave-0 key-lines each:
 * GaussianBlur(5 x 5, sigma 1), Sobel 3 x 3, the 9-band statistics of the 63-row line support region in float and in the source's
 * order of operations, both normalisations, and the 32-byte binary form (3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:
 * 350-412, 539-687, 1026-1340 — source the reference holds; semantics pinned to oracle/stvo_lbd_oracle.c, which cites it line by
 * line; parity unpinned because that file needs OpenCV to build).  The key-lines themselves come from the caller, for instance
 * stvo_lsd_detect[_dev] or stvo_fld_detect[_dev] below. */
typedef struct stvo_lbd stvo_lbd;
int stvo_lbd_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keylines, stvo_lbd** out);
int stvo_lbd_destroy(stvo_lbd* lbd);
/* Host buffers in / out, synchronises.  images [B][rows][cols]; lines [B][max_keylines]; n_lines [B]; desc [B][max_keylines][32] =
 * the rows of ldesc; desc_float (may be NULL) [B][max_keylines][72] = the float descriptor (returnFloatDescr). */
int stvo_lbd_compute(stvo_lbd* lbd, const uint8_t* images, const stvo_keyline* lines, const int32_t* n_lines, uint8_t* desc,
                     float* desc_float);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_lbd_compute_dev(stvo_lbd* lbd, const uint8_t* images, const stvo_keyline* lines, const int32_t* n_lines, uint8_t* desc,
                         float* desc_float);
/* One image SIZE per image for the following calls: the contract of stvo_orb_set_image_sizes (image i is sizes_host[i % n] = {cols,
 * rows}, n divides B, top-left of its slot at the slot's pitch, the rest of the slot influences nothing).  The descriptors, and the
 * float descriptors where asked for, of image i's key-lines are bit for bit those of a descriptor object created at (cols_i, rows_i)
 * on the crop: the 5 x 5 blur and the Sobel reflect at the image's own border and the support region is clamped to the image's own
 * last column and row.  STVO_ERR_INVALID_ARG and nothing changes: n <= 0, n > B, B % n != 0, an entry larger than the slot or below
 * 8 x 8.  No synchronisation; sizes_host == NULL: every image fills its slot again, on the kernels of an object never given a table. */
int stvo_lbd_set_image_sizes(stvo_lbd* lbd, const int32_t* sizes_host /* [n][2] = cols, rows */, int n);

/* ---- LSD line detector (second half) -------------------------------------------------------- */

/* Replaces  lsd->detect(img, lines, Config::lsdScale(), 1, opts)  + the top-N cut by response of StereoFrame::detectLineFeatures
 * (src/stereoFrame.cpp:219-240; LSDDetectorC::detectImpl, 3rdparty/line_descriptor/src/LSDDetector_custom.cpp:227-325, one
 * octave) for B images of cols x rows bytes: cv::LineSegmentDetector — third-party code the reference does not hold — as restated
 * in oracle/stvo_lsd_oracle.c from the published algorithm (parity unpinned), lsd_refine = 0 (LSD_REFINE_NONE: what every
 * shipped configuration uses) or 1 (LSD_REFINE_STD: a region too sparse for its rectangle is given back, grown again under a tolerance
 * from the angles near its seed and cut back by radius — one wavefront per image for every batch size, since flags then also turn
 * off); 2 (LSD_REFINE_ADV: rect_improve + the NFA test): STVO_ERR_UNSUPPORTED.  Images up to 2^20 pixels after scaling.  Blur, resize, gradient /
 * level-line angles and the pseudo-ordering are data-parallel kernels; region growing is inherently sequential per image (a
 * pixel joins a region depending on the running region angle and on what every earlier region took) and runs as ONE wavefront
 * per image, the images of the batch side by side.
 *
 * The scaled image (scale != 1): cv::GaussianBlur with sigma = sigma_scale / scale below scale 1 and sigma_scale above it, kernel
 * (1 + 2h) x (1 + 2h) with h = ceil(sigma sqrt(2 3 ln 10)), in OpenCV 3's 8-bit fixed point (integer weights x 2^8 per pass, one
 * rounding shift, bytes), then cv::resize(…, Size(), scale, scale).  Every pair with h = 0 .. STVO_LSD_MAX_RADIUS is built
 * (sigma <= 4.03: scale >= 0.25 at sigma_scale <= 1); a larger radius is STVO_ERR_UNSUPPORTED, a negative sigma_scale
 * STVO_ERR_INVALID_ARG.  stvo_lsd_geometry tells what a pair means without a device. */
#define STVO_LSD_MAX_RADIUS 15
#define STVO_LSD_MAX_TAPS (1 + 2 * STVO_LSD_MAX_RADIUS)
typedef struct stvo_lsd_params {
    int32_t refine;        /* Config::lsdRefine()      0 (or 1) */
    int32_t n_bins;        /* Config::lsdNBins()       1024 (1 .. 2048; more: STVO_ERR_UNSUPPORTED) */
    double scale;          /* Config::lsdScale()       1.2 */
    double sigma_scale;    /* Config::lsdSigmaScale()  0.6 */
    double quant;          /* Config::lsdQuant()       2.0 */
    double ang_th;         /* Config::lsdAngTh()       22.5 */
    double log_eps;        /* Config::lsdLogEps()      (unused: it belongs to refine 2) */
    double density_th;     /* Config::lsdDensityTh()   0.6 (read with refine 1) */
    double min_length;     /* LSDOptions::min_length = min_line_length x min(cols, rows) (stereoFrame.cpp:78) */
    int32_t nfeatures;     /* Config::lsdNFeatures()   300, 0: keep all */
    int32_t flags;         /* STVO_LSD_* bits below; other bits are ignored; 0: none (the field was `reserved`, never read) */
} stvo_lsd_params;
/* stvo_lsd_params::flags, bit 0: stvo_lsd_set_image_sizes also takes this detector when its scale is not 1 and its blur radius not 3
 * (lsd_scale : 0.5 among them).  It changes nothing at creation and nothing while no size table is set. */
#define STVO_LSD_SIZES_ANY_RADIUS 1
typedef struct stvo_lsd stvo_lsd;
/* HOST ONLY, no context: what stvo_lsd_create derives from the parameters and the image size, and the same verdict on them
 * (STVO_ERR_INVALID_ARG / STVO_ERR_UNSUPPORTED / STVO_ERR_CAPACITY exactly where stvo_lsd_create returns them; it takes its own
 * numbers from here).  Every output may be NULL: the size of the scaled image, sigma and the radius h of the blur (0, 0 at scale 1:
 * no blur), and the 1 + 2h integer weights  lrint((float)(k_i / sum) 256)  of one pass in weights[STVO_LSD_MAX_TAPS] (the rest
 * zeroed; h = 0: the single weight 256, the identity).  The weights need not add up to 256 (252 .. 259 occur), and one can BE 256. */
int stvo_lsd_geometry(const stvo_lsd_params* prm, int cols, int rows, int32_t* scaled_cols, int32_t* scaled_rows, double* sigma,
                      int32_t* radius, int32_t* weights);
int stvo_lsd_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keylines, const stvo_lsd_params* prm, stvo_lsd** out);
int stvo_lsd_destroy(stvo_lsd* lsd);
/* Host buffers in / out, synchronises.  images [B][rows][cols]; lines [B][max_keylines] (what stvo_lbd_compute consumes: in-octave
 * end points, angle, LineIterator count), response (may be NULL) [B][max_keylines] = KeyLine::response, n_lines [B]; lines come
 * in detection order, or by descending response when the top-N cut applied — also when max_keylines is what cuts (nfeatures 0 or
 * above the capacity): the strongest max_keylines lines are kept, and stvo_lsd_counts tells that a cut happened. */
int stvo_lsd_detect(stvo_lsd* lsd, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines);
/* Counts of the last detection before its cuts, host arrays [B] (either may be NULL), synchronises: n_segments = segments the
 * detector core found (the first 8192 are ranked), n_passing = those longer than min_length. */
int stvo_lsd_counts(stvo_lsd* lsd, int32_t* n_segments, int32_t* n_passing);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_lsd_detect_dev(stvo_lsd* lsd, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines);
/* Device helper between stvo_lsd_detect_dev / stvo_lbd_compute_dev and stvo_seq_upload_dev: the end points (sx, sy, ex, ey) of
 * the key-line records [B][stride] as the float rows [B][stride][4] that stvo_frame_features::kl_l / kl_r take (device pointers,
 * enqueued on the context's stream; rows beyond n_lines[b] are zeroed). */
int stvo_keylines_xy_dev(stvo_ctx* ctx, int B, int stride, const stvo_keyline* lines, const int32_t* n_lines, float* kl_xy);
/* test hook: the raw segments of the detector core (cv::LineSegmentDetector::detect), host buffers, synchronises:
 * segments [B][cap][4], n_segments [B] (all found; at most cap stored) */
int stvo_lsd_segments(stvo_lsd* lsd, const uint8_t* images, float* segments, int cap, int32_t* n_segments);
/* test hook: the image the detector core sees — blurred and resized (the input itself at scale 1) — host buffers, synchronises:
 * images [B][rows][cols] in, scaled [B][scaled_rows][scaled_cols] out (sizes: stvo_lsd_geometry); nothing is detected */
int stvo_lsd_scaled_image(stvo_lsd* lsd, const uint8_t* images, uint8_t* scaled);
/* One image SIZE, and minimum line length, per image for the following calls: the contract of stvo_orb_set_image_sizes.  Image i of the B
 * images is sizes_host[i % n] = {cols, rows}; n must divide B.  The image buffer keeps the layout [B][rows][cols] of the size given at
 * creation (the slot): image i occupies the top-left cols_i x rows_i of its slot and keeps the slot's row pitch; the bytes of the slot
 * outside the image influence nothing.  min_length_host[i % n] is the image's minimum line length (the reference's
 * Config::minLineLength() x min(width, height) of the sequence's camera); min_length_host == NULL: every entry keeps the detector's
 * min_length.  What comes back for image i is, bit for bit, what a detector created at (cols_i, rows_i) with that min_length returns
 * for the crop — key-line records, responses, n_lines, stvo_lsd_counts, stvo_lsd_segments, and the top-left scaled cols_i x scaled
 * rows_i of its slot of stvo_lsd_scaled_image (the slot's scaled pitch; the rest of that slot is not defined) — through every detect
 * entry point, for lsd_refine 0 and 1 and at every n_bins: the gradient's bounds, the largest gradient and the bins, the units of the
 * pseudo-ordering, the search's image and its smallest region, the clamps, the response divisor and the pixel count of a key-line are
 * all the image's own.
 *   The route: two are built, and stvo_lsd_set_table_route (below) chooses.  STVO_LSD_TABLE_ONE_WAVE, the default: with a table set
 * the search runs ONE wavefront per image at every batch size; the many-wave form that a detector of up to 128 images otherwise uses
 * is not launched (a small batch under a table then pays the one-wave time: README, profiles/mixed_lines_bench.json).
 * STVO_LSD_TABLE_BY_BATCH: a table does not change the route — a detector that launches the many-wave form with no table launches its
 * table-reading instance under one (README, profiles/lsd_table_route_bench.json).  Either way image i comes back bit for bit the same.
 *   STVO_ERR_INVALID_ARG and nothing changes: n <= 0, n > B, B % n != 0, an entry larger than the slot, an entry stvo_lsd_create would
 * refuse as an image size (a side below 8, nothing left after scaling), a NaN minimum length.  STVO_ERR_UNSUPPORTED and nothing
 * changes: a detector whose blur radius is not 3 at a scale other than 1 (stvo_lsd_geometry tells the radius; every shipped yaml but
 * lsd_scale : 0.5 gives 3) that was created WITHOUT STVO_LSD_SIZES_ANY_RADIUS in stvo_lsd_params::flags.  With the flag such a
 * detector is taken at every built radius 0 .. STVO_LSD_MAX_RADIUS under the same contract: its fused blur + resize then runs every
 * image under the slot's tile plan, whose LDS bounds the need of every image that fits the slot, reading nothing outside the image's
 * crop and writing nothing outside the top-left scaled size of its slot; the scaled image does not depend on the tile, so the crop
 * comes back as a detector of its own size — with its own tile — returns it.  At radius 3 and at scale 1 the flag changes nothing.
 * sizes_host and min_length_host are read during the
 * call; the table travels on the context's stream behind the detections already enqueued, through pinned staging that is not reused
 * before its copy has completed: no synchronisation.  The device table is allocated at the first call; sizes_host == NULL: every image
 * fills its slot again, on the very kernels of a detector that was never given a table. */
int stvo_lsd_set_image_sizes(stvo_lsd* lsd, const int32_t* sizes_host /* [n][2] = cols, rows */, const double* min_length_host /* [n] or NULL */,
                             int n);
/* What a size table does to the route of the search, for the detections enqueued after the call.  HOST ONLY: no device work, no
 * synchronisation.  STVO_LSD_TABLE_ONE_WAVE (the default): one wavefront per image under a table.  STVO_LSD_TABLE_BY_BATCH: the route
 * is the one the detector takes with no table — the many-wave search for a detector that holds its scratch (at most 128 images,
 * lsd_refine 0, a scaled image within the many-wave form's limit, not under STVO_LSD_WAVES=0); any other detector takes the call and
 * stays on one wave.  The results do not depend on the route.  The value survives stvo_lsd_set_image_sizes, NULL included, and means
 * nothing while no table is set.  Another value: STVO_ERR_INVALID_ARG and nothing changes. */
#define STVO_LSD_TABLE_ONE_WAVE 0
#define STVO_LSD_TABLE_BY_BATCH 1
int stvo_lsd_set_table_route(stvo_lsd* lsd, int route);
/* HOST ONLY: the search kernel the next detection launches, as things stand (parameters, batch size, table, table route, developer
 * switches).  STVO_LSD_SEARCH_ONE_WAVE: one wavefront per image, the fast growth.  STVO_LSD_SEARCH_ONE_WAVE_PLAIN: one wavefront per
 * image on the plain statement of the growth, with (lsd_refine 1) or without (STVO_LSD_GROW=0) refinement.
 * STVO_LSD_SEARCH_MANY_WAVES: a committing wave and speculating workgroups per image. */
#define STVO_LSD_SEARCH_ONE_WAVE 0
#define STVO_LSD_SEARCH_ONE_WAVE_PLAIN 1
#define STVO_LSD_SEARCH_MANY_WAVES 2
int stvo_lsd_search_route(stvo_lsd* lsd, int32_t* route);

/* ---- FLD line detector (use_fld_lines = true) -------------------------------------------------------------------------- */

/* Replaces  createFastLineDetector(min_line_length)->detect(fld_img, fld_lines)  + the top-N cut by length + the KeyLine fields of
 * StereoFrame::detectLineFeatures (src/stereoFrame.cpp:244-298) for B images of cols x rows bytes: cv::ximgproc::FastLineDetector
 * (OpenCV contrib 3.x — third-party code the reference does not hold) as restated in tests/cpp/fld_ref.c (parity unpinned, DESIGN.md
 * §10): Canny (aperture 3, L1, th1 == th2), the edge chains, extractSegments, the length / border filters and the orientation by the
 * brighter side.  Images up to 2^20 pixels, at least 16 x 16.  Canny, the 8-connected components of the edge map and the segment
 * fitting are data-parallel kernels; the chain walk runs one lane per component (exact: a chain never leaves its component).  One
 * size for all images, or one size and threshold per image (stvo_fld_set_image_sizes below). */
typedef struct stvo_fld_params {
    int32_t length_threshold;    /* (int)(min_line_length x min(cols, rows)) (stereoFrameHandler.cpp:39, truncated), >= 1 */
    float distance_threshold;    /* 1.414213562f */
    double canny_th1;            /* 50 */
    double canny_th2;            /* 50; != canny_th1 (hysteresis): STVO_ERR_UNSUPPORTED */
    int32_t canny_aperture_size; /* 3; other apertures: STVO_ERR_UNSUPPORTED */
    int32_t do_merge;            /* 0; 1: STVO_ERR_UNSUPPORTED */
    int32_t nfeatures;           /* Config::lsdNFeatures()   300, 0: keep all */
    int32_t reserved;
} stvo_fld_params;
typedef struct stvo_fld stvo_fld;
int stvo_fld_create(stvo_ctx* ctx, int B, int cols, int rows, int max_keylines, const stvo_fld_params* prm, stvo_fld** out);
int stvo_fld_destroy(stvo_fld* fld);
/* Host buffers in / out, synchronises.  Output as stvo_lsd_detect's: lines [B][max_keylines] (what stvo_lbd_compute consumes: end
 * points, angle = atan2(ey - sy, ex - sx), LineIterator count), response (may be NULL) [B][max_keylines] = lineLength / max(cols,
 * rows), n_lines [B]; detection order, or by descending length when the top-N cut applied — also when max_keylines is what cuts
 * (nfeatures 0 or above the capacity).  STVO_ERR_CAPACITY if an internal store filled up (never drops a point silently). */
int stvo_fld_detect(stvo_fld* fld, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_fld_detect_dev(stvo_fld* fld, const uint8_t* images, stvo_keyline* lines, float* response, int32_t* n_lines);
/* Segments the last detection found before its cuts, host array [B], synchronises (the first 8192 are ranked). */
int stvo_fld_counts(stvo_fld* fld, int32_t* n_segments);
/* test hooks, host buffers, synchronise: the raw segments of FastLineDetector::detect in detection order, segments [B][cap][4],
 * n_segments [B] (all found; at most min(cap, 8192) stored); the edge map the chains are walked on (corner quirk applied),
 * edges [B][rows][cols] = 0 / 255. */
int stvo_fld_segments(stvo_fld* fld, const uint8_t* images, float* segments, int cap, int32_t* n_segments);
int stvo_fld_edges(stvo_fld* fld, const uint8_t* images, uint8_t* edges);
/* One image SIZE, and length threshold, per image for the following calls: the contract of stvo_lsd_set_image_sizes.  Image i of the B
 * images is sizes_host[i % n] = {cols, rows}; n must divide B.  The image buffer keeps the layout [B][rows][cols] of the size given at
 * creation (the slot): image i occupies the top-left cols_i x rows_i of its slot and keeps the slot's row pitch; the bytes of the slot
 * outside the image influence nothing.  length_threshold_host[i % n] is the image's length threshold (the reference's
 * (int)(Config::minLineLength() x min(width, height)) of the sequence's camera); length_threshold_host == NULL: every entry keeps the
 * detector's.  What comes back for image i is, bit for bit, what a detector created at (cols_i, rows_i) with that threshold returns for
 * the crop — key-line records, responses, n_lines, stvo_fld_counts, stvo_fld_segments; stvo_fld_edges gives the crop's edge map
 * top-left in a slot-shaped output whose rest is 0 — through stvo_fld_detect and stvo_fld_detect_dev: the Sobel border, the corner
 * quirk, the neighbourhoods of the components and of the walk, the clamps and border filters of a segment, the chain length, the
 * response divisor and the pixel count of a key-line are all the image's own.
 *   The stores of chains and segments were cut at creation for (the slot's pixels, the detector's threshold) and an image places its
 * segments by its OWN threshold, so an entry is taken only if cols_i rows_i / (L_i + 1) + 1 <= slot pixels / (L + 1) + 1; L_i >= L
 * always satisfies it: create a detector meant for mixed sizes with the smallest threshold it will be given.
 *   STVO_ERR_INVALID_ARG and nothing changes: n <= 0, n > B, B % n != 0, an entry larger than the slot, a side below 16, a threshold
 * below 1.  STVO_ERR_CAPACITY and nothing changes: an entry the store rule refuses (stvo_ctx_last_error names it and both capacities).
 * sizes_host and length_threshold_host are read during the call; the table travels on the context's stream behind the detections
 * already enqueued, through pinned staging that is not reused before its copy has completed: no synchronisation.  The device table is
 * allocated at the first call; sizes_host == NULL: every image fills its slot again, on the very kernels of a detector that was never
 * given a table. */
int stvo_fld_set_image_sizes(stvo_fld* fld, const int32_t* sizes_host /* [n][2] = cols, rows */,
                             const int32_t* length_threshold_host /* [n] or NULL */, int n);

/* ---- stereo rectification (input preparation of Dataset::nextFrame, src/dataset.cpp:147-157) ---------------------------- */

/* Replaces the rectification half of  PinholeStereoCamera(const string& params_file)  (src/pinholeStereoCamera.cpp:30-125):
 * stereoRectify(CALIB_ZERO_DISPARITY, alpha 0) in the form of OpenCV 3.4's cvStereoRectify, then initUndistortRectifyMap (rad-tan)
 * or fisheye::initUndistortRectifyMap per side, CV_16SC2 maps (DESIGN.md §9 states the form and what stays unpinned).  Host only,
 * no device needed.  map1 [2][rows][cols][2] int16 (integer source position) and map2 [2][rows][cols] uint16 (5-bit fractions,
 * iv & 31) * 32 + (iu & 31)), left side first; either may be NULL.  Form KITTI: both sides hold the left map (:119-120). */
int stvo_rectify_compute(const stvo_rect_calib* calib, stvo_rect_camera* out, int16_t* map1, uint16_t* map2);

/* Replaces  PinholeStereoCamera::rectifyImagesLR / rectifyImage  (src/pinholeStereoCamera.cpp:196-208): cv::remap(INTER_LINEAR,
 * BORDER_CONSTANT 0) of 8-bit images with the CV_16SC2 maps, bit for bit, or a copy when dist is 0.  One rectifier serves up to
 * B stereo pairs per call; the maps stay resident in HBM. */
typedef struct stvo_rectify stvo_rectify;
int stvo_rectify_create(stvo_ctx* ctx, int B, const stvo_rect_calib* calib, stvo_rectify** out);
/* Caller-made maps (own calibration tools): map1 / map2 as stvo_rectify_compute writes them, both sides; dist = 1. */
int stvo_rectify_create_from_maps(stvo_ctx* ctx, int B, int cols, int rows, const int16_t* map1, const uint16_t* map2,
                                  stvo_rectify** out);
int stvo_rectify_destroy(stvo_rectify* rect);
int stvo_rectify_camera(const stvo_rectify* rect, stvo_rect_camera* out);
/* n (1 .. B) pairs: src_l / dst_l hold n left images and src_r / dst_r n right images, rows * cols bytes apart; the left map applies
 * to the left images, the right map to the right ones.  A destination that overlaps any source is STVO_ERR_INVALID_ARG.
 * Host buffers, synchronises. */
int stvo_rectify_images(stvo_rectify* rect, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_rectify_images_dev(stvo_rectify* rect, int n, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l, uint8_t* dst_r);

/* ---- colour images in (8-bit interleaved B, G, R or B, G, R, A; alpha is ignored) -------------------------------------- */

/* The reference reads its images unchanged and rectifies them with all their channels; every consumer then makes its own grey
 * image: cv::ORB, LSDDetectorC::detect and BinaryDescriptor::compute with COLOR_BGR2GRAY, the FLD branch with CV_RGB2GRAY on the
 * same bytes (src/stereoFrame.cpp:249-258), which swaps the weights of channels 0 and 2.  weights: cvtColor's 8-bit integer form,
 * (wb blue + wg green + wr red + 2^(s-1)) >> s with (1868, 9617, 4899), s = 14 (OpenCV 3.0 - 3.4.1) or (3735, 19235, 9798), s = 15
 * (later releases); the two differ by one grey level on 43 864 of the 2^24 triples.  order: which colour channel 0 holds. */
#define STVO_GRAY_Q14 0
#define STVO_GRAY_Q15 1
#define STVO_ORDER_BGR 0
#define STVO_ORDER_RGB 1
/* src [n][rows][cols][channels] -> gray [n][rows][cols] in the given order and, where gray_swapped is not NULL, the plane of the
 * other order (red and blue weights swapped) from the same pass.  channels other than 3 and 4, a NULL src / gray, or a plane that
 * overlaps the source or the other plane: STVO_ERR_INVALID_ARG.  Host buffers, synchronises. */
int stvo_color_to_gray(stvo_ctx* ctx, int n, int rows, int cols, int channels, int order, int weights, const uint8_t* src, uint8_t* gray,
                       uint8_t* gray_swapped);
/* The same with DEVICE pointers of any alignment, enqueued on the context's stream (no synchronisation). */
int stvo_color_to_gray_dev(stvo_ctx* ctx, int n, int rows, int cols, int channels, int order, int weights, const uint8_t* src,
                           uint8_t* gray, uint8_t* gray_swapped);
/* rectifyImagesLR on colour images: stvo_rectify_images with rows * cols * channels bytes per image, every channel remapped and
 * rounded as a grey image is (a copy when dist is 0).  n > B, channels other than 3 and 4, a NULL pointer or a destination that
 * overlaps a source or the other destination: STVO_ERR_INVALID_ARG.  Host buffers, synchronises. */
int stvo_rectify_color_images(stvo_rectify* rect, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                              uint8_t* dst_r);
/* The same with DEVICE pointers, enqueued on the context's stream (no synchronisation). */
int stvo_rectify_color_images_dev(stvo_rectify* rect, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                                  uint8_t* dst_r);
/* Raw colour pairs -> the grey planes of the rectified colour images in one kernel: every colour channel is remapped and rounded to
 * 8 bits, then weighted; the rectified colour image is never written (with dist 0: the plain conversion).  gray_l / gray_r [n][rows]
 * [cols] in the given order; swapped_l / swapped_r the other order, both or neither NULL.  DEVICE pointers, no synchronisation. */
int stvo_rectify_color_to_gray_dev(stvo_rectify* rect, int n, int channels, int order, int weights, const uint8_t* src_l,
                                   const uint8_t* src_r, uint8_t* gray_l, uint8_t* gray_r, uint8_t* swapped_l, uint8_t* swapped_r);

/* ---- one rectifier for mixed cameras: a calibration and an image size per pair of one launch ---------------------------- */

/* A bank over K rectifiers of the same context (from stvo_rectify_create, any form, dist 0 or 1, or stvo_rectify_create_from_maps), each
 * no larger than the slot slot_cols x slot_rows, for up to B pairs per call.  The bank BORROWS the rectifiers' resident maps and copies
 * nothing: every rectifier must outlive the bank (destroy the bank first).  Every pair starts on calibration 0.
 * Images are slot-shaped, the layout stvo_orb_set_image_sizes reads: buffers are [n][slot_rows][slot_cols][channels], and image b
 * occupies the top-left cols_k x rows_k of its slot at the slot's row pitch, k being the calibration of pair b. */
typedef struct stvo_rectify_bank stvo_rectify_bank;
int stvo_rectify_bank_create(stvo_ctx* ctx, int B, int slot_cols, int slot_rows, stvo_rectify* const* rects, int K,
                             stvo_rectify_bank** out);
int stvo_rectify_bank_destroy(stvo_rectify_bank* bank);
/* stvo_rectify_camera of rectifier k. */
int stvo_rectify_bank_camera(const stvo_rectify_bank* bank, int k, stvo_rect_camera* out);
/* Pair b takes calibration calib_of_pair_host[b] (0 .. K - 1) for the calls that follow.  An index out of range:
 * STVO_ERR_INVALID_ARG and nothing changes.  calib_of_pair_host is read during the call; the split of the work it implies travels on
 * the context's stream behind the calls already enqueued, through pinned staging that is not reused before its copy has completed: no
 * synchronisation (the contract of stvo_orb_set_image_sizes). */
int stvo_rectify_bank_assign(stvo_rectify_bank* bank, const int32_t* calib_of_pair_host /* [B] */);
/* n (1 .. B) pairs, channels 1, 3 or 4, DEVICE pointers, ONE kernel launch on the context's stream for all calibrations and both sides,
 * no synchronisation.  For every pair the crop of the destination is, bit for bit, what rectifier k alone returns for the crop of the
 * source (stvo_rectify_images_dev / stvo_rectify_color_images_dev; with dist 0 a copy of the crop): a tap outside the image reads 0
 * even where it lies inside the slot, and no byte of the destination outside the crop is written.  A NULL pointer, n or channels out
 * of range, a destination that overlaps a source or the other destination: STVO_ERR_INVALID_ARG. */
int stvo_rectify_bank_images_dev(stvo_rectify_bank* bank, int n, int channels, const uint8_t* src_l, const uint8_t* src_r, uint8_t* dst_l,
                                 uint8_t* dst_r);
/* The fused form, per pair the contract of stvo_rectify_color_to_gray_dev (every channel remapped and rounded to 8 bits, then weighted;
 * with dist 0 the plain conversion) in the slot layout: src [n][slot_rows][slot_cols][channels] (3 or 4), planes [n][slot_rows]
 * [slot_cols]; swapped_l / swapped_r both or neither NULL.  One launch, nothing written outside the crops, no synchronisation. */
int stvo_rectify_bank_color_to_gray_dev(stvo_rectify_bank* bank, int n, int channels, int order, int weights, const uint8_t* src_l,
                                        const uint8_t* src_r, uint8_t* gray_l, uint8_t* gray_r, uint8_t* swapped_l, uint8_t* swapped_r);

/* ---- measurement helpers --------------------------------------------------------------------- */
/* Times `iters` launches of the named kernel stage on the context's stream with hipEvents and
 * returns the average milliseconds per launch (used by bench.py for the roofline line).
 * stage: 0 = the forward top-2 scan (K1m hamming_knn2_mfma, or K1 hamming_knn2 for contexts beyond 8192 rows /
 * STVO_KNN_MFMA=0), 1 = pose kernel, 3 = the reverse-check scans (K1m's two sparse scans, or K1v hamming_verify) on
 * the column claims and lists left by the last stvo_track_batched_dev call. */
int stvo_time_stage_dev(stvo_ctx* ctx, const stvo_track_batch_dev* batch, const stvo_cam* cam,
                        const stvo_opt_params* params, float nnr, int stage, int iters, float* avg_ms);

/* Live timing of the dominant kernel INSIDE the batched path: with enable = 1 every stvo_track_batched_dev
 * call brackets its forward top-2 scan and its reverse (mutual) check — planning kernel + scans — on
 * the point descriptors with hipEvents on the stream they are launched on.  get_kernel_timing synchronises,
 * returns the average duration of each and the number of calls measured since the last get / set, and
 * resets the pool. */
int stvo_ctx_set_kernel_timing(stvo_ctx* ctx, int enable);
int stvo_ctx_get_kernel_timing(stvo_ctx* ctx, float* avg_ms_forward, float* avg_ms_reverse, int32_t* n_calls);

/* Number of right-hand (curr) rows the LAST batched mutual match had to verify, per frame pair (only columns
 * claimed by some row's accepted forward match are examined). */
int stvo_last_reverse_counts(stvo_ctx* ctx, int B, int32_t* counts);
/* The plan of the LAST mutual match's reverse check on the matrix cores (B = the batch size of that call; 1 for
 * stvo_match_nnr_mutual), plan = [5][B]: claimed columns; LIGHT columns (verified against the few rows whose second-best
 * forward distance is within the cut); HEAVY columns (verified against every row); |S| = number of such rows; the cut tau
 * (-1: every column heavy).  Diagnostics for tests and bench.py; meaningless after a match that took the VALU kernels. */
int stvo_last_reverse_plan(stvo_ctx* ctx, int B, int32_t* plan);

/* Integer-VALU micro-benchmark (xor + popcount-accumulate chains, no memory traffic): measured
 * 32-bit lane-ops/s of this device, the empirical roof K1 is priced against. */
int stvo_valu_peak_probe(stvo_ctx* ctx, double* lane_ops_per_s);

/* Developer switches (csrc/debug_switches.h lists every STVO_* environment variable the library knows): they are parsed once,
 * on first use; this re-reads the environment so that one test process can drive several kernel variants. */
void stvo_debug_reparse_env(void);

#ifdef __cplusplus
}
#endif
#endif /* STVO_HIP_H */
