// kernels.h — internal launch interface between the C-ABI translation unit and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "../../include/stvo_hip.h"
#include "debug_switches.h"
#include "grid_scratch.h"
#include "lsd_scale_plan.h"
#include "match_scratch.h"
#include "point_tail.h"
#include "pose_scratch.h"
#include "seq_layout.h"

namespace stvo {

// More than 64 KB of dynamic LDS per workgroup needs an explicit opt-in, and hipFuncSetAttribute applies to the CURRENT device
// only: the largest size granted so far is remembered per (kernel, device) — a later, larger request raises the attribute again
// (a kernel whose dynamic LDS depends on the problem, e.g. the fused line matcher, must not run on a stale smaller opt-in).
inline bool lds_opt_in(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int> granted;  // bytes granted, -1: the runtime refused
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kernel, dev);
    const auto it = granted.find(key);
    if (it != granted.end() && (it->second >= bytes || it->second < 0)) return it->second >= bytes;
    const bool ok = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    if (ok) granted[key] = bytes;
    else if (it == granted.end()) granted[key] = -1;
    return ok;
}

// CUs of the current device (persistent-workgroup launches size their grids with it), cached per device
inline int device_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> lk(mu);
    const auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
    return n;
}

// ---- the brute-force descriptor matcher: StVO::match of B frame pairs (match_kernels.hip, match_mfma.hip) ----------------------
// cv::BFMatcher(NORM_HAMMING).knnMatch(., ., 2) + the ratio test of StVO::matchNNR + the mutual check of StVO::match.  The scratch
// it works in, and what a problem needs of it: match_scratch.h.  Two paths, chosen once per launch_match from the row count: the
// matrix cores (K1m, row_stride <= 8192) or the VALU kernels (beyond, and under STVO_KNN_MFMA=0).
struct MatchProblem {
    int B, row_stride;  // frame pairs; rows per frame of d1, d2 and m12
    const uint8_t* d1;  // [B][row_stride][32] descriptors of the previous frames, n1[b] rows valid
    const int32_t* n1;  // [B]
    const uint8_t* d2;  // the current frames
    const int32_t* n2;
    float nnr;          // ratio of the test, <= 1
};
enum class MatchForm {  // (the vocabulary of step_plan.h: MatchRoute; its SMALL is launch_match_small below)
    ONE_WAY,    // forward scan, ratio test (nnr_mutual_kernel): no mutual check
    BOTH_DIRS,  // both directions as full scans in one launch, ratio tests + mutual check (nnr_mutual_kernel)
    LAZY,       // mutual check by a reverse pass over the claimed columns only.  Matrix cores: forward scan, forward_plan_kernel,
                // hamming_knn2_mfma_reverse_kernel.  VALU: forward scan, nnr_forward_kernel, compact_need_kernel, hamming_verify_kernel,
                // nnr_reverse_check_kernel
};
struct MatchOptions {  // every default is "none"
    int lds_pad_bytes = 0;                   // VALU scans only: dynamic LDS that caps the resident workgroups per CU (stvo_ctx_set_overlap)
    hipEvent_t wait_before_m12 = nullptr;    // awaited on the stream before the first kernel that writes m12
    hipEvent_t* timing_events = nullptr;     // LAZY only: [0], [1] recorded around the forward scan, [2], [3] (either may be null) around the reverse pass
    int nseg_cap = 0;                        // > 0: at most this many train segments per query tile (MatchPlan::nseg_cap)
};
// m12[b][i] = the match of row i of frame pair b, or -1; everything on stream s, in the order named at MatchForm
void launch_match(hipStream_t s, const MatchProblem& p, MatchForm form, const MatchScratch& w, int32_t* m12, const MatchOptions& o = MatchOptions());
// single launches of the above, for timing tools (stvo_time_stage_dev): the forward scan; both directions as full scans; the reverse
// scans of the LAZY form on the claims the last launch_match left in w (they clear the same entries of m12 again)
void launch_forward_scan_alone(hipStream_t s, const MatchProblem& p, const MatchScratch& w, int lds_pad_bytes);
void launch_both_dirs_scan_alone(hipStream_t s, const MatchProblem& p, const MatchScratch& w, int lds_pad_bytes);
void launch_reverse_check_alone(hipStream_t s, const MatchProblem& p, const MatchScratch& w, int lds_pad_bytes, int32_t* m12);
// between match_kernels.hip and match_mfma.hip: one top-2 scan (out: knn12, and knn21 with both_directions; [nseg][B][row_stride] each)
struct KnnScan {
    const MatchProblem& p;
    int nseg;
    bool both_directions;
    uint2 *knn12, *knn21;
    uint32_t* claim_init;  // or nullptr: [B][row_stride] reset to "unclaimed" on the way (VALU path of LAZY)
};
// K1m hamming_knn2_mfma_kernel<qb, 0>: qb = query blocks of 32 rows per wave (1, 2 or 4; a workgroup covers 128 * qb query rows).
// Train indices must fit 13 bits (row_stride <= 8192).
void launch_hamming_knn2_mfma(hipStream_t s, const KnnScan& a, int qb);
// hamming_knn2_mfma_reverse_kernel: the reverse check of the claimed columns in one launch — light columns against S (v.tsel), heavy
// columns against all rows; `slots` workgroups per frame pair share the frame's units; m12[claimant] = -1 for every listed column
// whose claim another row blocks
void launch_hamming_knn2_mfma_reverse(hipStream_t s, const MatchProblem& p, const MatchViews& v, int32_t* m12, int slots);
// StVO::match of B frame pairs with at most 512 rows per set (key-lines): one workgroup per frame pair, both sets in LDS
bool match_small_ok(int row_stride);
void launch_match_small(hipStream_t s, int B, int row_stride, const uint8_t* d1, const int32_t* n1, const uint8_t* d2,
                        const int32_t* n2, float nnr, int mutual, int32_t* m12, int cap = 0 /* rows per set the LDS is sized for; 0: row_stride */);
void launch_valu_probe(hipStream_t s, int blocks, int iters, uint32_t* sink);
// 16-byte-granular copy kernel; either side may be pinned host memory.  For the few hundred KB a single-stream call
// moves it has ~5 us less latency than the DMA engine behind hipMemcpyAsync (6 us vs 11 us on top of an empty launch,
// and ~0 vs 3 us for a result block written straight into pinned memory).
void launch_copy16(hipStream_t s, const void* src, void* dst, size_t bytes);
extern const double kValuProbeOpsPerThreadIter;

// ---- K4-K6: pose optimisation, one workgroup per frame pair (pose_kernel.hip, pose_kernel2p.hip) ------------------------------
// StereoFrameHandler::optimizePose of B frame pairs.  A launch is a problem, the stereo points in ONE of two record forms, and what
// it may be given on top (PoseOptions); the route it takes and the arena it needs: pose_scratch.h.  The kernels are handed one flat
// by-value copy of all of it (pose_args.h, private to the two pose files).
// The problem: what optimizePose takes, batched.
struct PoseProblem {
    int B, max_pts, max_lines;  // frame pairs; rows per frame of the point / key-line arrays
    const int32_t* n_prev_pts;  // [B], or nullptr: no points
    const int32_t* m12p;        // [B][max_pts] match of prev point i, or nullptr: identity association (records mode)
    const int32_t* init_inl_p;  // nullptr: every matched record starts as inlier
    // the key-line records
    const int32_t* n_prev_lines;
    const double* prev_sP;
    const double* prev_eP;
    const double* prev_spl;
    const double* prev_epl;
    const double* prev_s2l;
    const double* curr_le;
    const int32_t* m12l;
    const int32_t* init_inl_l;
    const double* init_T;  // [B][16] or nullptr
    double* next_T;        // [B][16] or nullptr: the next frame pair's init_T under use_motion_model (pose_block.h: t0_commit); may alias init_T
    stvo_cam cam;
    const stvo_cam* cams;  // [B] per-frame-pair calibration (device) or nullptr: `cam` for every pair
    stvo_opt_params prm;
    stvo_pose_result* results;
    int32_t* inl_p_out;  // [B][max_pts] or nullptr
    int32_t* inl_l_out;
};
// The stereo point records, [B][max_pts] each, in one of two forms (doubles() / compact() make one and leave the other empty):
//   doubles   P, sigma2 of prev point i and the observation of curr point j, as the C-ABI's batches hold them;
//   compact   of the device-resident pipeline (seq_pipeline.hip): a stereo point is {u, v, disparity as floats, pyramid level} —
//             exactly what the reference's PointFeature is built from (src/stereoFrame.cpp:152-167: float key-point coordinates, a
//             float difference, backProjection of the three) — so P, sigma2 and the observation are recomputed on chip instead of
//             being stored and re-read as seven doubles.  prev_rc[i] gives P and sigma2 of prev point i, curr_rc[j] the observation.
// Half a compact form (prev_rc without curr_rc / q_tab) is STVO_ERR_INVALID_ARG.
struct PosePoints {
    const double *prev_P = nullptr, *prev_s2p = nullptr, *curr_pl = nullptr;
    const float4 *prev_rc = nullptr, *curr_rc = nullptr;
    const double* q_tab = nullptr;  // [STVO_POSE_QTAB] sqrt(sigma2) of pyramid level l (device memory; levels beyond the table are computed)
    double level_scale = 0.0;       // orbScaleFactor: sigma2 = 1 / scale^(2 level) (src/stereoFeatures.cpp:41-47)
    bool is_compact() const { return prev_rc != nullptr; }
    static PosePoints doubles(const double* prev_P, const double* prev_s2p, const double* curr_pl) {
        PosePoints r;
        r.prev_P = prev_P; r.prev_s2p = prev_s2p; r.curr_pl = curr_pl;
        return r;
    }
    static PosePoints compact(const float4* prev_rc, const float4* curr_rc, const double* q_tab, double level_scale) {
        PosePoints r;
        r.prev_rc = prev_rc; r.curr_rc = curr_rc; r.q_tab = q_tab; r.level_scale = level_scale;
        return r;
    }
};
// In-kernel ordering for single-stream operation, instead of events between streams — on this runtime every recorded / awaited event
// delays the next kernel of its stream by ~6 us.  Every device is absent by default; which of them a launch honours: PoseRoute.
struct PoseSync {
    // the kernel starts by waiting until *wait_flag has reached wait_value (device memory, set by launch_stream_signal behind the last
    // kernel of another stream whose results this launch reads).  PoseRoute::inline_sync, else the launch is refused.
    const unsigned* wait_flag = nullptr;
    unsigned wait_value = 0;
    // the solver wave of workgroup 0 copies fetch_n16 16-byte words (by-products the host wants while this kernel runs) to pinned host
    // memory and then publishes fetch_value in *fetch_flag (pinned, system scope).  PoseRoute::inline_sync, else the launch is refused.
    const uint4* fetch_src = nullptr;
    uint4* fetch_dst = nullptr;
    unsigned fetch_n16 = 0;
    unsigned* fetch_flag = nullptr;
    unsigned fetch_value = 0;
    // the FIRST workgroup of the launch publishes start_value in *start_flag when it starts — the launch is taking its CUs (1024
    // workgroups are placed within a few microseconds).  PoseRoute::start_flag, ignored otherwise.  seq_pipeline.hip holds the next
    // step's key-line kernels behind it (launch_stream_gate), so that their workgroups do not take the CUs first.  Not the LAST
    // workgroup: 1024 frame pairs fill every VGPR of the chip (2 waves x 256 registers per SIMD), so the SIMD that hosts the waiting
    // gate wave has room for one pose wave only — the last workgroup could not start before the gate left, and the gate waited for the
    // last workgroup: a circular wait that resolved only when the first frame pair of the launch finished, 160 us later (round 6: every
    // second pipeline of a process ran 0.864 instead of 0.793 ms per step that way, depending on where the gate wave had landed).
    unsigned* start_flag = nullptr;
    unsigned start_value = 0;
    // != 0 (latency kernel only; the caller reads the results through stvo_seq_read): cov_eig is left to the reader, flagged in
    // stvo_pose_result::path (PATH_EIG_PENDING)
    int lazy_eig = 0;
};
struct PoseOptions {  // every default is "none"
    PoseSync sync;
    double* eval_out = nullptr;     // [B][44] H(36) g(6) e n: present = ONE optimizeFunctions evaluation at init_T instead of the optimisation
    int eval_robust = 0;            // != 0: that evaluation is optimizeFunctionsRobust
    long long* prof_out = nullptr;  // [B][16] phase ticks (tools only)
};
// One pose launch on `s`: the route pose_route names.  arena: device memory the batch kernels keep their records in while they run,
// at least PoseRoute::arena_bytes (STVO_ERR_CAPACITY otherwise) and the caller's until the launch has completed; nothing is allocated here.
int launch_pose(hipStream_t s, const PoseProblem& p, const PosePoints& r, void* arena, size_t arena_bytes, const PoseOptions& o = PoseOptions());
// the route of a launch on the current device under the developer switches in force
inline PoseRoute pose_route(int B, bool compact, bool eval) {
    const DebugSwitches& sw = dbg();
    return pose_route(B, compact, eval, pose_takes_batch_kernel(B, eval, sw) ? device_cu_count() : 0, sw);
}
// one thread that leaves when *flag has reached value, or after 3000 polls ~0.45 us apart, ~1.3-1.5 ms (a scheduling hint, never a
// dependence)
void launch_stream_gate(hipStream_t s, const unsigned* flag, unsigned value);
constexpr int STVO_POSE_QTAB = 16;
// internal flag in stvo_pose_result::path (never leaves the library): the eigenvalues of `cov` are still to be computed by the reader
constexpr int PATH_EIG_PENDING = 1 << 30;
// *flag = value (release, device scope) once everything enqueued on `s` so far has completed
void launch_stream_signal(hipStream_t s, unsigned* flag, unsigned value);

// ---- 8-bit image operations of the ORB front-end that the line detector reuses (orb_kernels.hip) ----
// cv::GaussianBlur(7 x 7) in 8-bit fixed point with the integer kernel k7 (weights x 2^8), BORDER_REFLECT_101
// sz (device, or nullptr: every image fills cols x rows): one size per image, image b being the top-left of its cols x rows slot at the
// slot's pitch, sized by row (b % n_sz) * sz_stride + level of the table (orb_sizes.h) — the MIXED instance of the kernel
struct OrbLevelSize;
void launch_blur7_u8(hipStream_t s, int B, int cols, int rows, const uint8_t* src, uint8_t* dst, const int* k7, const OrbLevelSize* sz = nullptr,
                     int n_sz = 0, int sz_stride = 0, int level = 0);
// cv::resize(INTER_LINEAR) for 8-bit images, 11-bit fixed point; fx = fy = 0: resize to a given dsize (sample step ssize / dsize),
// fx, fy > 0: resize(src, dst, Size(), fx, fy) with dsize = cvRound(ssize f) — the sample step stays 1 / f (LSD's scaled image).
// sz: as above, from row `level - 1` (the source) to row `level` (the destination and its inverse scales) of image b's entry
void launch_resize_linear_u8(hipStream_t s, int B, int scols, int srows, int dcols, int drows, const uint8_t* src, uint8_t* dst, double fx = 0.0,
                             double fy = 0.0, const OrbLevelSize* sz = nullptr, int n_sz = 0, int sz_stride = 0, int level = 0);
// ---- the same two operations fused, for every blur radius 0 .. STVO_LSD_MAX_RADIUS (lsd_scale_kernels.hip) ----
// cv::GaussianBlur((1 + 2 radius)^2) with the integer weights (x 2^8, 32-bit: one can be 256) + cv::resize(…, Size(), scale, scale):
// one workgroup per tile of the scaled image, the blurred bytes only in LDS.  The plan (tile, dynamic LDS) depends on the geometry
// alone and is made once (lsd_scale_plan.h: BlurResizePlan, plan_blur_resize_u8; false: no tile fits the LDS, scales far below 0.01).
// sz (device, or nullptr: every image fills scols x srows): one size per image, image b being the top-left of its slot at the slot's
// pitch — source and scaled — sized by row b % n_sz of the detector's table (lsd_sizes.h), under the SLOT's plan, which bounds the
// need of every image that fits the slot (lsd_scale_plan.h) — the MIXED instance of the kernel
struct LsdSizeRow;
void launch_blur_resize_u8(hipStream_t s, int B, int scols, int srows, int dcols, int drows, const uint8_t* src, uint8_t* dst, double scale,
                           int radius, const int* weights, const BlurResizePlan& p, const LsdSizeRow* sz = nullptr, int n_sz = 0);

// ---- K3: grid-windowed stereo matchers, batched over frame pairs (blockIdx.y) ----------------------
constexpr int GRID_LW = STVO_GRID_COLS + 16, GRID_LCELLS = STVO_GRID_ROWS * GRID_LW, GRID_LSTART_STRIDE = GRID_LCELLS + 4;
// the cells phase of the key-points of a frame (point_cells.h): what it reads and writes
struct PointCells {
    int K, ws;               // rows per frame of every array below; matching_s_ws (stereoFrame.cpp:141-143)
    const float* kp_l;       // [B][K][2]
    const float* kp_r;       // [B][K][2]
    const int32_t* n_kp_l;   // [B]
    const int32_t* n_kp_r;   // [B]
    const double* inv_wh;    // [B][2] 64 / cols, 48 / rows (stereoFrame.cpp:47-48)
    int32_t* pstart;         // [B][3073] out: exclusive cell starts of the right key-points
    uint32_t* plstart;       // [B][GRID_LSTART_STRIDE] out: cell starts of the left key-points (nullptr: not sorted)
    int32_t* plperm;         // [B][K] out: position -> left key-point
    int32_t* pperm;          // [B][K] out: scan position -> right key-point
    int32_t* pcell;          // [B][K] out: cell (y * 64 + x) of the right key-point at each scan position, -1: outside the grid
    // inputs of the scan formulation only (LEAN == false)
    int32_t* pxy_l;              // [B][K][2]
    unsigned long long* top2_p;  // [B][K]
    int32_t* govf_p;             // [B]
    int32_t* prange;             // [B][K][2]
    int32_t* pitems;             // [B][K]
    int32_t* prank;              // [B][K]
};

// The grid matcher's arguments in three parts (GridMatch); grid_kernels.hip hands its kernels ONE flat by-value copy of them.
// The problem: what both overloads of StVO::matchGrid take, batched, plus the scan order of the right features and the result.
struct GridProblem {
    int B, stride1, stride2;   // frame pairs; rows per frame of the left / right feature arrays
    int xy_width;              // 2 (points: cx, cy) or 4 (lines: sx, sy, ex, ey)
    int items_stride;          // CSR items per frame
    int words64, n1p;          // grid_matrix_dims(stride1, stride2), grid_scratch.h
    const int32_t* cell_xy1;   // [B][stride1][xy_width]
    const uint8_t* d1;         // [B][stride1][32]
    const int32_t* n1;         // [B]
    const int32_t* cell_start; // [B][3073]
    const int32_t* cell_items; // [B][items_stride]
    const uint8_t* d2;         // [B][stride2][32]
    const int32_t* n2;         // [B]
    const double* dir2;        // [B][stride2][2] (lines) or nullptr
    stvo_grid_window w;
    double ratio, line_sim_th;
    int mutual;
    const int32_t* rank;       // [B][stride2] right feature id -> scan position
    const int32_t* perm;       // [B][stride2] scan position -> right feature id
    int32_t* m12;              // [B][stride1] out
    bool lines() const { return xy_width == 4; }
};
// What the device-CSR point route of the pipeline adds (all null / 0 for lines and for the C-ABI points call).
// range1 != nullptr — the RANGE FORM (points, window of one grid row, right features numbered in CSR order): the candidates of a left
// feature are ONE contiguous range of scan positions, cell_start[row][x - w_lo] .. cell_start[row][x + w_hi + 1); the scan derives its
// masks from it and no candidate bit-matrix is built (GridScratch::cover may be nullptr); top2 / ovf must then be initialised by the
// caller (kTop2Empty = 0x00000000FFFFFFFF, 0).
struct PointRoute {
    const int32_t* range1;     // [B][stride1][2] (lo, hi) of every left feature
    const int32_t* cell2;      // [B][stride2] or nullptr: grid cell (y * 64 + x) of the right feature at each scan position, -1 outside the grid
    // left key-points counting-sorted by cell for the one-workgroup-per-frame point matcher (both or none), on a grid GRID_LW
    // columns wide (a left key-point up to w_lo columns right of the grid still has candidates)
    const uint32_t* lstart;    // [B][GRID_LSTART_STRIDE] exclusive cell starts, [GRID_LCELLS] = number of placed left key-points
    const int32_t* lperm;      // [B][stride1] position -> left feature
    // ---- what the step planner decides (step_plan.h), each only with grid_points_fused_ok
    // != 0: the caller left range1 / top2 / ovf uninitialised; the one-workgroup matcher derives them from cell_start / lstart / lperm
    // for the frames it hands to the scan formulation
    int lean_cells;
    // != 0: the one-workgroup matcher also runs the tail of the stereo association on the frame it just matched (filters,
    // back-projection, ordered compaction, point_tail.h) — no point_tail_kernel launch, no second pass over the matches
    int has_tail;
    // != 0 (and B <= the number of workgroups of the launch, i.e. one frame per workgroup): the one-workgroup matcher builds the grid
    // of its frame itself as its first phase — no point_cells_kernel launch
    int fused_cells;
    PointTail tail;
    PointCells cells;
};
struct GridMatch {
    GridProblem p;
    GridScratch s;  // grid_scratch.h
    PointRoute r;
};
// scan_events (optional): [0] / [1] are recorded on `s` before / after the two grid_scan passes
void launch_grid_batch(hipStream_t s, const GridMatch& g, hipEvent_t* scan_events = nullptr);
// true when launch_grid_batch will run the one-workgroup-per-frame point matcher for this batch
bool grid_points_fused_ok(const GridMatch& g);
// test hook, see stvo_seq_debug_grid: the masks the range form gives frame b, into g.s.cover = ONE frame's matrix
void launch_grid_range_debug(hipStream_t s, const GridMatch& g, int b);

// ---- the stereo association kernels of the device-resident pipeline (stereo_assoc_kernels.hip), one workgroup per frame of d.B ----
struct SeqDev;  // seq_state.h
void launch_point_cells(hipStream_t s, const SeqDev& d, bool lean);
void launch_point_tail(hipStream_t s, const SeqDev& d);
void launch_line_cells(hipStream_t s, const SeqDev& d);
void launch_line_tail(hipStream_t s, const SeqDev& d);
void launch_line_stereo_fused(hipStream_t s, const SeqDev& d, int lds_bytes, int Mk, int mutual, double ratio);
bool line_stereo_fused_lds_opt_in(int lds_bytes);  // lds_opt_in for line_stereo_fused_kernel<256>

// StereoFrameHandler::updateFrame's adaptive FAST rule for B streams, one lane per stream (fast_adapt_kernel.hip): th[b] moves by what
// results[b] says.  `results` may be device memory or the pinned block a zero-copy step writes its results to.
// ctl ([B] device, or nullptr = exactly the launch above all): the control words of the step the results come from (stvo_seq_control_next_step);
// the thresholds of the streams that did not RUN stay.
void launch_fast_adapt(hipStream_t s, int B, const stvo_pose_result* results, const stvo_fast_adapt& prm, int32_t* th, const int32_t* ctl = nullptr);

// Trajectory and key-frame decision for B streams, one lane per stream (traj_kernel.hip): state[b] advances by results[b] (T, cov, status),
// records (may be null) [B] takes what the update leaves for the caller.  `results` as for launch_fast_adapt.
void launch_traj_init(hipStream_t s, int B, stvo_traj_state* state);
// ctl ([B] device, or nullptr = the update for every stream, by the kernel that has always run it): the control words of the step the
// results come from.  RESTART: state[b] becomes what launch_traj_init writes, PARK: state[b] stays, bit for bit; the record of either is
// all-zero (frame == 0: no pose in this step).
void launch_traj_update(hipStream_t s, int B, const stvo_pose_result* results, const stvo_traj_params& prm, stvo_traj_state* state,
                        stvo_traj_record* records, const int32_t* ctl = nullptr);

// The per-stream control word of the device-resident pipeline (stream_control.hip).  ctl: [B] device, STVO_STREAM_*.
// pre: in front of the f2f stage — the streams that do not RUN present an empty previous stereo set (counts 0, their f2f match rows -1).
void launch_stream_ctl_pre(hipStream_t s, int B, const int32_t* ctl, int32_t* n_prev, int32_t* nl_prev, int32_t* m12p, int K, int32_t* m12l, int M);
// post: behind the pose kernel — their result record all-zero, their motion-model seed (motion_T, may be null) the identity, their
// inlier rows (inl_p / inl_l, may be null) -1.  results / inl_*: device memory or the pinned blocks the pose kernel wrote.
void launch_stream_ctl_post(hipStream_t s, int B, const int32_t* ctl, stvo_pose_result* results, double* motion_T, int32_t* inl_p, int K,
                            int32_t* inl_l, int M);
// th[b] = th0 for the RESTART streams
void launch_fast_restart(hipStream_t s, int B, const int32_t* ctl, int32_t* th, int th0);
// the camera a RESTART stream takes with its new sequence (stvo_seq_restart_cameras): calibration, grid scale 64 / cols, 48 / rows, image size
struct CamRestart {
    stvo_cam cam;
    double inv_w, inv_h;
    int32_t cols, rows;
};
void launch_cam_restart(hipStream_t s, int B, const int32_t* ctl, const CamRestart* upd, stvo_cam* cams, double* inv_wh, int32_t* snap_img /* [B][2] or nullptr */);

// Feature tracks and key-frame sets per stream (track_kernel.hip around track_update.h), one workgroup per stream, one launch per step.
// (StereoSetPtrs, the arrays of one stereo set of the pipeline: seq_layout.h)
struct TrackArgs {
    int B, K, M;         // K <= STVO_POSE_MAX_POINTS, M <= STVO_POSE_MAX_LINES: the winners of a stream fit the kernel's LDS
    int first;           // the pipeline's first step: every stream starts a sequence; nothing below up to `ctl` is read
    const int32_t *n_prev, *nl_prev;  // [B] counts of the previous stereo set, as the f2f stage saw them (0 for a stream under a control)
    const int32_t *m12p, *m12l;       // [B][K] / [B][M] f2f match of previous feature i1, or -1
    const int32_t *inlp, *inll;       // [B][K] / [B][M] the pose kernel's flag of previous feature i1 (device memory or the pinned block)
    const int32_t* ctl;               // [B] STVO_STREAM_* of this step, or nullptr = all RUN
    const stvo_traj_record* traj;     // [B] the trajectory records of this step (new_kf is read), or nullptr = no trajectory
    const int32_t *n_cur, *nl_cur;    // [B] counts of the current stereo set
    const stvo_track *prev_p, *prev_l;  // state the step propagates from ...
    stvo_track *next_p, *next_l;        // ... and leaves (another copy)
    stvo_track *rec_p, *rec_l;          // the step's ring row
    int32_t* rec_counts;                // [B][2] the counts that go with it
    // key-frame sets (kf_hdr == nullptr: off): at a key-frame the stream's rows [0, n) of `cur` are copied to `kf`
    StereoSetPtrs cur, kf;
    stvo_kf_header* kf_hdr;             // [B]
    int frame;                          // the pipeline step
};
void launch_track_update(hipStream_t s, const TrackArgs& a);

}  // namespace stvo
