// seq_state.h — the state of the device-resident pipeline (stvo_seq), the argument block of its association kernels (SeqDev) and the
// layout of its one device allocation.  Shared by seq_pipeline.hip, seq_features.hip, seq_debug.hip and stereo_assoc_kernels.hip.
#pragma once
#include <vector>

#include "ctx_internal.h"
#include "seq_layout.h"
#include "step_plan.h"

namespace stvo {

constexpr int LENT = STVO_GRID_COLS + STVO_GRID_ROWS + 4;  // upper bound of Bresenham cells of one in-image line

struct SeqDev {
    int B, K, M;
    const stvo_cam* cams;   // [B] one calibration per sequence (config/dataset_params/kitti00-02 / 03 / 04-10.yaml differ)
    const double* inv_wh;   // [B][2] 64 / cols, 48 / rows of the sequence's images (stereoFrame.cpp:47-48)
    stvo_match_params mp;
    RawFrameView raw;  // raw features of the current frame (seq_layout.h)
    // grid scratch
    int32_t* pxy_l;    // [B][K][2]
    int32_t* pstart;   // [B][3073]
    int32_t* pitems;   // [B][K]
    int32_t* prank;    // [B][K]
    int32_t* pperm;    // [B][K]
    int32_t* lxy_l;    // [B][M][4]
    int32_t* lstart;   // [B][3073]
    int32_t* litems;   // [B][M*LENT]
    int32_t* lrank;    // [B][M]
    int32_t* lperm;    // [B][M]
    double* ldir;      // [B][M][2]
    const int32_t* m12s_p;  // [B][K] stereo matches of the left points
    const int32_t* m12s_l;  // [B][M]
    StereoSetPtrs cur;  // stereo set being built (curr)
    // optional mirrors of n / nl in pinned HOST memory (zero-copy read-back for small batches), or nullptr
    int32_t* host_n;
    int32_t* host_nl;
    int zero_nl;  // line stage skipped for this frame: the point tail clears nl[b] (saves a memset launch)
    // scratch of the point grid matcher that point_cells_kernel initialises (no candidate bit-matrix kernel runs for points)
    unsigned long long* top2_p;  // [B][K]
    int32_t* govf_p;             // [B]
    uint32_t* plstart;           // [B][GRID_LSTART_STRIDE] | left key-points counting-sorted by cell for the one-workgroup-per-frame
    int32_t* plperm;             // [B][K]                  | matcher (PointRoute); nullptr when capacity or window exceed what it handles
    int32_t* pcell;              // [B][K] grid cell (y * 64 + x) of the right key-point at each CSR position, -1: outside the grid
    int32_t* prange;             // [B][K][2] candidate range of every left key-point in CSR positions (GridStructure::get, one-row window)
};

// The arguments of the two key-point phases (point_cells.h, point_tail.h): for their kernels, and for the grid matcher where it runs them itself.
__host__ __device__ __forceinline__ PointCells point_cells_args(const SeqDev& s) {
    PointCells c;
    c.K = s.K; c.ws = s.mp.matching_s_ws;
    c.kp_l = s.raw.kp_l; c.kp_r = s.raw.kp_r; c.n_kp_l = s.raw.n_kp_l; c.n_kp_r = s.raw.n_kp_r; c.inv_wh = s.inv_wh;
    c.pstart = s.pstart; c.plstart = s.plstart; c.plperm = s.plperm; c.pperm = s.pperm; c.pcell = s.pcell;
    c.pxy_l = s.pxy_l; c.top2_p = s.top2_p; c.govf_p = s.govf_p; c.prange = s.prange; c.pitems = s.pitems; c.prank = s.prank;
    return c;
}
__host__ __device__ __forceinline__ PointTail point_tail_args(const SeqDev& s) {
    PointTail t;
    t.kp_l = s.raw.kp_l; t.kp_r = s.raw.kp_r; t.oct_l = s.raw.oct_l; t.desc_l = s.raw.desc_l; t.cams = s.cams;
    t.max_dist_epip = s.mp.max_dist_epip; t.min_disp = s.mp.min_disp;
    t.rc = s.cur.rc; t.desc = s.cur.desc; t.n = s.cur.n; t.host_n = s.host_n; t.nl = s.cur.nl; t.zero_nl = s.zero_nl;
    return t;
}

}  // namespace stvo

struct stvo_seq {
    stvo_ctx* ctx = nullptr;
    int B = 0, K = 0, M = 0, frame_idx = 0;
    stvo_match_params mp{};
    stvo_opt_params op{};
    double ratio_grid = 0;         // Config::minRatio12P() as the DOUBLE matchGrid compares with (matching.cpp:160,241)
    stvo_cam* d_cams = nullptr;    // [B] per-sequence calibration (device)
    double* d_inv_wh = nullptr;    // [B][2] per-sequence grid scale (device)
    double* d_qtab = nullptr;      // [STVO_POSE_QTAB] sqrt(sigma2) of pyramid level l (kernels.h: PosePoints::q_tab)
    double* d_motion_T = nullptr;  // [B][16] use_motion_model: the next step's initial DT per sequence, written by the pose kernel's commit (stvo_seq_set_motion_model)
    // trajectory and key-frame decision per stream (stvo_seq_set_trajectory): null = off
    stvo_traj_state* d_traj_state = nullptr;   // [B]
    stvo_traj_record* d_traj_ring = nullptr;   // [traj_log_steps][B]: tracked step k writes row k % traj_log_steps
    stvo_traj_params traj_prm{};
    int traj_log_steps = 0;
    unsigned long long traj_steps = 0;         // tracked steps enqueued so far
    // per-stream control of the NEXT step (stvo_seq_control_next_step; stream_control.hip): nothing of it exists until a control with a
    // word other than RUN is staged.  Two device copies: the one being staged for the next step, and the one the last step consumed, which
    // stvo_seq_adapt_fast_dev behind that step still reads while a caller may already stage the next.  Every reader and the copy that fills
    // them run on the context's stream.  Two pinned staging blocks used alternately, each with an event behind the copy that read it.
    int32_t* d_ctl[2] = {nullptr, nullptr};
    int32_t* ctl_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_ctl[2] = {nullptr, nullptr};
    bool ctl_stage_busy[2] = {false, false};
    int ctl_stage_next = 0, ctl_next = 0;   // the staging block / device copy the next stvo_seq_control_next_step fills
    bool ctl_staged = false;                // d_ctl[ctl_next] holds a control for the next step
    const int32_t* last_ctl = nullptr;      // the control the last enqueued step carried out (device), or nullptr
    // the cameras of restarting streams (stvo_seq_restart_cameras): nothing of it exists until the first call.  One device block [B] of its
    // own — the copy that fills it and the kernel that reads it run on the context's stream — and two pinned staging blocks used
    // alternately, each with an event behind the copy that read it
    stvo::CamRestart* d_cam_upd = nullptr;
    stvo::CamRestart* cam_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_cam[2] = {nullptr, nullptr};
    bool cam_stage_busy[2] = {false, false};
    int cam_stage_next = 0;
    bool cams_pending = false;              // cameras were written on the point stream since the last step: that step forks with its own event
    // feature tracks and key-frame sets per stream (stvo_seq_set_tracks; track_kernel.hip): null = off.  d_tracks is one allocation of
    // 2 + track_log_steps rows of [B][K] point records followed by [B][M] key-line records — rows 0 / 1 the state (step k reads copy
    // (k + 1) & 1 and writes copy k & 1), row 2 + k % track_log_steps the record of step k — and behind them the ring's counts
    // [track_log_steps][B][2].  d_kf is one allocation of B key-frame sets (the arrays of a stereo set without the counts) and their headers.
    char* d_tracks = nullptr;
    char* d_kf = nullptr;
    int track_log_steps = 0;
    unsigned long long track_steps = 0;     // steps enqueued with the tracks on
    stvo::StereoSetPtrs kf_set{};
    stvo_kf_header* d_kf_hdr = nullptr;
    size_t track_row_bytes() const { return (size_t)B * ((size_t)K + (size_t)M) * sizeof(stvo_track); }
    stvo_track* track_row_p(size_t row) const { return reinterpret_cast<stvo_track*>(d_tracks + row * track_row_bytes()); }
    stvo_track* track_row_l(size_t row) const { return track_row_p(row) + (size_t)B * K; }
    int32_t* track_counts(size_t ring_row) const {
        return reinterpret_cast<int32_t*>(d_tracks + (size_t)(2 + track_log_steps) * track_row_bytes()) + ring_row * (size_t)B * 2;
    }
    // export / import of single streams (stvo_seq_export_streams / stvo_seq_import_streams; seq_snapshot.hip).  The calibration and image
    // size of every stream as the pipeline was created with them; everything else exists from the first call on, each its own allocation:
    // the image sizes and the stream list of a call on the device (every reader and the copy that fills the list run on the context's
    // stream), two pinned staging blocks for the list used alternately, each with an event behind the copy that read it, and the device
    // buffer the host forms stage their blobs in.
    std::vector<stvo_cam> cams_host;
    std::vector<int32_t> img_size_host;     // [B][2] cols, rows
    int32_t* d_snap_img = nullptr;          // [B][2]
    int32_t* d_snap_streams = nullptr;      // [snap_streams_cap][2]
    int32_t* snap_stage[2] = {nullptr, nullptr};
    int snap_streams_cap = 0;
    hipEvent_t ev_snap[2] = {nullptr, nullptr};
    bool snap_stage_busy[2] = {false, false};
    int snap_stage_next = 0;
    char* snap_buf = nullptr;
    size_t snap_buf_bytes = 0;
    bool imported = false;                  // streams were imported since the last step (StepFacts::after_import)
    long long* d_prof = nullptr;   // STVO_POSE_PROF (developer aid): [B][16] phase ticks of the last pose launch, printed by stvo_seq_read
    char* dev = nullptr;     // one allocation, cut by stvo::seq_layout below
    size_t dev_bytes = 0;
    // pinned mirrors of the raw-feature block: two, used alternately — packing frame k + 1 on the host overlaps the device work
    // of frame k.  A block may be written again once the copy that last read it has completed.  The usual caller synchronises the
    // stream once per frame anyway (stvo_seq_read), so the uploads are numbered and the read remembers the last one it has
    // waited for: no event behind the copy (on this runtime a recorded event delays the next kernel of the stream by several
    // microseconds).  Only a caller that uploads a third frame without a read in between pays for an event, at that upload.
    char* raw_host[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    unsigned long long stage_upload[2] = {0, 0};  // number of the upload that last read the block (0: none)
    unsigned long long uploads = 0, uploads_done = 0;
    int stage_next = 0;
    // The key-line kernels of a step run on their own stream, which must see the frame's key-line arrays.  When the point stream
    // has been idle since the last read (single-stream operation: upload, step, read per frame) stvo_seq_upload copies the key-line
    // part of the block ON the line stream and the step forks without an event; st_dirty = something the line stream would have to
    // wait for has been enqueued on the point stream since the last synchronisation.
    bool st_dirty = false;
    // ordering inside the pose kernel instead of events (kernels.h: PoseSync::wait_flag / fetch_*), small batches only
    unsigned* d_join_flag = nullptr;     // device word the line stream's last launch of a step is followed by a signal on
    unsigned join_epoch = 0;
    unsigned fetch_epoch = 0;            // the last value handed to a pose kernel to publish in the pinned flag once the match indices are in fetch_host
    bool fetch_by_pose = false;          // the last step's by-products come that way (stvo_seq_fetch_matches polls the flag)
    unsigned fetch_value = 0;            // ... and the value its pose kernel publishes
    std::vector<char> raw_split;  // per slot: its key-line arrays were copied on the line stream
    stvo::RawFrameSpan raw_span{};  // bytes of a raw frame slot and where its key-line part begins (seq_layout.h)
    stvo::SeqDev d{};          // pointers into `dev` (set = current)
    // carve results
    // raw frame slots: 0 / 1 are carved from `dev` (push alternates between them); stvo_seq_set_slots adds more so that a
    // throughput caller can keep several frames of every sequence resident in HBM and rotate through them
    std::vector<char*> raw_dev;
    char* extra_raw = nullptr;
    stvo::StereoSetPtrs set[3];  // THREE stereo sets (round 6): step k writes set k mod 3 and reads set (k - 1) mod 3, so that the key-line stage of step
                                 // k + 1 (key-line stage ahead, below), which writes set (k + 1) mod 3, may run while the pose kernel of step k still reads sets k - 1 and k
    int cur = 0;
    int prev_set() const { return (cur + 2) % 3; }
    // scratch of the grid matchers (grid_scratch.h): key-points — no bit-matrix, the pipeline's point routes never read one — and key-lines
    stvo::GridScratch grid_p{}, grid_l{};
    int32_t* counts;
    stvo::FetchBlock fb{};  // the stereo and f2f match indices and the inlier masks, back to back (seq_layout.h)
    // ---- key-line stage AHEAD (the default for batches, round 6; STVO_LINES_AHEAD=0 switches it off): the key-line kernels of step k + 1
    // (stereo association + f2f of ~100 rows per image: 1024 small workgroups each) do not depend on anything the point stream does in
    // step k + 1, so the line stream no longer waits for that step's fork event.  It waits for the fork event of step k — recorded behind
    // optimizePose(k - 1), the last reader of the line set and of the key-line match indices step k + 1 overwrites (three sets; odd steps
    // write the second copy m12l_alt) — and passes a gate that opens when optimizePose(k) has been dispatched: the small workgroups then
    // fill the slots that kernel's one residency round frees as its frame pairs finish, instead of sharing the issue ports with the forward
    // scan K1m(k + 1), which they stretched by ~40 us per step.  The gate (launch_stream_gate) waits for PoseSync::start_flag (kernels.h
    // says why not "has been dispatched completely"): bounded, a hint — every data dependence is carried by the events.  The point stream
    // needs no second copy of its match indices: the point f2f of step k + 1 follows optimizePose(k) in stream order.
    int32_t* m12l_alt = nullptr;  // batches only
    unsigned* d_pose_flag = nullptr;
    unsigned pose_epoch = 0;         // the last start value handed to a pose kernel
    stvo::StepHistory hist;          // which step last recorded ev_fork / published its pose kernel's start / forked the line stream (step_plan.h)
    unsigned pose_flag_value = 0;    // what d_pose_flag reaches when the pose kernel of step hist.pose_flag_frame starts
    stvo_pose_result* results;
    char* out_host = nullptr;  // pinned: results + counts
    // second stream: the line stage (stereo association + f2f of the key-lines) is independent of the point stage
    // until optimizePose (the reference runs the two in parallel threads, stereoFrame.cpp:67-72, stereoFrameHandler.cpp:
    // 115-118) and its kernels are far too small to fill the GPU, so it runs concurrently on its own scratch
    hipStream_t line_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Batches: the grid of frame k + 1 (point_cells_kernel) is enqueued on the LINE stream, which is idle from ~0.2 ms into step k on, and
    // the point stream only waits for it in front of its matcher — 38 us less in the chain of a step (step_plan.h: cells_ahead).  The kernel's
    // outputs are double-buffered by the parity of the step (cells_buf[cur]): the grid of frame k + 1 may be built while the matcher
    // of frame k still reads its own.
    hipEvent_t ev_cells = nullptr, ev_upload = nullptr;
    unsigned long long upload_seq = 0, upload_seen = 0;  // uploads enqueued on the point stream / the last one the line stream has been made to wait for
    struct CellsBuf {
        int32_t *pstart, *pperm, *pcell, *plperm;
        uint32_t* plstart;
    } cells_buf[2] = {};
    // the matcher's scratch for the key-lines, as the layout below cuts it (the context owns the key-points').  `need` holds the column
    // claims — MatchScratch::claim; the buffer keeps the name the pipeline's buffer list knows it by (tests/cpp/seq_layout_host.cpp)
    struct KeylineMatchBufs {
        uint2 *knn12, *knn21;
        int32_t* cand;
        uint32_t* need;
        int32_t *qsel, *nsel;
        size_t knn_capacity;
        stvo::MatchScratch match_scratch() const { return stvo::MatchScratch{knn12, knn21, cand, need, qsel, nsel, knn_capacity}; }
    } lazy_l{};
    // optional by-products for callers that mirror the reference's host-side feature lists (StereoFrameHandler):
    // the four match-index arrays are copied to pinned memory right after the f2f stage (ev_fetch), i.e. while the
    // pose kernel still runs; the inlier masks follow the pose kernel.  fetch_host mirrors `fb`, offset for offset.
    bool fetch = false;
    char* fetch_host = nullptr;
    hipEvent_t ev_fetch = nullptr;
    // optional live stage timing (bench.py): event pairs around the kernels of every step, on the stream they run on
    int timing = 0;  // 1: every stage; 2: "light" — only the three big kernels of the point stream, the step otherwise as untimed
    std::vector<hipEvent_t> tev;  // STVO_SEQ_NSTAGE start/stop pairs per step, grown on demand
    size_t tev_used = 0;
    bool zero_copy = false;    // small batches: kernels write results / counts straight into out_host
    std::vector<char> raw_lines;  // slot holds at least one left and one right key-line
    std::vector<int> raw_max_lines;  // most key-lines of one image in the slot, as far as the host knows (device ingests: M)
    int set_lines_cap[3] = {0, 0, 0};   // the same bound for the stereo line sets
    bool set_lines[3] = {false, false, false};  // stereo set was built from a frame with key-lines
    bool last_lines = false;             // the last step ran the line stage
    int last_slot = 0;                   // raw slot of the last step
    // what the test hooks need of the last step's routes; they rebuild the matchers' arguments (point_grid_args / line_grid_args)
    bool last_point_lean = false;        // its point stage ran the lean cells phase and the one-workgroup matcher (StepPlan::lean_cells)
    bool last_mutual = false;            // its matchers ran with best_lr_matches (ovf is written)
    bool last_line_fused = false;        // it ran line_stereo_fused_kernel: the hook rebuilds the grid arrays
    int32_t last_schedule[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // what the last enqueued step decided (stvo_seq_last_schedule)
    // inside the pinned mirror of `fb`: the array at byte offset `off` (FetchBlock::off_*), the flag word behind the block
    int32_t* fetch_mirror(size_t off) const { return reinterpret_cast<int32_t*>(fetch_host + off); }
    unsigned* fetch_flag() const { return reinterpret_cast<unsigned*>(fetch_host + fb.off_flag); }
    stvo::RawFrameView raw_view(int slot) const { return stvo::raw_frame<true>(raw_dev[slot], B, K, M); }  // what the kernels of a step read (SeqDev::raw)
    // where a step's pose kernel writes its results (PoseProblem::results) and the readers behind it find them
    stvo_pose_result* step_results() const { return zero_copy ? reinterpret_cast<stvo_pose_result*>(out_host) : results; }
};

namespace stvo {

// Every buffer of stvo_seq::dev, in the order it is cut: each is named here once, where its pointer is stored.  stvo_seq_create_multi runs
// this on a null base for the size (what it stores then are bare offsets, overwritten by the second run) and on the allocation.
// Reads s.B, s.K, s.M, s.mp and s.raw_span.
inline size_t seq_layout(stvo_seq& s, char* base) {
    const int B = s.B, K = s.K, M = s.M, R = K > M ? K : M, ws = s.mp.matching_s_ws;
    const size_t nb = (size_t)B, nK = nb * K, nM = nb * M, n_cells = nb * (STVO_GRID_CELLS + 1), n_lstart = nb * GRID_LSTART_STRIDE;
    SeqDev& d = s.d;
    Carver c(base);
    auto i32 = [&c](size_t count) { return c.take<int32_t>(count); };
    // the two raw frame slots of stvo_seq_push (mirrored in pinned host memory, one H2D per frame)
    s.raw_dev = {c.take<char>(s.raw_span.bytes), c.take<char>(s.raw_span.bytes)};  // (a braced list is evaluated left to right)
    d.cams = s.d_cams = c.take<stvo_cam>(nb); d.inv_wh = s.d_inv_wh = c.take<double>(nb * 2); s.d_qtab = c.take<double>(STVO_POSE_QTAB);
    s.d_join_flag = c.take<unsigned>(16); s.d_pose_flag = c.take<unsigned>(16);
    // grids of the stereo association: key-points
    d.pxy_l = i32(nK * 2); d.pstart = i32(n_cells); d.pitems = i32(nK); d.prank = i32(nK); d.pperm = i32(nK); d.prange = i32(nK * 2); d.pcell = i32(nK);
    const bool lsort = K <= 2048 && ws >= 0 && ws <= GRID_LW - STVO_GRID_COLS;
    d.plstart = lsort ? c.take<uint32_t>(n_lstart) : nullptr; d.plperm = lsort ? i32(nK) : nullptr;
    // second copy of what the lean point_cells_kernel writes (batches only: stvo_seq::cells_buf)
    const bool cells2 = lsort && B >= 64;
    stvo_seq::CellsBuf& cb = s.cells_buf[1];
    cb = s.cells_buf[0] = {d.pstart, d.pperm, d.pcell, d.plperm, d.plstart};
    if (cells2) {
        cb.pstart = i32(n_cells); cb.pperm = i32(nK); cb.pcell = i32(nK); cb.plstart = c.take<uint32_t>(n_lstart); cb.plperm = i32(nK);
    }
    // ... key-lines
    d.lxy_l = i32(nM * 4); d.lstart = i32(n_cells); d.litems = i32(nM * LENT); d.lrank = i32(nM); d.lperm = i32(nM); d.ldir = c.take<double>(nM * 2);
    // scratch of the grid matchers (grid_scratch.h).  Key-points: no bit-matrix, misfit behind ovf; top2 / owner2 keep the R rows they
    // have always had.  Key-lines: the eligible-pair half here, the half with the bit-matrix behind the fetch block.
    carve_grid_scratch(c, s.grid_p, B, R, R, false, true, GRID_SCRATCH_ROWS);
    carve_grid_scratch(c, s.grid_p, B, K, K, false, true, GRID_SCRATCH_ELIG);
    d.top2_p = s.grid_p.top2; d.govf_p = s.grid_p.ovf;
    carve_grid_scratch(c, s.grid_l, B, M, M, true, false, GRID_SCRATCH_ELIG);
    s.fb = carve_fetch_block(c, B, K, M);
    d.m12s_p = s.fb.m12s_p; d.m12s_l = s.fb.m12s_l;
    s.results = c.take<stvo_pose_result>(nb); s.counts = i32(nb * 4);
    const bool alt_l = B >= 64;  // second copy of the key-line match indices (key-line stage ahead: batches only)
    s.m12l_alt = alt_l ? i32(nM) : nullptr;
    carve_grid_scratch(c, s.grid_l, B, M, M, true, false, GRID_SCRATCH_ROWS);
    stvo_seq::KeylineMatchBufs& w = s.lazy_l;
    w.knn_capacity = nM * 4;  // line f2f: up to 4 train segments; stvo_seq_create_multi holds it against match_scratch_fits
    w.knn12 = c.take<uint2>(w.knn_capacity); w.knn21 = c.take<uint2>(w.knn_capacity);
    w.cand = i32(nM); w.need = c.take<uint32_t>(nM); w.qsel = i32(nM); w.nsel = i32(nb * 5);
    for (StereoSetPtrs& q : s.set) q = carve_stereo_set(c, B, K, M, true);
    return c.off;
}

// Rows [0, n) / [0, nl) of sequence b of a stereo set to the host (synchronous copies; the caller has synchronised the streams that
// write the set).  `dst` holds the host arrays, its counts are not used.
inline int copy_out_stereo_set(stvo_ctx* ctx, const StereoSetPtrs& q, int b, size_t K, size_t M, int n, int nl, const StereoSetPtrs& dst) {
    const size_t p = b * K, l = b * M, D = sizeof(double);
    const struct { void* to; const void* from; size_t row_bytes; int rows; } cols[] = {
        {dst.rc, q.rc + p, sizeof(float4), n}, {dst.desc, q.desc + p * STVO_DESC_BYTES, STVO_DESC_BYTES, n},
        {dst.spl, q.spl + l * 2, 2 * D, nl}, {dst.epl, q.epl + l * 2, 2 * D, nl}, {dst.sP, q.sP + l * 3, 3 * D, nl}, {dst.eP, q.eP + l * 3, 3 * D, nl},
        {dst.le, q.le + l * 3, 3 * D, nl}, {dst.s2l, q.s2l + l, D, nl}, {dst.s2lm, q.s2lm + l, D, nl}, {dst.ldesc, q.ldesc + l * STVO_DESC_BYTES, STVO_DESC_BYTES, nl}};
    for (const auto& c : cols)
        if (c.rows) HIP_TRY(ctx, hipMemcpy(c.to, c.from, (size_t)c.rows * c.row_bytes, hipMemcpyDeviceToHost));
    return STVO_OK;
}

// What stvo_seq_step_dev (seq_pipeline.hip) decides before it plans, and hands to the feature tracks behind the step (seq_features.hip).
struct StepFlags {
    bool lines_now, lines_prev, track;
    const int32_t* ctl;  // [B] device: the control words this step carries out (only a step that tracks does), or nullptr
};
int enqueue_track_update(stvo_seq* s, const StepPlan& plan, const StepFlags& fl);

// The arguments of the two stereo grid matchers for the arrays in `d` (seq_pipeline.hip): the step's, and what the test hooks rebuild.
// The point matcher's up to what the plan decides (PointRoute::lean_cells, has_tail, fused_cells).
GridMatch point_grid_args(const stvo_seq* s, const SeqDev& d);
GridMatch line_grid_args(const stvo_seq* s, const SeqDev& d);

}  // namespace stvo
