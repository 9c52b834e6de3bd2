// step_plan.h — the schedule of one step of the device-resident pipeline (seq_pipeline.hip), decided on the host in ONE pure function.
// seq_enqueue_step gathers StepFacts, calls plan_step and then only enqueues what the StepPlan says; every rule of the schedule, with
// its measurement or its safety argument, is stated here and nowhere else.  Host only: no HIP include, no call into the runtime, no
// read of dbg() or of stvo_seq — tests/test_step_plan_host.py builds this header with g++ and checks the rules without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/stvo_hip.h"
#include "debug_switches.h"

namespace stvo {

// line_stereo_fused_kernel: the most key-lines per image it is built for, and the LDS it carves per line its launch is sized for
constexpr int LSF_MAX_LINES = 512, LSF_BYTES_PER_LINE = 32 + 16 + 16 + 4 + 2 * STVO_GRID_ROWS + 2 + 2 + 1;

// Every developer switch unset (DebugSwitches holds ints only): what a StepFacts starts from.
inline DebugSwitches switches_unset() {
    static_assert(sizeof(DebugSwitches) % sizeof(int) == 0, "DebugSwitches holds ints only");
    DebugSwitches d;
    int* v = reinterpret_cast<int*>(&d);
    for (size_t k = 0; k < sizeof(d) / sizeof(int); ++k) v[k] = DBG_UNSET;
    return d;
}

// Everything the decisions read, and nothing else.
struct StepFacts {
    int B = 0, K = 0, M = 0, cus = 0;  // streams, key-point / key-line capacity per image, CUs of the device
    bool has_points = false, has_lines = false, best_lr_matches = false;
    bool lines_now = false, lines_prev = false, track = false;  // StepFlags
    long long frame_idx = 0;
    bool raw_split = false;   // the slot's key-line arrays were copied on the line stream (stvo_seq::raw_split)
    int raw_max_lines = 0;    // most key-lines of one image in the slot, as far as the host knows
    int set_lines_cap_prev = 0;  // stvo_seq::set_lines_cap of the previous set ...
    int set_lines_cap_cur = 0;   // ... and what the set this step builds still holds from its last use (read only when the line stage is skipped)
    bool st_dirty = false, fetch = false, zero_copy = false;
    int timing = 0;              // stvo_seq_set_stage_timing: 0 off, 1 every stage, 2 light
    bool timing_events = false;  // ... and the step obtained its events
    bool has_alt_m12l = false;   // the second copy of the key-line match indices exists (batches)
    bool cells_differ = false;   // the two copies of the grid buffers differ (batches)
    // what the launch helpers answer (asked by the gather step as before, each only where it was asked before)
    bool grid_points_fused_ok = false, match_small_ok_K = false, match_small_ok_M = false, pose_inline_sync_ok = false,
         pose_batch_kernel_selected = false, pose_start_flag_ok = false;
    int pose2p_waves_per_pair = 0;
    // the step tracks AND carries a per-stream control (stvo_seq_control_next_step): a kernel at the very start of the step, on the point
    // stream, empties the previous stereo set of the streams that restart or are parked.  false (every other step): every plan as before.
    bool has_control = false;
    // streams were imported since the last step (stvo_seq_import_streams): the unpack kernel, on the point stream behind
    // optimizePose(k - 1), wrote rows and counts of the previous stereo set — key-line rows and counts included, which the line stream's f2f
    // match of this step reads.  The same hazard as a control's, so the same answer: the line stream does nothing in this step before it
    // has waited for the step's OWN fork event (no grid and no key-line stage ahead, no event-free fork).  Nothing else of the plan reads
    // it: the step's results depend on no stage-ahead work and on no StepHistory, and the step behind it may run ahead again.
    // false (every step of a pipeline that never imports): every plan as before.
    bool after_import = false;
    DebugSwitches sw = switches_unset();
};

// Which step last did what a later step's overlap leans on.  commit() moves them, only when the whole step has been enqueued, so
// that no later step waits on an event or a flag that a failed step never recorded.
struct StepHistory {
    long long fork_rec_frame = -2;   // the last step that recorded ev_fork on the point stream behind its grid
    long long pose_flag_frame = -2;  // the last step whose pose kernel publishes its start (d_pose_flag reaches pose_flag_value)
    long long sl_forked_frame = -2;  // the last step in which the line stream waited for an event of the point stream
};

// The four frame-to-frame match routes.
enum class MatchRoute : int32_t {
    SMALL = 0,     // match_small_kernel: one workgroup per frame pair
    BOTH_DIRS = 1, // both directions as full scans in one K1m launch + one ratio / mutual kernel
    LAZY = 2,      // forward scan + plan + selective reverse scans + final check
    ONE_WAY = 3,   // best_lr_matches off: forward scan + ratio test
};
struct MatchPlan {
    MatchRoute route = MatchRoute::ONE_WAY;
    int small_cap = 0;  // SMALL: rows per set the kernel sizes its LDS for (0: the stride)
    int nseg_cap = 0;   // BOTH_DIRS: most train segments (0: knn_pick_nseg's own)
};

struct StepPlan {
    bool light = false;          // light timing: event pairs around the three big kernels of the point stream only
    bool par = false;            // the line stage runs on the line stream
    bool mid_fork = false;       // ... which forks behind the cells kernel (ev_fork recorded there)
    bool fork_at_start = false;  // ... or at the start of the step: ev_fork recorded and awaited there
    bool line_forked = false;    // the line stream waits for an event of the point stream in this step
    bool zero_nl = false;        // no key-lines in this frame: the point tail zeroes the key-line counts of the set too
    bool point_stage = false, line_stage = false;  // the stereo association of the key-points / key-lines runs
    bool clear_nl = false;       // ... or the key-line counts of the set are cleared by a memset
    bool lean_cells = false, has_tail = false, fused_cells = false, cells_ahead = false, lines_ahead = false, gate = false;
    int Mk = 0;                  // key-lines per image the fused line kernel's LDS is sized for = set_lines_cap of the set built
    size_t line_lds = 0;
    bool line_fused = false;
    MatchPlan match_points, match_lines;
    bool track = false;          // frame-to-frame matching and optimizePose run (every step but the first)
    bool match_lines_run = false, clear_m12l = false;  // the line set is matched / has nothing to match against: indices cleared by a memset
    bool use_alt_m12l = false;
    bool inline_sync = false, fetch_by_pose = false, inl_zero_copy = false, lazy_eig = false, pose_flagged = false;
    bool join_signal = false;    // the line stream ends the step with a signal the pose kernel waits for (else, with `par`: ev_join)
    bool fetch_copy = false;     // the match indices leave for the host by a copy kernel + ev_fetch behind the join
    bool inl_copy = false;       // ... and the inlier masks by a copy kernel behind the pose kernel
    int32_t schedule[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // stvo_seq_last_schedule (include/stvo_hip.h: STVO_SCHED_*): bookkeeping only
};

// lds_fits(bytes): may line_stereo_fused_kernel<256> be launched with that much dynamic LDS?  Asked only above 48 KB and only when
// everything in front of it holds (the answer costs a runtime call the first time).
template <class LdsFits>
inline StepPlan plan_step(const StepFacts& f, const StepHistory& h, LdsFits&& lds_fits) {
    StepPlan p;
    const int B = f.B;
    const long long last = f.frame_idx - 1;
    const bool tev = f.timing != 0 && f.timing_events;
    // light timing (stvo_seq_set_stage_timing(.., 2)): event pairs around the grid matcher, the forward scan and the pose kernel only, on
    // the point stream; the key-line stream runs unmarked and the next frame's grid is still built ahead on it, so the three kernels
    // keep the neighbours they have in an untimed step (bench.py: `roofline` must come from the region that produced `value`)
    p.light = tev && f.timing == 2;
    // two copies of the key-line match indices, by the parity of the step (batches without the by-product fetch, whose copies read the
    // first): with the key-line stage ahead, the matches of step k + 1 may be written while optimizePose(k) reads those of step k
    const bool alt_ok = f.has_alt_m12l && !f.fetch;
    p.use_alt_m12l = alt_ok && (f.frame_idx & 1);
    // fork: everything enqueued so far (ingest, the previous step) happens-before the line stream's work
    p.par = f.lines_now && f.has_points;
    // Where the line stream forks off.  Every big kernel of the point stream fills the register file of the CUs it runs on, so work
    // of the line stream never runs BESIDE it, only instead of it.  Forked at the start of the step (small batches) the line kernels
    // share the GPU with point_cells_kernel and delay the start of some of the persistent point matcher's workgroups (0.158 -> 0.198 ms
    // per 1024 frames) but leave the key-point scan alone (0.467 ms); forked after the point stage (measured, then removed) they
    // stretched the scan instead (0.510 ms): 1024 KITTI-shaped streams 929 k (start) vs 935 k (after) frame pairs/s, 512 EuRoC-shaped
    // streams 857 k vs 777 k, one stream 0.252 vs 0.280 ms per frame.
    // Round 5: behind the cells kernel (mid), the default for batches: the line kernels then become ready together with the
    // persistent point matcher, whose workgroups (already queued) take their CUs first, instead of finding four line workgroups per CU
    // in their way.  1024 KITTI-shaped streams 0.872 -> 0.853 ms per step, 512 EuRoC-shaped 1.036 -> 1.105 M frame pairs/s; one
    // stream is SLOWER that way (0.205 -> 0.211 ms: its line kernels lose their head start), so small batches keep the fork at the start.
    p.mid_fork = p.par && B >= 64;
    // single-stream operation: the upload copied the key-line arrays ON the line stream and nothing the line stream would have to wait
    // for has been enqueued on the point stream since the last synchronisation — the step forks without an event
    // (a step with a control forks WITH an event: the line stream's f2f match reads the key-line count the control kernel cleared on the
    // point stream)
    const bool own_fork = f.has_control || f.after_import;  // the line stream starts behind this step's own fork event
    const bool fork_free = p.par && f.raw_split && !f.st_dirty && !own_fork;
    p.fork_at_start = p.par && !p.mid_fork && !fork_free;
    p.line_forked = p.par && (p.mid_fork || !fork_free);
    p.zero_nl = !f.lines_now && f.has_points;
    p.point_stage = f.has_points;
    p.line_stage = f.lines_now;  // a frame without key-lines skips the whole line stage (7 launches) and, below, the f2f line matching (6)
    p.clear_nl = !f.lines_now && !p.zero_nl;
    p.track = f.track;

    // ---- point stage
    if (f.has_points) {
        // the one-workgroup matcher: lean cells kernel in front, the tail of the association as its last phase
        p.lean_cells = f.grid_points_fused_ok;
        p.has_tail = p.lean_cells && f.sw.grid_tail != 0;  // (STVO_GRID_TAIL=0, developer: point_tail_kernel as its own launch)
        // one frame per workgroup of the matcher (single-stream operation, small batches): the grid of the frame is the matcher's
        // first phase — one dependent launch less in the chain of a frame
        p.fused_cells = p.lean_cells && B <= f.cus && f.sw.grid_cells != 0;
        // Batches: the grid of this frame on the LINE stream, which has been idle since ~0.2 ms into the previous step — the kernel (38 us
        // per 1024 frames; few instructions, mostly waiting) then runs beside the previous step's forward scan or pose kernel and
        // the point stream meets it with one awaited event in front of the matcher.  Safe because (a) its outputs are double-buffered
        // by the parity of the step (the matcher of the previous frame may still read the other copy; the copy written here was
        // last read two steps ago, and the line stream's work of the previous step waited for an event the point stream recorded
        // after that: sl_forked_frame), (b) the line stream has been made to wait for every upload enqueued on the point stream
        // (stvo_seq_step_dev), (c) everything else the kernel reads is the resident slot.  STVO_CELLS_AHEAD=0: in the point stream.
        // Never in a step with a control, and with it (below) never the key-line stage ahead: the key-line f2f match of such a step must see
        // the previous set's key-line counts as the control kernel left them, and that kernel runs on the point stream behind
        // optimizePose(k - 1), which still reads the set before.  So the line stream does nothing in such a step before it has waited for the
        // step's OWN fork event, recorded behind the control kernel.  The next step may run ahead again: the event it waits for is this
        // step's, and nothing its key-line kernels touch is written by the control kernels.
        p.cells_ahead = p.mid_fork && p.lean_cells && !p.fused_cells && (!tev || p.light) && f.cells_differ && h.sl_forked_frame == last &&
                        f.sw.cells_ahead != 0 && !own_fork;
        // key-line stage ahead (stvo_seq::m12l_alt has the whole argument): the line stream waits for the PREVIOUS step's fork event — in
        // front of the cells kernel, whose output copy the matcher of two steps ago read — and not for this step's.  Safe only while the
        // second copy of the key-line match indices is in use (alt_ok) and after a step that recorded the fork event (fork_rec_frame).
        // Only where it was measured to pay: ~100 key-lines per image (their kernels are a few per cent of the step) behind a pose kernel
        // that publishes its start, i.e. the two-waves-per-pair batch kernel.  With hundreds of key-lines per image the line kernels are
        // long enough to hold the pose kernel's freed slots against the next matcher: 512 EuRoC-shaped streams 0.442 -> 0.520 ms per step
        // (round 6), so those keep the fork of their own step.  STVO_LINES_AHEAD=1 forces it wherever it is safe.
        const bool flagged_last = h.pose_flag_frame == last;
        const bool la_pays = flagged_last && B > 2 * f.cus && std::max(f.raw_max_lines, f.set_lines_cap_prev) <= 128;
        p.lines_ahead = p.cells_ahead && alt_ok && h.fork_rec_frame == last && f.sw.lines_ahead != 0 && (f.sw.lines_ahead == 1 || la_pays);
        // ... and its kernels behind the dispatch of optimizePose(k - 1): the stream gate, where that kernel publishes its start
        p.gate = p.lines_ahead && flagged_last;
    }

    // ---- line stage
    if (f.lines_now) {
        // few key-lines per frame: the whole association in one workgroup per frame (STVO_LINE_FUSED=0: the general grid matcher)
        // LDS for the lines the slot holds, not for the capacity
        p.Mk = std::min(f.M, std::max(64, (f.raw_max_lines + 63) & ~63));
        p.line_lds = (size_t)p.Mk * LSF_BYTES_PER_LINE + 4 + (size_t)p.Mk * (p.Mk / 32) * 4;
        // (a single stream with hundreds of key-lines is better off with the general matcher's many small workgroups: EuRoC-shaped,
        // 300 key-lines, one stream 0.310 vs 0.360 ms per frame; 102 key-lines 0.257 vs 0.252)
        const int ef = f.sw.line_fused;
        p.line_fused = f.M <= LSF_MAX_LINES && (ef != DBG_UNSET ? ef != 0 : (B >= 16 || p.Mk <= 128)) &&
                       (p.line_lds <= (48u << 10) || lds_fits((int)p.line_lds));
    }

    // ---- frame-to-frame matching, join and pose
    if (f.track) {
        const int lines_cap = std::max(f.lines_now ? p.Mk : f.set_lines_cap_cur, f.set_lines_cap_prev);
        // one workgroup per frame pair (match_small_kernel) up to 128 key-lines per image; beyond that its row-by-row scan is the
        // longest thing on the key-line stream and the general machinery (K1m + planned reverse check, five launches) wins for every
        // batch size: 512 EuRoC-shaped streams with ~250 key-lines 844 k -> 913 k frame pairs/s (both directions in one K1m launch +
        // one ratio / mutual kernel: 895 k), one such stream 0.360 -> 0.310 ms (round 3).  STVO_MATCH_SMALL=0 (developer): the general
        // machinery for the key-line sets too.
        const int esm = f.sw.match_small;
        const bool small_sets = esm != DBG_UNSET ? esm != 0 : lines_cap <= 128;
        const bool elz = f.sw.match_lazy == 1;  // developer: the lazy formulation for small batches too
        auto route = [&](bool small_ok, bool timed, int small_cap) {
            MatchPlan m;
            if (small_ok && small_sets && !timed) {  // (timed: the stage timers want the general launches)
                m.route = MatchRoute::SMALL;
                m.small_cap = small_cap;
            } else if (f.best_lr_matches && B <= 4 && !timed && !elz) {
                // a few frame pairs leave most of the GPU idle: the reverse direction as a full scan in the SAME launch and one
                // ratio / mutual kernel, instead of the plan + two selective reverse scans + final check of the lazy formulation
                // (five dependent launches: 42 -> ~18 us of a single stream's 230 us)
                // (four train segments, not the 16 a single direction gets: both directions already double the workgroups, and the
                // ratio / mutual kernel merges 2 x nseg partial keys per row — one stream 0.2465 -> 0.2357 ms)
                m.route = MatchRoute::BOTH_DIRS;
                m.nseg_cap = 4;
            } else {
                m.route = f.best_lr_matches ? MatchRoute::LAZY : MatchRoute::ONE_WAY;
            }
            return m;
        };
        p.match_points = route(f.match_small_ok_K, tev, 0);
        p.match_lines = route(f.match_small_ok_M, false, lines_cap);
        p.match_lines_run = f.lines_prev && f.lines_now;
        p.clear_m12l = f.lines_prev && !f.lines_now;  // nothing to match against: every prev line is unmatched
        // Small batches (single-stream operation): the pose kernel itself waits for the line stream and hands the match indices to
        // the host — an event awaited or recorded in front of it delays its start by ~6 us each on this runtime.
        p.inline_sync = f.pose_inline_sync_ok && f.sw.seq_inline != 0 && !tev && (!f.fetch || (B == 1 && f.zero_copy));
        p.join_signal = p.par && p.inline_sync;
        p.fetch_by_pose = f.fetch && p.inline_sync;
        // small batches with the by-product fetch on (the StereoFrameHandler mirror): the pose kernel writes the inlier masks straight
        // into the pinned block — like its result — instead of a copy kernel behind it (one launch less on the single-stream chain)
        p.inl_zero_copy = f.fetch && f.zero_copy;
        p.inl_copy = f.fetch && !p.inl_zero_copy;
        // single-stream operation: the eigenvalues of the committed covariance (an output only) are computed by stvo_seq_read
        p.lazy_eig = p.inline_sync && f.zero_copy && f.sw.pose_kernel != 4;
        // batches on the batch kernel: the key-line stage of the next step may wait for this launch to begin
        p.pose_flagged = f.has_alt_m12l && f.pose_start_flag_ok;
        p.schedule[STVO_SCHED_POSE_KERNEL] = f.pose_batch_kernel_selected ? STVO_SCHED_POSE_BATCH : STVO_SCHED_POSE_LATENCY;
        p.schedule[STVO_SCHED_POSE_WAVES] = f.pose_batch_kernel_selected ? f.pose2p_waves_per_pair : 0;
    }
    p.fetch_copy = f.fetch && !p.fetch_by_pose;
    p.schedule[STVO_SCHED_FUSED_CELLS] = p.fused_cells;
    p.schedule[STVO_SCHED_CELLS_AHEAD] = p.cells_ahead;
    p.schedule[STVO_SCHED_LINES_AHEAD] = p.lines_ahead;
    p.schedule[STVO_SCHED_GATE] = p.gate;
    p.schedule[STVO_SCHED_MID_FORK] = p.mid_fork;
    p.schedule[STVO_SCHED_LINE_FUSED] = p.line_fused;
    return p;
}

// What an enqueued step has published for the steps after it.
inline void commit(StepHistory& h, const StepPlan& p, long long frame_idx) {
    if (p.mid_fork) h.fork_rec_frame = frame_idx;
    if (p.pose_flagged) h.pose_flag_frame = frame_idx;
    if (p.line_forked) h.sl_forked_frame = frame_idx;
}

}  // namespace stvo
