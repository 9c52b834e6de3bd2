// seq_features.hip — the optional per-stream features of the device-resident pipeline (seq_pipeline.hip; state: seq_state.h): trajectory and
// key-frame decision, feature tracks and key-frame sets, per-stream control of the next step, the adaptive FAST threshold and its restart.
#include "seq_state.h"

namespace stvo {

// The feature tracks of the step stvo_seq_step_dev has just committed (cur, frame_idx, traj_steps have moved on): the last launch of the
// step on the context's stream, behind the pose kernel, stream_ctl_post_kernel and the trajectory update.  It reads the counts of the
// previous set, every array of the set the step built, the copy of the key-line match indices the step used, the inlier rows where
// the pose kernel wrote them and the step's trajectory records.  DESIGN.md (feature tracks) has the argument why the key-line stage
// ahead, which recycles the set and the match copy, cannot overtake it.
int enqueue_track_update(stvo_seq* s, const stvo::StepPlan& plan, const StepFlags& fl) {
    stvo_ctx* ctx = s->ctx;
    const StereoSetPtrs& cs = s->set[s->prev_set()];
    const StereoSetPtrs& ps = s->set[(s->cur + 1) % 3];
    stvo::TrackArgs a{};
    std::memset(&a, 0, sizeof(a));
    a.B = s->B; a.K = s->K; a.M = s->M;
    a.first = fl.track ? 0 : 1;
    a.frame = s->frame_idx - 1;
    if (fl.track) {
        a.n_prev = ps.n; a.nl_prev = ps.nl;
        a.m12p = s->fb.m12p; a.m12l = plan.use_alt_m12l ? s->m12l_alt : s->fb.m12l;
        // (StepEnq::pose: under inl_zero_copy the pose kernel wrote the masks straight into the pinned block)
        a.inlp = plan.inl_zero_copy ? s->fetch_mirror(s->fb.off_inlp) : s->fb.inlp;
        a.inll = plan.inl_zero_copy ? s->fetch_mirror(s->fb.off_inll) : s->fb.inll;
        a.ctl = fl.ctl;
        if (s->d_traj_state) a.traj = s->d_traj_ring + (size_t)((s->traj_steps - 1) % (unsigned long long)s->traj_log_steps) * s->B;
    }
    a.n_cur = cs.n; a.nl_cur = cs.nl;
    const size_t k = (size_t)(s->track_steps & 1ull), ring = (size_t)(s->track_steps % (unsigned long long)s->track_log_steps);
    a.prev_p = s->track_row_p(k ^ 1); a.prev_l = s->track_row_l(k ^ 1);
    a.next_p = s->track_row_p(k); a.next_l = s->track_row_l(k);
    a.rec_p = s->track_row_p(2 + ring); a.rec_l = s->track_row_l(2 + ring);
    a.rec_counts = s->track_counts(ring);
    a.cur = cs;
    a.kf = s->kf_set;
    a.kf_hdr = s->d_kf_hdr;
    stvo::launch_track_update(ctx->stream, a);
    s->track_steps++;
    return check_launch(ctx);
}

}  // namespace stvo

extern "C" {

// Trajectory per stream inside the pipeline (stvo_hip.h).  The state and the ring are new device memory: filled on the context's own stream.
int stvo_seq_set_trajectory(stvo_seq* s, const stvo_traj_params* prm, int log_steps) {
    if (!s || s->frame_idx != 0) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    if (!prm) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (s->d_traj_state) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (its fill may still run)
            (void)hipFree(s->d_traj_state);
            (void)hipFree(s->d_traj_ring);
        }
        s->d_traj_state = nullptr; s->d_traj_ring = nullptr; s->traj_log_steps = 0;
        return STVO_OK;
    }
    if (log_steps < 1) return STVO_ERR_INVALID_ARG;
    const unsigned long long ring_bytes = (unsigned long long)log_steps * (unsigned long long)s->B * sizeof(stvo_traj_record);
    if (ring_bytes > (1ull << 30)) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->d_traj_state) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(s->d_traj_state);
        (void)hipFree(s->d_traj_ring);
        s->d_traj_state = nullptr; s->d_traj_ring = nullptr; s->traj_log_steps = 0;
    }
    stvo_traj_state* st = nullptr;
    stvo_traj_record* ring = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&st, (size_t)s->B * sizeof(stvo_traj_state)));
    if (hipMalloc((void**)&ring, (size_t)ring_bytes) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(st);
        std::snprintf(ctx->last_error, sizeof(ctx->last_error), "%s", "hipMalloc of the trajectory ring failed");
        return STVO_ERR_HIP;
    }
    stvo::launch_traj_init(ctx->stream, s->B, st);
    if (hipMemsetAsync(ring, 0, (size_t)ring_bytes, ctx->stream) != hipSuccess || check_launch(ctx) != STVO_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(st);
        (void)hipFree(ring);
        return STVO_ERR_HIP;
    }
    s->d_traj_state = st; s->d_traj_ring = ring; s->traj_prm = *prm; s->traj_log_steps = log_steps; s->traj_steps = 0;
    return STVO_OK;
}

int stvo_seq_read_trajectory(stvo_seq* s, int n_last, stvo_traj_record* records, int32_t* n_got) {
    if (!s || !s->d_traj_state || n_last < 1 || !records || !n_got) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long n = (unsigned long long)n_last;
    if (n > (unsigned long long)s->traj_log_steps) n = (unsigned long long)s->traj_log_steps;
    if (n > s->traj_steps) n = s->traj_steps;
    const size_t row = (size_t)s->B * sizeof(stvo_traj_record);
    for (unsigned long long i = 0; i < n; ++i) {  // oldest first
        const size_t r = (size_t)((s->traj_steps - n + i) % (unsigned long long)s->traj_log_steps);
        HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char*>(records) + i * row, reinterpret_cast<const char*>(s->d_traj_ring) + r * row, row,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_got = (int32_t)n;
    return STVO_OK;
}

// Feature tracks and key-frame sets per stream inside the pipeline (stvo_hip.h).  New device memory, zeroed on the context's own stream.
int stvo_seq_set_tracks(stvo_seq* s, int keyframe_sets, int log_steps) {
    if (!s || s->frame_idx != 0 || log_steps < 0 || (keyframe_sets != 0 && keyframe_sets != 1)) return STVO_ERR_INVALID_ARG;
    if (log_steps == 0 && keyframe_sets) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->d_tracks || s->d_kf) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the fill may still run)
        if (s->d_tracks) (void)hipFree(s->d_tracks);
        if (s->d_kf) (void)hipFree(s->d_kf);
    }
    s->d_tracks = nullptr; s->d_kf = nullptr; s->d_kf_hdr = nullptr; s->track_log_steps = 0; s->track_steps = 0;
    s->kf_set = stvo::StereoSetPtrs{};
    if (log_steps == 0) return STVO_OK;
    if ((unsigned long long)log_steps * s->track_row_bytes() > (1ull << 34)) return STVO_ERR_INVALID_ARG;
    const size_t nb = (size_t)s->B;
    const size_t track_bytes = (size_t)(2 + log_steps) * s->track_row_bytes() + (size_t)log_steps * nb * 2 * sizeof(int32_t);
    // d_kf: the arrays of a stereo set without the counts, then the headers (run on a null base for the size, then on the allocation)
    stvo::StereoSetPtrs kf_set{};
    stvo_kf_header* kf_hdr = nullptr;
    auto kf_layout = [&](char* base) {
        stvo::Carver c(base);
        kf_set = stvo::carve_stereo_set(c, s->B, s->K, s->M, false);
        kf_hdr = c.take<stvo_kf_header>(nb);
        return c.off;
    };
    const size_t kf_bytes = kf_layout(nullptr);
    char *tr = nullptr, *kf = nullptr;
    bool ok = hipMalloc((void**)&tr, track_bytes) == hipSuccess;
    if (ok && keyframe_sets) ok = hipMalloc((void**)&kf, kf_bytes) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (tr) (void)hipFree(tr);
        std::snprintf(ctx->last_error, sizeof(ctx->last_error), "%s", "hipMalloc of the feature tracks or the key-frame sets failed");
        return STVO_ERR_HIP;
    }
    if (hipMemsetAsync(tr, 0, track_bytes, ctx->stream) != hipSuccess || (kf && hipMemsetAsync(kf, 0, kf_bytes, ctx->stream) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(tr);
        if (kf) (void)hipFree(kf);
        return STVO_ERR_HIP;
    }
    s->d_tracks = tr; s->track_log_steps = log_steps;
    if (kf) {
        s->d_kf = kf;
        kf_layout(kf);
        s->kf_set = kf_set;
        s->d_kf_hdr = kf_hdr;
    }
    return STVO_OK;
}

int stvo_seq_read_tracks(stvo_seq* s, int n_last, stvo_track* pts, stvo_track* lines, int32_t* counts, int32_t* n_got) {
    if (!s || !s->d_tracks || n_last < 1 || !n_got) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long n = (unsigned long long)n_last;
    if (n > (unsigned long long)s->track_log_steps) n = (unsigned long long)s->track_log_steps;
    if (n > s->track_steps) n = s->track_steps;
    const size_t bp = (size_t)s->B * s->K * sizeof(stvo_track), bl = (size_t)s->B * s->M * sizeof(stvo_track), bc = (size_t)s->B * 2 * sizeof(int32_t);
    for (unsigned long long i = 0; i < n; ++i) {  // oldest first
        const size_t r = (size_t)((s->track_steps - n + i) % (unsigned long long)s->track_log_steps);
        if (pts) HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char*>(pts) + i * bp, s->track_row_p(2 + r), bp, hipMemcpyDeviceToHost, ctx->stream));
        if (lines) HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char*>(lines) + i * bl, s->track_row_l(2 + r), bl, hipMemcpyDeviceToHost, ctx->stream));
        if (counts) HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char*>(counts) + i * bc, s->track_counts(r), bc, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_got = (int32_t)n;
    return STVO_OK;
}

int stvo_seq_tracks_dev(stvo_seq* s, const stvo_track** pts_dev, const stvo_track** lines_dev, const int32_t** counts_dev) {
    if (!s || !s->d_tracks || s->track_steps == 0) return STVO_ERR_INVALID_ARG;
    const size_t r = (size_t)((s->track_steps - 1) % (unsigned long long)s->track_log_steps);
    if (pts_dev) *pts_dev = s->track_row_p(2 + r);
    if (lines_dev) *lines_dev = s->track_row_l(2 + r);
    if (counts_dev) *counts_dev = s->track_counts(r);
    return STVO_OK;
}

int stvo_seq_keyframe_headers(stvo_seq* s, stvo_kf_header* hdr) {
    if (!s || !s->d_kf_hdr || !hdr) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(hdr, s->d_kf_hdr, (size_t)s->B * sizeof(stvo_kf_header), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_seq_read_keyframe(stvo_seq* s, int b, stvo_kf_header* hdr, int32_t cap_pts, float* rc, uint8_t* desc, int32_t cap_lines, double* spl,
                           double* epl, double* sP, double* eP, double* le, double* s2l, double* s2lm, uint8_t* ldesc) {
    if (!s || !s->d_kf_hdr || b < 0 || b >= s->B || !hdr || cap_pts < 0 || cap_lines < 0) return STVO_ERR_INVALID_ARG;
    if ((cap_pts > 0 && (!rc || !desc)) || (cap_lines > 0 && (!spl || !epl || !sP || !eP || !le || !s2l || !s2lm || !ldesc)))
        return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    stvo_kf_header h{};
    HIP_TRY(ctx, hipMemcpy(&h, s->d_kf_hdr + b, sizeof(h), hipMemcpyDeviceToHost));
    const size_t K = (size_t)s->K, M = (size_t)s->M;
    if (h.n_pts < 0 || (size_t)h.n_pts > K || h.n_lines < 0 || (size_t)h.n_lines > M) return STVO_ERR_HIP;
    *hdr = h;
    if (h.n_pts > cap_pts || h.n_lines > cap_lines) return STVO_ERR_CAPACITY;
    return stvo::copy_out_stereo_set(ctx, s->kf_set, b, K, M, h.n_pts, h.n_lines,
                                     stvo::StereoSetPtrs{reinterpret_cast<float4*>(rc), desc, nullptr, spl, epl, sP, eP, le, s2l, s2lm, ldesc, nullptr});
}

int stvo_seq_read_trajectory_state(stvo_seq* s, stvo_traj_state* state) {
    if (!s || !s->d_traj_state || !state) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(state, s->d_traj_state, (size_t)s->B * sizeof(stvo_traj_state), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return STVO_OK;
}

int stvo_seq_trajectory_state_dev(stvo_seq* s, stvo_traj_state** state_dev) {
    if (!s || !s->d_traj_state || !state_dev) return STVO_ERR_INVALID_ARG;
    *state_dev = s->d_traj_state;
    return STVO_OK;
}

// updateFrame's adaptive FAST rule (:66-86) behind the last enqueued step, on the stream its pose kernel ran on.  That step tracked iff it
// was not the first of the sequence (StepFlags::track = frame_idx > 0, and frame_idx has moved on since): initialize() has no updateFrame().
int stvo_seq_adapt_fast_dev(stvo_seq* s, const stvo_fast_adapt* prm, int32_t* th_dev) {
    if (!s || !prm || !th_dev || prm->min_th > prm->max_th || s->frame_idx < 1) return STVO_ERR_INVALID_ARG;
    if (s->frame_idx == 1) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::launch_fast_adapt(ctx->stream, s->B, s->step_results(), *prm, th_dev, s->last_ctl);
    return check_launch(ctx);
}

// Per-stream control of the next step (stvo_hip.h).  Validated before anything changes; the words reach the device now, in stream order.
int stvo_seq_control_next_step(stvo_seq* s, const int32_t* ctl_host) {
    if (!s || !ctl_host) return STVO_ERR_INVALID_ARG;
    bool any = false;
    for (int b = 0; b < s->B; ++b) {
        if (ctl_host[b] < STVO_STREAM_RUN || ctl_host[b] > STVO_STREAM_PARK) return STVO_ERR_INVALID_ARG;
        any = any || ctl_host[b] != STVO_STREAM_RUN;
    }
    if (!any) {  // all-RUN: nothing to stage, and nothing staged stays
        s->ctl_staged = false;
        return STVO_OK;
    }
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)s->B * sizeof(int32_t), span = (bytes + 255) & ~size_t(255);
    if (!s->d_ctl[0]) {  // first use
        HIP_TRY(ctx, hipMalloc((void**)&s->d_ctl[0], 2 * span));
        s->d_ctl[1] = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(s->d_ctl[0]) + span);
    }
    if (!s->ctl_stage[0]) {
        HIP_TRY(ctx, hipHostMalloc((void**)&s->ctl_stage[0], 2 * span, hipHostMallocDefault));
        s->ctl_stage[1] = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(s->ctl_stage[0]) + span);
    }
    for (auto& e : s->ev_ctl)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int hb = s->ctl_stage_next;
    if (s->ctl_stage_busy[hb]) {  // the copy that last read this block (two calls ago): done long since, unless nothing has synchronised
        HIP_TRY(ctx, hipEventSynchronize(s->ev_ctl[hb]));
        s->ctl_stage_busy[hb] = false;
    }
    std::memcpy(s->ctl_stage[hb], ctl_host, bytes);
    HIP_TRY(ctx, hipMemcpyAsync(s->d_ctl[s->ctl_next], s->ctl_stage[hb], bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(s->ev_ctl[hb], ctx->stream));
    s->ctl_stage_busy[hb] = true;
    s->ctl_stage_next = hb ^ 1;
    s->ctl_staged = true;
    return STVO_OK;
}

// initialize()'s orb_fast_th (:38) for the streams the staged control restarts, in front of the detection of their first frame.
int stvo_seq_restart_fast_dev(stvo_seq* s, int32_t* th_dev, int th0) {
    if (!s || !th_dev || th0 < 1 || th0 > 254) return STVO_ERR_INVALID_ARG;
    if (!s->ctl_staged) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::launch_fast_restart(ctx->stream, s->B, s->d_ctl[s->ctl_next], th_dev, th0);
    return check_launch(ctx);
}

// The camera of the sequence a RESTART stream begins (stvo_hip.h): for every stream the STAGED control marks RESTART, d_cams[b], d_inv_wh[b]
// and what a snapshot header says of the stream become the given values, by one small kernel enqueued NOW on the context's stream (the
// point stream), behind the copy of the control words it reads and in front of the step they belong to.
// Why no reader sees a half-old camera.  The readers are the cells kernels (inv_wh), the stereo tails of key-points and key-lines (cams),
// the pose kernel (cams) and the snapshot export (cams, image size).
//   * Of step k - 1 and earlier: everything on the point stream — its pose kernel last — was enqueued there earlier, so it precedes this
//     kernel in stream order; the key-line stream's work of step k - 1 was joined in FRONT of that pose kernel (the join event, or the flag
//     the pose kernel waits for), so it has completed as well.  An export enqueued earlier runs on the context's stream too.
//   * Of step k: a step with a control runs nothing ahead of its own fork event (step_plan.h: never the cells kernel or the key-line stage
//     ahead, never the event-free fork), and that event is recorded on the point stream behind the control kernel of the step, which is
//     enqueued behind this one.  So every kernel of step k on either stream follows this kernel.
//   * A step that follows this call WITHOUT carrying the control — the pipeline's own first step (a control staged for it is consumed
//     without effect, but the cameras given here are taken), or a step before which an all-RUN stvo_seq_control_next_step withdrew the
//     control after the cameras were written — would be free to fork without an event or to run its cells kernel ahead on the key-line
//     stream, beside this kernel.  The call therefore leaves cams_pending set until the next step is enqueued, which the planner reads as
//     it reads an import (StepFacts::after_import -> own_fork): that step, too, does nothing on the key-line stream before its own fork
//     event.  It also marks the point stream as holding work (st_dirty), so that an upload in between copies nothing ahead either.
//   * Later steps may run ahead again: what they wait for is step k's fork event or a later one.
// The host copies (cams_host, img_size_host: what stvo_seq_import_streams checks a blob against) change during the call, in host order.
int stvo_seq_restart_cameras(stvo_seq* s, const stvo_cam* cams_host, const int32_t* img_cols, const int32_t* img_rows) {
    if (!s || !cams_host || !img_cols || !img_rows || !s->ctl_staged) return STVO_ERR_INVALID_ARG;
    const int32_t* ctl = s->ctl_stage[s->ctl_stage_next ^ 1];  // the words stvo_seq_control_next_step staged last (host copy)
    bool any = false;
    for (int b = 0; b < s->B; ++b) {
        if (ctl[b] != STVO_STREAM_RESTART) continue;  // entries of RUN and PARK streams are not read
        if (img_cols[b] <= 0 || img_rows[b] <= 0) return STVO_ERR_INVALID_ARG;
        any = true;
    }
    if (!any) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)s->B * sizeof(stvo::CamRestart), span = (bytes + 255) & ~size_t(255);
    if (!s->d_cam_upd) HIP_TRY(ctx, hipMalloc((void**)&s->d_cam_upd, span));
    if (!s->cam_stage[0]) {
        HIP_TRY(ctx, hipHostMalloc((void**)&s->cam_stage[0], 2 * span, hipHostMallocDefault));
        s->cam_stage[1] = reinterpret_cast<stvo::CamRestart*>(reinterpret_cast<char*>(s->cam_stage[0]) + span);
    }
    for (auto& e : s->ev_cam)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int hb = s->cam_stage_next;
    if (s->cam_stage_busy[hb]) {  // the copy that last read this block (two calls ago)
        HIP_TRY(ctx, hipEventSynchronize(s->ev_cam[hb]));
        s->cam_stage_busy[hb] = false;
    }
    stvo::CamRestart* u = s->cam_stage[hb];
    std::memset(u, 0, bytes);
    for (int b = 0; b < s->B; ++b) {
        if (ctl[b] != STVO_STREAM_RESTART) continue;
        u[b].cam = cams_host[b];
        u[b].inv_w = STVO_GRID_COLS / (double)img_cols[b];  // stereoFrame.cpp:47-48, as stvo_seq_create_multi forms them
        u[b].inv_h = STVO_GRID_ROWS / (double)img_rows[b];
        u[b].cols = img_cols[b];
        u[b].rows = img_rows[b];
    }
    HIP_TRY(ctx, hipMemcpyAsync(s->d_cam_upd, u, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(s->ev_cam[hb], ctx->stream));
    s->cam_stage_busy[hb] = true;
    s->cam_stage_next = hb ^ 1;
    stvo::launch_cam_restart(ctx->stream, s->B, s->d_ctl[s->ctl_next], s->d_cam_upd, s->d_cams, s->d_inv_wh, s->d_snap_img);
    s->st_dirty = true;
    s->cams_pending = true;
    for (int b = 0; b < s->B; ++b) {
        if (ctl[b] != STVO_STREAM_RESTART) continue;
        s->cams_host[b] = cams_host[b];
        s->img_size_host[2 * b] = img_cols[b];
        s->img_size_host[2 * b + 1] = img_rows[b];
    }
    return check_launch(ctx);
}

}  // extern "C"
