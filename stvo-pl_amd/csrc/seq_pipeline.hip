// seq_pipeline.hip — device-resident per-frame pipeline for B independent stereo sequences (SURVEY.md §8f
// rank 1): everything between "features extracted" and "pose committed" stays in HBM.
//
//   stvo_seq_push(features of frame k for B sequences)
//     1  point_cells_kernel   cell coordinates of the left key-points, CSR grid of the right key-points
//                             (src/stereoFrame.cpp:129-139 of the reference; GridStructure as CSR)
//     2  K3 grid matcher      StVO::matchGrid (points)               (src/matching.cpp:111-177)
//     3  point_tail_kernel    epipolar / disparity filters, back-projection, sigma2, ordered compaction of
//                             the stereo points and their descriptor rows (stereoFrame.cpp:149-172)
//     4  line_cells_kernel    end-point cells, Bresenham rasterisation of the right lines into the CSR grid,
//                             unit directions (stereoFrame.cpp:318-338, src/lineIterator.cpp:34-77)
//     5  K3 grid matcher      StVO::matchGrid (lines)                (src/matching.cpp:179-258)
//     6  line_tail_kernel     overlap, end-point re-intersection, disparity filters, back-projection,
//                             ordered compaction (stereoFrame.cpp:348-397, :405-415, :473-508)
//     7  K1/K2                f2f mutual matching against the previous frame's stereo sets
//                             (src/stereoFrameHandler.cpp:131-180 -> matching.cpp:63-91)
//     8  pose kernel          optimizePose                           (src/stereoFrameHandler.cpp:307-392)
//   then the two stereo-set buffers swap roles (updateFrame, :89-100).  One upload, one small download
//   (B pose results + counters) and one synchronisation per frame.
// Here: create / destroy, the raw frame slots and the two upload routes, the step, read, fetch and push.  The kernels of stages 1, 3, 4
// and 6: stereo_assoc_kernels.hip.  The state: seq_state.h.  The optional features: seq_features.hip.  The test hooks: seq_debug.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>

#include "seq_state.h"
// (behind the HIP headers: its functions are __host__ __device__)
#include "pose_math.h"

namespace {

// ---- 0: device-resident features (e.g. the output of stvo_orb_detect_dev) into a raw frame slot ------------------------------
struct IngestArgs {
    int B, K, M, has_points, has_lines;
    stvo_frame_features f;  // DEVICE pointers, counts included
    stvo::RawFrame raw;     // the slot
};
__global__ __launch_bounds__(256) void seq_ingest_kernel(IngestArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    auto count = [&](const int32_t* n, int cap, int stride) { return n ? min(max(n[b], 0), min(cap, stride)) : 0; };
    const int nl = a.has_points ? count(a.f.n_kp_l, a.K, a.f.stride_kp) : 0, nr = a.has_points ? count(a.f.n_kp_r, a.K, a.f.stride_kp) : 0;
    const int ml = a.has_lines ? count(a.f.n_kl_l, a.M, a.f.stride_kl) : 0, mr = a.has_lines ? count(a.f.n_kl_r, a.M, a.f.stride_kl) : 0;
    if (tid == 0) {
        a.raw.n_kp_l[b] = nl;
        a.raw.n_kp_r[b] = nr;
        a.raw.n_kl_l[b] = ml;
        a.raw.n_kl_r[b] = mr;
    }
    const size_t sp = (size_t)b * a.f.stride_kp, dp = (size_t)b * a.K, sl = (size_t)b * a.f.stride_kl, dl = (size_t)b * a.M;
    auto rows32 = [&](const uint8_t* src, uint8_t* dst, int n) {  // 32-byte rows as two 16-byte words
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (int i = tid; i < 2 * n; i += 256) d4[i] = s4[i];
    };
    for (int i = tid; i < 2 * nl; i += 256) a.raw.kp_l[dp * 2 + i] = a.f.kp_l[sp * 2 + i];
    for (int i = tid; i < nl; i += 256) a.raw.oct_l[dp + i] = a.f.oct_l ? a.f.oct_l[sp + i] : 0;  // no octaves: one pyramid level
    rows32(a.f.desc_l + sp * 32, a.raw.desc_l + dp * 32, nl);
    for (int i = tid; i < 2 * nr; i += 256) a.raw.kp_r[dp * 2 + i] = a.f.kp_r[sp * 2 + i];
    rows32(a.f.desc_r + sp * 32, a.raw.desc_r + dp * 32, nr);
    for (int i = tid; i < 4 * ml; i += 256) a.raw.kl_l[dl * 4 + i] = a.f.kl_l[sl * 4 + i];
    for (int i = tid; i < ml; i += 256) a.raw.oct_ll[dl + i] = a.f.oct_ll ? a.f.oct_ll[sl + i] : 0;
    if (ml) rows32(a.f.ldesc_l + sl * 32, a.raw.ldesc_l + dl * 32, ml);
    for (int i = tid; i < 4 * mr; i += 256) a.raw.kl_r[dl * 4 + i] = a.f.kl_r[sl * 4 + i];
    if (mr) rows32(a.f.ldesc_r + sl * 32, a.raw.ldesc_r + dl * 32, mr);
}

// The per-slot records for n raw frame slots: slots 0 / 1 keep what is known of their contents, the others start empty, no slot is split.
void reset_slot_records(stvo_seq* s, size_t n) {
    s->raw_lines.resize(2); s->raw_lines.resize(n, 0);
    s->raw_max_lines.resize(2); s->raw_max_lines.resize(n, 0);
    s->raw_split.assign(n, 0);
}

}  // namespace

namespace stvo {

// What the two stereo matchers share: the problem of `rows` x `rows` features per frame, and the owner's scratch — its eligible-pair
// arrays only with best_lr_matches (GridScratch::elig == nullptr: two full scan passes).
static GridMatch grid_args(const stvo_seq* s, int rows, int xy_width, int items_stride, const GridScratch& scratch) {
    GridMatch g;
    std::memset(&g, 0, sizeof(g));
    const GridMatrixDims md = grid_matrix_dims(rows, rows);
    GridProblem& p = g.p;
    p.B = s->B; p.stride1 = rows; p.stride2 = rows; p.xy_width = xy_width; p.items_stride = items_stride; p.words64 = md.words64; p.n1p = md.n1p;
    p.w = stvo_grid_window{s->mp.matching_s_ws, 0, 0, 0};  // stereoFrame.cpp:141-143, :340-342
    p.ratio = s->ratio_grid;  // minRatio12P for the key-lines too (sic, matching.cpp:241)
    p.mutual = s->mp.best_lr_matches;
    g.s = scratch;
    if (!p.mutual) g.s.elig = nullptr, g.s.elig_cnt = nullptr, g.s.ovf = nullptr;
    return g;
}

// The arguments of the stereo point matcher, up to what the plan decides (lean_cells, has_tail, fused_cells).
GridMatch point_grid_args(const stvo_seq* s, const SeqDev& d) {
    GridMatch g = grid_args(s, s->K, 2, s->K, s->grid_p);
    GridProblem& p = g.p;
    p.cell_xy1 = d.pxy_l; p.d1 = d.raw.desc_l; p.n1 = d.raw.n_kp_l; p.cell_start = d.pstart; p.cell_items = d.pitems;
    p.d2 = d.raw.desc_r; p.n2 = d.raw.n_kp_r;
    p.rank = d.prank; p.perm = d.pperm; p.m12 = s->fb.m12s_p;
    // device CSR: right key-points are numbered in cell order, one grid row per window — the range form
    g.r.range1 = d.prange; g.r.cell2 = d.pcell; g.r.lstart = d.plstart; g.r.lperm = d.plperm;
    return g;
}

// ... and of the general matcher for the key-lines
GridMatch line_grid_args(const stvo_seq* s, const SeqDev& d) {
    GridMatch g = grid_args(s, s->M, 4, s->M * LENT, s->grid_l);
    GridProblem& p = g.p;
    p.cell_xy1 = d.lxy_l; p.d1 = d.raw.ldesc_l; p.n1 = d.raw.n_kl_l; p.cell_start = d.lstart; p.cell_items = d.litems;
    p.d2 = d.raw.ldesc_r; p.n2 = d.raw.n_kl_r; p.dir2 = d.ldir;
    p.line_sim_th = s->mp.line_sim_th;
    p.rank = d.lrank; p.perm = d.lperm; p.m12 = s->fb.m12s_l;
    return g;
}

}  // namespace stvo

extern "C" {

int stvo_seq_create_multi(stvo_ctx* ctx, int B, int max_keypoints, int max_keylines, const int32_t* img_cols,
                          const int32_t* img_rows, const stvo_cam* cams, const stvo_match_params* mp,
                          const stvo_opt_params* op, stvo_seq** out) {
    if (!ctx || !out || B <= 0 || max_keypoints <= 0 || max_keylines < 0 || !img_cols || !img_rows || !cams || !mp || !op)
        return STVO_ERR_INVALID_ARG;
    for (int b = 0; b < B; ++b)
        if (img_cols[b] <= 0 || img_rows[b] <= 0) return STVO_ERR_INVALID_ARG;
    if (max_keypoints > STVO_POSE_MAX_POINTS || max_keylines > STVO_POSE_MAX_LINES) return STVO_ERR_CAPACITY;
    // the pipeline runs the context's matching scratch (cand / claim / qsel: max_rows x max_batch ints, nsel: [5][max_batch])
    // with K = max_keypoints rounded up to 64 as row stride: validate the ROUNDED figures
    const int K = (max_keypoints + 63) & ~63;
    const int M = max_keylines > 0 ? ((max_keylines + 63) & ~63) : 64;
    if (B > ctx->max_batch || K > ctx->max_rows || (size_t)B * (size_t)K > (size_t)ctx->max_batch * (size_t)ctx->max_rows)
        return STVO_ERR_CAPACITY;
    if (!stvo::match_scratch_fits(B, K, ctx->knn_capacity)) return STVO_ERR_CAPACITY;  // forward top-2 + reverse-check scratch (match_scratch.h)
    if (!(mp->min_ratio_12_p <= 1.0f) || !(mp->min_ratio_12_l <= 1.0f)) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo_seq* s = new (std::nothrow) stvo_seq();
    if (!s) return STVO_ERR_HIP;
    s->ctx = ctx;
    s->B = s->d.B = B; s->K = s->d.K = K; s->M = s->d.M = M;
    s->mp = s->d.mp = *mp;
    s->op = *op;
    s->ratio_grid = mp->min_ratio_12_p_d > 0.0 ? mp->min_ratio_12_p_d : (double)mp->min_ratio_12_p;
    if (!(s->ratio_grid <= 1.0)) {
        delete s;
        return STVO_ERR_INVALID_ARG;
    }
    const size_t nb = (size_t)B;
    s->cams_host.assign(cams, cams + B);  // what a snapshot's header says of a stream (seq_snapshot.hip)
    for (int b = 0; b < B; ++b) s->img_size_host.insert(s->img_size_host.end(), {img_cols[b], img_rows[b]});
    s->raw_span = stvo::raw_frame_span(B, K, M);
    s->dev_bytes = stvo::seq_layout(*s, nullptr);
    if (!stvo::match_scratch_fits(B, M, s->lazy_l.knn_capacity)) {  // the key-line scratch, as the context's for the key-points above
        delete s;
        return STVO_ERR_CAPACITY;
    }
    bool ok = hip_ok(ctx, hipMalloc((void**)&s->dev, s->dev_bytes), "hipMalloc seq") && zero_device(ctx, s->dev, s->dev_bytes, "hipMemset seq");
    for (char*& h : s->raw_host) ok = ok && hip_ok(ctx, hipHostMalloc((void**)&h, s->raw_span.bytes, hipHostMallocDefault), "hipHostMalloc seq");
    ok = ok && hip_ok(ctx, hipHostMalloc((void**)&s->out_host, nb * (sizeof(stvo_pose_result) + 16), hipHostMallocDefault), "hipHostMalloc seq out") &&
         hip_ok(ctx, hipStreamCreateWithFlags(&s->line_stream, hipStreamNonBlocking), "hipStreamCreate seq");
    for (hipEvent_t* e : {&s->ev_fork, &s->ev_join, &s->ev_cells, &s->ev_upload, &s->ev_stage[0], &s->ev_stage[1]})
        ok = ok && hip_ok(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate seq");
    s->zero_copy = B <= 16;
    if (!ok) {
        stvo_seq_destroy(s);
        return STVO_ERR_HIP;
    }
    for (char* h : s->raw_host) std::memset(h, 0, s->raw_span.bytes);
    stvo::seq_layout(*s, s->dev);
    reset_slot_records(s, 2);
    {
        std::vector<double> iw(2 * nb);
        for (int b = 0; b < B; ++b) {
            iw[2 * b + 0] = STVO_GRID_COLS / (double)img_cols[b];  // stereoFrame.cpp:47-48
            iw[2 * b + 1] = STVO_GRID_ROWS / (double)img_rows[b];
        }
        double qtab[stvo::STVO_POSE_QTAB];  // sqrt(sigma2) per pyramid level: the same operations as the kernels' own computation
        for (int l = 0; l < stvo::STVO_POSE_QTAB; ++l) qtab[l] = std::sqrt(pm::level_sigma2(l, s->mp.orb_scale_factor));
        ok = upload_now(ctx, s->d_qtab, qtab, sizeof(qtab), "hipMemcpy qtab") &&
             upload_now(ctx, s->d_cams, cams, nb * sizeof(stvo_cam), "hipMemcpy cams") &&
             upload_now(ctx, s->d_inv_wh, iw.data(), iw.size() * sizeof(double), "hipMemcpy inv_wh");
        if (!ok) {
            stvo_seq_destroy(s);
            return STVO_ERR_HIP;
        }
    }
    *out = s;
    return STVO_OK;
}

int stvo_seq_create(stvo_ctx* ctx, int B, int max_keypoints, int max_keylines, int img_cols, int img_rows,
                    const stvo_cam* cam, const stvo_match_params* mp, const stvo_opt_params* op, stvo_seq** out) {
    if (B <= 0 || !cam) return STVO_ERR_INVALID_ARG;
    const std::vector<int32_t> cols((size_t)B, img_cols), rows((size_t)B, img_rows);
    const std::vector<stvo_cam> cams((size_t)B, *cam);
    return stvo_seq_create_multi(ctx, B, max_keypoints, max_keylines, cols.data(), rows.data(), cams.data(), mp, op, out);
}

// More raw frame slots than the two of stvo_seq_push: a throughput caller uploads n_slots consecutive frames of every
// sequence once and rotates stvo_seq_step_dev through them, so that the per-step working set is not the same two frames
// over and over.  Slots 0 / 1 keep their contents.
int stvo_seq_set_slots(stvo_seq* s, int n_slots) {
    if (!s || n_slots < 2 || n_slots > STVO_SEQ_MAX_SLOTS) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (s->extra_raw) {
        HIP_TRY(ctx, hipFree(s->extra_raw));
        s->extra_raw = nullptr;
    }
    s->raw_dev.resize(2);
    reset_slot_records(s, n_slots);
    if (n_slots > 2) {
        HIP_TRY(ctx, hipMalloc((void**)&s->extra_raw, (size_t)(n_slots - 2) * s->raw_span.bytes));
        if (!zero_device(ctx, s->extra_raw, (size_t)(n_slots - 2) * s->raw_span.bytes, "hipMemset seq raw")) return STVO_ERR_HIP;
        for (int k = 2; k < n_slots; ++k) s->raw_dev.push_back(s->extra_raw + (size_t)(k - 2) * s->raw_span.bytes);
    }
    return STVO_OK;
}

int stvo_seq_destroy(stvo_seq* s) {
    if (!s) return STVO_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    if (s->line_stream) {
        (void)hipStreamSynchronize(s->line_stream);
        (void)hipStreamDestroy(s->line_stream);
    }
    // (d_ctl and ctl_stage: one allocation for both copies each)
    for (void* p : {(void*)s->d_prof, (void*)s->d_motion_T, (void*)s->d_traj_state, (void*)s->d_traj_ring, (void*)s->d_tracks, (void*)s->d_kf,
                    (void*)s->d_ctl[0], (void*)s->d_cam_upd, (void*)s->dev, (void*)s->extra_raw, (void*)s->d_snap_img, (void*)s->d_snap_streams, (void*)s->snap_buf})
        if (p) (void)hipFree(p);
    // (snap_stage: one allocation for both blocks)
    for (void* p : {(void*)s->ctl_stage[0], (void*)s->cam_stage[0], (void*)s->snap_stage[0], (void*)s->fetch_host, (void*)s->raw_host[0], (void*)s->raw_host[1], (void*)s->out_host})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {s->ev_snap[0], s->ev_snap[1], s->ev_ctl[0], s->ev_ctl[1], s->ev_cam[0], s->ev_cam[1], s->ev_fork, s->ev_join, s->ev_cells, s->ev_upload, s->ev_stage[0], s->ev_stage[1], s->ev_fetch})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->tev) (void)hipEventDestroy(e);
    delete s;
    return STVO_OK;
}

// Copies one frame's features of all B sequences into device slot 0 / 1 (pinned gather + ONE H2D, asynchronous
// on the context's stream).
int stvo_seq_upload(stvo_seq* s, int slot, const stvo_frame_features* f) {
    if (!s || !f || slot < 0 || slot >= (int)s->raw_dev.size()) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int B = s->B, K = s->K, M = s->M;
    // contract: a positive count needs its arrays (checked before anything is touched)
    for (int b = 0; b < B; ++b) {
        const bool kl = f->n_kp_l && f->n_kp_l[b] > 0, kr = f->n_kp_r && f->n_kp_r[b] > 0;
        const bool ll = f->n_kl_l && f->n_kl_l[b] > 0 && s->op.has_lines, lr = f->n_kl_r && f->n_kl_r[b] > 0 && s->op.has_lines;
        if ((kl && (!f->kp_l || !f->oct_l || !f->desc_l)) || (kr && (!f->kp_r || !f->desc_r)) ||
            (ll && (!f->kl_l || !f->oct_ll || !f->ldesc_l)) || (lr && (!f->kl_r || !f->ldesc_r)))
            return STVO_ERR_INVALID_ARG;
    }
    // two pinned staging blocks used alternately: only wait for the copy that last read THIS block (two uploads ago)
    const int sb = s->stage_next;
    s->stage_next ^= 1;
    if (s->stage_upload[sb] > s->uploads_done) {  // everything enqueued so far covers that copy
        HIP_TRY(ctx, hipEventRecord(s->ev_stage[sb], ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(s->ev_stage[sb]));
        if (s->line_stream) HIP_TRY(ctx, hipStreamSynchronize(s->line_stream));  // (its share of a split copy reads the same block)
        s->uploads_done = s->uploads;
    }
    char* H = s->raw_host[sb];
    const stvo::RawFrame h = stvo::raw_frame<false>(H, B, K, M);
    int32_t *nkl = h.n_kp_l, *nkr = h.n_kp_r, *nll = h.n_kl_l, *nlr = h.n_kl_r;
    auto rows = [](auto* dst, const auto* src, size_t drow, size_t srow, int n, int width) {  // n rows of `width` elements, caller's row srow -> the block's row drow
        std::memcpy(dst + drow * width, src + srow * width, (size_t)n * width * sizeof(*dst));
    };
    int max_lines = 0;
    for (int b = 0; b < B; ++b) {
        const int a = f->n_kp_l ? f->n_kp_l[b] : 0, r = f->n_kp_r ? f->n_kp_r[b] : 0;
        const int la = (f->n_kl_l && s->op.has_lines) ? f->n_kl_l[b] : 0, lr = (f->n_kl_r && s->op.has_lines) ? f->n_kl_r[b] : 0;
        if (a < 0 || r < 0 || la < 0 || lr < 0 || a > K || r > K || la > M || lr > M || a > f->stride_kp || r > f->stride_kp ||
            la > f->stride_kl || lr > f->stride_kl)
            return STVO_ERR_CAPACITY;
        nkl[b] = s->op.has_points ? a : 0;
        nkr[b] = s->op.has_points ? r : 0;
        nll[b] = la;
        nlr[b] = lr;
        max_lines = std::max(max_lines, std::max(la, lr));
        const size_t so = (size_t)b * f->stride_kp, dof = (size_t)b * K;
        if (nkl[b]) {
            rows(h.kp_l, f->kp_l, dof, so, a, 2);
            rows(h.oct_l, f->oct_l, dof, so, a, 1);
            rows(h.desc_l, f->desc_l, dof, so, a, STVO_DESC_BYTES);
        }
        if (nkr[b]) {
            rows(h.kp_r, f->kp_r, dof, so, r, 2);
            rows(h.desc_r, f->desc_r, dof, so, r, STVO_DESC_BYTES);
        }
        const size_t sl = (size_t)b * f->stride_kl, dl = (size_t)b * M;
        if (la) {
            rows(h.kl_l, f->kl_l, dl, sl, la, 4);
            rows(h.oct_ll, f->oct_ll, dl, sl, la, 1);
            rows(h.ldesc_l, f->ldesc_l, dl, sl, la, STVO_DESC_BYTES);
        }
        if (lr) {
            rows(h.kl_r, f->kl_r, dl, sl, lr, 4);
            rows(h.ldesc_r, f->ldesc_r, dl, sl, lr, STVO_DESC_BYTES);
        }
    }
    bool any_lines = false;
    for (int b = 0; b < B; ++b) any_lines = any_lines || (nll[b] > 0 && nlr[b] > 0);
    s->raw_lines[slot] = any_lines;
    s->raw_max_lines[slot] = max_lines;
    s->raw_split[slot] = 0;
    if (s->raw_span.bytes <= (size_t)4 << 20) {
        // copy kernel instead of the DMA engine: ~5 us less latency for the ~200 KB of one frame
        if (any_lines && s->op.has_points && !s->st_dirty && s->line_stream) {
            const size_t lo = s->raw_span.lines_off;  // the key-line arrays are the tail of a slot (seq_layout.h: raw_frame)
            stvo::launch_copy16(ctx->stream, H, s->raw_dev[slot], lo);
            stvo::launch_copy16(s->line_stream, H + lo, s->raw_dev[slot] + lo, s->raw_span.bytes - lo);
            s->raw_split[slot] = 1;
        } else {
            stvo::launch_copy16(ctx->stream, H, s->raw_dev[slot], s->raw_span.bytes);
        }
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(s->raw_dev[slot], H, s->raw_span.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    s->stage_upload[sb] = ++s->uploads;
    if (s->B >= 64 && s->line_stream) {  // batches: the line stream may read a slot first (stvo_seq::ev_cells); no event in single-stream operation
        HIP_TRY(ctx, hipEventRecord(s->ev_upload, ctx->stream));
        ++s->upload_seq;
    }
    return STVO_OK;
}

// The same for features that are already in device memory (every pointer of `f`, the count arrays included, is a DEVICE
// pointer; oct_l / oct_ll may be NULL = octave 0).  Enqueued on the context's stream, no host transfer, no synchronisation:
// counts are clamped to the capacities on the device instead of being validated on the host.
int stvo_seq_upload_dev(stvo_seq* s, int slot, const stvo_frame_features* f) {
    if (!s || !f || slot < 0 || slot >= (int)s->raw_dev.size()) return STVO_ERR_INVALID_ARG;
    if (f->stride_kp < 0 || f->stride_kl < 0) return STVO_ERR_INVALID_ARG;
    const bool pts = s->op.has_points && f->n_kp_l && f->n_kp_r, lns = s->op.has_lines && f->n_kl_l && f->n_kl_r;
    if ((pts && (!f->kp_l || !f->desc_l || !f->kp_r || !f->desc_r)) || (lns && (!f->kl_l || !f->ldesc_l || !f->kl_r || !f->ldesc_r)))
        return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    IngestArgs a{};
    a.B = s->B; a.K = s->K; a.M = s->M; a.has_points = pts; a.has_lines = lns; a.f = *f;
    a.raw = stvo::raw_frame<false>(s->raw_dev[slot], s->B, s->K, s->M);
    hipLaunchKernelGGL(seq_ingest_kernel, dim3(s->B), dim3(256), 0, ctx->stream, a);
    if (s->B >= 64 && s->line_stream) {
        HIP_TRY(ctx, hipEventRecord(s->ev_upload, ctx->stream));
        ++s->upload_seq;
    }
    s->st_dirty = true;
    s->raw_split[slot] = 0;
    s->raw_max_lines[slot] = s->M;
    s->raw_lines[slot] = lns;  // the line stage runs whenever line arrays were given (empty sets cost two small launches)
    return check_launch(ctx);
}

// One step of the pipeline on the features resident in a slot: gather the facts, plan (step_plan.h), enqueue.
namespace {


// The values a step drew from the epoch counters for the flags it publishes; stvo_seq_step_dev commits them, with the plan, only when
// the whole step has been enqueued.
struct StepPub {
    unsigned pose_flag_value = 0;  // StepPlan::pose_flagged: d_pose_flag reaches it when the pose kernel starts
    unsigned fetch_value = 0;      // StepPlan::fetch_by_pose: the pose kernel publishes it behind the match indices
};

// What the stages of one step share: the plan they carry out and where they enqueue.
struct StepEnq {
    stvo_seq* s;
    stvo_ctx* ctx;
    const stvo::StepPlan& p;
    hipEvent_t* tev;     // live stage timing: STVO_SEQ_NSTAGE event pairs of this step (see stvo_seq_get_stage_timing), or nullptr
    hipStream_t st, sl;  // the point stream, and the stream of the line stage
    const stvo::SeqDev& d;
    const stvo::StereoSetPtrs &cs, &ps;  // the stereo sets the step builds / tracks against
    int32_t* m12l_use;       // the copy of the key-line match indices of this step
    const int32_t* ctl;      // StepFlags::ctl
    void mark(int k, hipStream_t q) const {
        if (tev && !(p.light && k < 2)) (void)hipEventRecord(tev[k], q);
    }
    int point_stage(stvo::GridMatch& g) const;
    int line_stage() const;
    int f2f_and_join() const;
    int pose(StepPub& pub) const;
};

// Everything plan_step reads.  The launch helpers are asked what they were asked before, each only where it was asked before.
void gather_step_facts(const stvo_seq* s, int slot, const stvo::StepFlags& fl, bool timing_events, const stvo::GridMatch& g, stvo::StepFacts& f) {
    f.B = s->B; f.K = s->K; f.M = s->M; f.cus = stvo::device_cu_count();
    f.has_points = s->op.has_points; f.has_lines = s->op.has_lines; f.best_lr_matches = s->mp.best_lr_matches;
    f.lines_now = fl.lines_now; f.lines_prev = fl.lines_prev; f.track = fl.track;
    f.frame_idx = s->frame_idx;
    f.has_control = fl.ctl != nullptr;
    // (imported streams, and cameras written by stvo_seq_restart_cameras: state the point stream holds that the step's line-stream work must follow)
    f.after_import = s->imported || s->cams_pending;
    f.raw_split = s->raw_split[slot]; f.raw_max_lines = s->raw_max_lines[slot];
    f.set_lines_cap_prev = s->set_lines_cap[s->prev_set()]; f.set_lines_cap_cur = s->set_lines_cap[s->cur];
    f.st_dirty = s->st_dirty; f.fetch = s->fetch; f.zero_copy = s->zero_copy;
    f.timing = s->timing; f.timing_events = timing_events;
    f.has_alt_m12l = s->m12l_alt != nullptr;
    f.cells_differ = s->cells_buf[0].pstart != s->cells_buf[1].pstart;
    f.grid_points_fused_ok = f.has_points && stvo::grid_points_fused_ok(g);
    if (f.track) {
        f.match_small_ok_K = stvo::match_small_ok(f.K); f.match_small_ok_M = stvo::match_small_ok(f.M);
        const stvo::PoseRoute r = stvo::pose_route(f.B, s->set[s->prev_set()].rc != nullptr, false);  // as StepEnq::pose launches it
        f.pose_inline_sync_ok = r.inline_sync; f.pose_batch_kernel_selected = r.batch; f.pose_start_flag_ok = r.start_flag;
        f.pose2p_waves_per_pair = r.waves;
    }
    f.sw = stvo::dbg();
}

// ---- stereo association of the key-points into set[cur]
int StepEnq::point_stage(stvo::GridMatch& g) const {
    const int B = s->B;
    if (!p.point_stage) {
        HIP_TRY(ctx, hipMemsetAsync(cs.n, 0, (size_t)B * 4, st));
        return STVO_OK;
    }
    mark(0, st);
    stvo::PointRoute& r = g.r;
    r.lean_cells = p.lean_cells;
    r.has_tail = p.has_tail;
    if (p.has_tail) r.tail = stvo::point_tail_args(d);
    r.fused_cells = p.fused_cells;
    if (p.lines_ahead) HIP_TRY(ctx, hipStreamWaitEvent(sl, s->ev_fork, 0));  // the PREVIOUS step's fork event
    if (p.fused_cells)
        r.cells = stvo::point_cells_args(d);
    else if (p.lean_cells)
        stvo::launch_point_cells(p.cells_ahead ? sl : st, d, true);
    else
        stvo::launch_point_cells(st, d, false);
    if (p.cells_ahead) {
        HIP_TRY(ctx, hipEventRecord(s->ev_cells, sl));
        HIP_TRY(ctx, hipStreamWaitEvent(st, s->ev_cells, 0));
    }
    // light timing: the matcher's start stamp in FRONT of the fork — a barrier packet between the fork and the matcher would give the
    // key-line kernels a head start on the CUs, which the untimed step does not give them (first GPU call of round 6: 0.226 ms
    // instead of the timed region's 0.139)
    hipEvent_t gev_light[2] = {nullptr, tev ? tev[3] : nullptr};
    if (p.light) (void)hipEventRecord(tev[2], st);
    if (p.mid_fork) {
        HIP_TRY(ctx, hipEventRecord(s->ev_fork, st));
        if (!p.lines_ahead) HIP_TRY(ctx, hipStreamWaitEvent(sl, s->ev_fork, 0));
        if (p.gate) stvo::launch_stream_gate(sl, s->d_pose_flag, s->pose_flag_value);
    }
    s->last_point_lean = p.lean_cells;
    s->last_mutual = g.p.mutual != 0;
    stvo::launch_grid_batch(st, g, tev ? (p.light ? gev_light : tev + 2) : nullptr);
    if (!p.has_tail) stvo::launch_point_tail(st, d);
    mark(1, st);
    return STVO_OK;
}

// ---- stereo association of the key-lines into set[cur]
int StepEnq::line_stage() const {
    const int B = s->B;
    if (p.line_stage) {
        s->set_lines_cap[s->cur] = p.Mk;
        s->last_line_fused = p.line_fused;
        if (p.line_fused) {
            stvo::launch_line_stereo_fused(sl, d, p.line_lds, p.Mk, (int)s->mp.best_lr_matches, s->ratio_grid);
        } else {
            stvo::launch_line_cells(sl, d);
            stvo::launch_grid_batch(sl, stvo::line_grid_args(s, d));
            stvo::launch_line_tail(sl, d);
        }
    } else if (p.clear_nl) {
        HIP_TRY(ctx, hipMemsetAsync(cs.nl, 0, (size_t)B * 4, st));
    }
    return STVO_OK;
}

// ---- f2fTracking: prev stereo sets vs curr stereo sets, then the line stream joins (or signals) and the match indices leave for the host
int StepEnq::f2f_and_join() const {
    const int B = s->B;
    auto match_set = [&](const stvo::MatchPlan& m, hipStream_t q, const stvo::MatchScratch& ws, int stride, const uint8_t* da, const int32_t* na,
                         const uint8_t* db, const int32_t* nb, float nnr, int32_t* m12, hipEvent_t* mev) {
        if (m.route == stvo::MatchRoute::SMALL) {
            stvo::launch_match_small(q, B, stride, da, na, db, nb, nnr, s->mp.best_lr_matches, m12, m.small_cap);
            return;
        }
        const stvo::MatchForm form = m.route == stvo::MatchRoute::BOTH_DIRS ? stvo::MatchForm::BOTH_DIRS
                                     : m.route == stvo::MatchRoute::LAZY    ? stvo::MatchForm::LAZY
                                                                            : stvo::MatchForm::ONE_WAY;
        stvo::MatchOptions o;
        o.timing_events = mev;
        o.nseg_cap = m.nseg_cap;
        stvo::launch_match(q, stvo::MatchProblem{B, stride, da, na, db, nb, nnr}, form, ws, m12, o);
    };
    if (p.track) {
        const stvo::MatchScratch w = ctx->match_scratch();
        hipEvent_t mev_light[4] = {tev ? tev[4] : nullptr, tev ? tev[5] : nullptr, nullptr, nullptr};  // (light: no pair around plan + reverse scans)
        if (p.point_stage)
            match_set(p.match_points, st, w, s->K, ps.desc, ps.n, cs.desc, cs.n, s->mp.min_ratio_12_p, s->fb.m12p, tev ? (p.light ? mev_light : tev + 4) : nullptr);
        if (p.match_lines_run)
            match_set(p.match_lines, sl, s->lazy_l.match_scratch(), s->M, ps.ldesc, ps.nl, cs.ldesc, cs.nl, s->mp.min_ratio_12_l, m12l_use, nullptr);
        if (p.clear_m12l) HIP_TRY(ctx, hipMemsetAsync(m12l_use, 0xFF, (size_t)B * s->M * sizeof(int32_t), st));
    }
    if (p.join_signal) {
        stvo::launch_stream_signal(sl, s->d_join_flag, ++s->join_epoch);
    } else if (p.par) {  // join before optimizePose; first frame: nothing to track, but the main stream must still see the line stage's results
        HIP_TRY(ctx, hipEventRecord(s->ev_join, sl));
        HIP_TRY(ctx, hipStreamWaitEvent(st, s->ev_join, 0));
    }
    if (p.fetch_copy) {
        stvo::launch_copy16(st, s->fb.m12s_p, s->fetch_host, s->fb.m12_span());
        HIP_TRY(ctx, hipEventRecord(s->ev_fetch, st));
    }
    return STVO_OK;
}

// ---- optimizePose
int StepEnq::pose(StepPub& pub) const {
    const int B = s->B;
    stvo::PoseProblem a{};
    a.B = B; a.max_pts = s->K; a.max_lines = s->M;
    a.n_prev_pts = s->op.has_points ? ps.n : nullptr;
    a.m12p = s->fb.m12p;
    const stvo::PosePoints pts = stvo::PosePoints::compact(ps.rc, cs.rc, s->d_qtab, s->mp.orb_scale_factor);
    stvo::PoseOptions o;
    a.n_prev_lines = s->op.has_lines ? ps.nl : nullptr;
    a.prev_sP = ps.sP; a.prev_eP = ps.eP; a.prev_spl = ps.spl; a.prev_epl = ps.epl; a.prev_s2l = ps.s2lm;
    a.curr_le = cs.le; a.m12l = m12l_use;
    a.cams = s->d_cams; a.prm = s->op;
    a.init_T = s->d_motion_T; a.next_T = s->d_motion_T;  // (nullptr: DT = I, use_motion_model = false)
    a.results = s->step_results();
    a.inl_p_out = p.inl_zero_copy ? s->fetch_mirror(s->fb.off_inlp) : s->fb.inlp;
    a.inl_l_out = p.inl_zero_copy ? s->fetch_mirror(s->fb.off_inll) : s->fb.inll;
    if (stvo::dbg().pose_prof != stvo::DBG_UNSET) {  // (a developer's buffer, not a schedule)
        if (!s->d_prof) HIP_TRY(ctx, hipMalloc((void**)&s->d_prof, (size_t)B * 16 * sizeof(long long)));
        o.prof_out = s->d_prof;
    }
    stvo::PoseSync& y = o.sync;
    if (p.join_signal) {
        y.wait_flag = s->d_join_flag;
        y.wait_value = s->join_epoch;
    }
    y.lazy_eig = p.lazy_eig ? 1 : 0;
    if (p.fetch_by_pose) {
        y.fetch_src = reinterpret_cast<const uint4*>(s->fb.m12s_p);
        y.fetch_dst = reinterpret_cast<uint4*>(s->fetch_host);
        y.fetch_n16 = (unsigned)(s->fb.m12_span() / 16);
        y.fetch_flag = s->fetch_flag();
        y.fetch_value = pub.fetch_value = ++s->fetch_epoch;
    }
    if (p.pose_flagged) {
        y.start_flag = s->d_pose_flag;
        y.start_value = pub.pose_flag_value = ++s->pose_epoch;
    }
    mark(8, st);
    TRY(launch_pose_ctx(ctx, st, a, pts, o));
    mark(9, st);
    // the one place the results are written: behind it, the streams that restart or are parked read as "no pose in this step"
    if (ctl)
    {   // (the inlier rows of such streams matter to whoever reads them behind the step: the by-product fetch, the feature tracks)
        const bool rows = s->fetch || s->d_tracks;
        stvo::launch_stream_ctl_post(st, B, ctl, a.results, s->d_motion_T, rows ? a.inl_p_out : nullptr, s->K, rows ? a.inl_l_out : nullptr, s->M);
    }
    if (p.inl_copy) stvo::launch_copy16(st, s->fb.inlp, s->fetch_host + s->fb.off_inlp, s->fb.inl_span());
    return STVO_OK;
}

// Enqueues the kernel chain of one step on the context's stream and the line stream; returns the step's plan and, in `pub`, the flag
// values it handed out.  Of the state of `s` it changes only: the counters the three flags' values are drawn from (pose_epoch, join_epoch,
// fetch_epoch) — a value handed to a launch may reach the device even when a later launch of the step fails, so it is never handed out
// twice (which is why the planner draws none); later steps wait only for what stvo_seq_step_dev commits —, the key-line capacity of the
// set it builds (set_lines_cap[cur]), the stage-timing events it takes, and the test hooks' facts (last_point_lean, last_mutual, last_line_fused).
// The stream operations are those of the step before the planner existed, in the same order.  The queries that enqueue nothing — the
// LDS opt-ins behind grid_points_fused_ok and plan_step's lds_fits (hipGetDevice, and hipFuncSetAttribute the first time), the CU
// count — are the same ones, made under the same conditions, but all in front of the first stream operation instead of between them.
int seq_enqueue_step(stvo_seq* s, int slot, const stvo::StepFlags& fl, stvo::StepPlan& plan, StepPub& pub) {
    stvo_ctx* ctx = s->ctx;
    // live stage timing: STVO_SEQ_NSTAGE event pairs per step (see stvo_seq_get_stage_timing)
    hipEvent_t* tev = nullptr;
    if (s->timing) {
        while (s->tev.size() < s->tev_used + 2 * STVO_SEQ_NSTAGE) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            s->tev.push_back(e);
        }
        if (s->tev.size() >= s->tev_used + 2 * STVO_SEQ_NSTAGE) {
            tev = s->tev.data() + s->tev_used;
            s->tev_used += 2 * STVO_SEQ_NSTAGE;
        }
    }
    pub = StepPub{};
    // ---- gather: the step's arrays, then the facts
    const stvo::StereoSetPtrs& cs = s->set[s->cur];
    stvo::SeqDev d = s->d;
    d.raw = s->raw_view(slot);
    d.cur = cs;
    const size_t res_bytes = (size_t)s->B * sizeof(stvo_pose_result);
    d.host_n = s->zero_copy ? reinterpret_cast<int32_t*>(s->out_host + res_bytes) : nullptr;
    d.host_nl = s->zero_copy ? reinterpret_cast<int32_t*>(s->out_host + res_bytes + (size_t)s->B * 4) : nullptr;
    stvo::GridMatch g;
    if (s->op.has_points) g = stvo::point_grid_args(s, d);
    stvo::StepFacts facts;
    gather_step_facts(s, slot, fl, tev != nullptr, g, facts);
    // ---- plan
    plan = stvo::plan_step(facts, s->hist, [](int lds) {
        return stvo::line_stereo_fused_lds_opt_in(lds);
    });
    const stvo::StepPlan& p = plan;
    // ---- enqueue
    d.zero_nl = p.zero_nl ? 1 : 0;
    const StepEnq e{s, ctx, p, tev, ctx->stream, p.par ? s->line_stream : ctx->stream, d, cs, s->set[s->prev_set()], p.use_alt_m12l ? s->m12l_alt : s->fb.m12l, fl.ctl};
    // a control: the streams that restart or are parked present no previous features.  First on the point stream — behind the previous
    // step's pose kernel, the last reader of these counts, and in front of every event the line stream waits for in this step (step_plan.h)
    if (fl.ctl) stvo::launch_stream_ctl_pre(e.st, s->B, fl.ctl, e.ps.n, e.ps.nl, s->fb.m12p, s->K, e.m12l_use, s->M);
    if (p.fork_at_start) {
        HIP_TRY(ctx, hipEventRecord(s->ev_fork, e.st));
        HIP_TRY(ctx, hipStreamWaitEvent(e.sl, s->ev_fork, 0));
    }
    TRY(e.point_stage(g));
    TRY(e.line_stage());
    TRY(e.f2f_and_join());
    if (p.track) TRY(e.pose(pub));
    return check_launch(ctx);
}

}  // namespace

// Runs the whole per-frame pipeline on the features resident in `slot` (asynchronous; no host transfer).
int stvo_seq_step_dev(stvo_seq* s, int slot) {
    if (!s || slot < 0 || slot >= (int)s->raw_dev.size()) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::StepFlags fl;
    fl.lines_now = s->op.has_lines && s->raw_lines[slot];
    fl.lines_prev = s->op.has_lines && s->set_lines[s->prev_set()];
    fl.track = s->frame_idx > 0;
    // (the pipeline's own first step tracks nothing and stvo_seq_read zeroes its results: a control staged for it is consumed without effect)
    fl.ctl = (s->ctl_staged && fl.track) ? s->d_ctl[s->ctl_next] : nullptr;
    {   // the grid buffers of this step (stvo_seq::cells_buf), and the line stream behind every upload the point stream holds
        const stvo_seq::CellsBuf& cb = s->cells_buf[s->frame_idx & 1];
        s->d.pstart = cb.pstart; s->d.pperm = cb.pperm; s->d.pcell = cb.pcell; s->d.plperm = cb.plperm; s->d.plstart = cb.plstart;
        if (s->line_stream && s->upload_seen != s->upload_seq) {
            HIP_TRY(ctx, hipStreamWaitEvent(s->line_stream, s->ev_upload, 0));
            s->upload_seen = s->upload_seq;
        }
    }
    stvo::StepPlan plan;
    StepPub pub;
    TRY(seq_enqueue_step(s, slot, fl, plan, pub));
    // the whole step is enqueued: what it published
    stvo::commit(s->hist, plan, s->frame_idx);
    if (plan.pose_flagged) s->pose_flag_value = pub.pose_flag_value;
    s->fetch_by_pose = plan.fetch_by_pose;
    s->fetch_value = pub.fetch_value;
    std::memcpy(s->last_schedule, plan.schedule, sizeof(s->last_schedule));
    s->st_dirty = true;
    s->imported = false;
    s->cams_pending = false;
    s->set_lines[s->cur] = fl.lines_now;
    s->last_lines = fl.lines_now;
    s->last_slot = slot;
    s->cur = (s->cur + 1) % 3;  // updateFrame: curr becomes prev
    s->frame_idx++;
    s->last_ctl = fl.ctl;
    if (s->ctl_staged) {  // one-shot: the next step is all-RUN again, the next control goes to the other device copy
        s->ctl_staged = false;
        s->ctl_next ^= 1;
    }
    if (s->d_traj_state && fl.track) {  // the trajectory behind the pose kernel, reading the results where PoseProblem::results pointed
        // (the step above is committed: a launch that fails here returns its error from a step that counts as taken, ring row included)
        stvo::launch_traj_update(ctx->stream, s->B, s->step_results(), s->traj_prm, s->d_traj_state,
                                 s->d_traj_ring + (size_t)(s->traj_steps % (unsigned long long)s->traj_log_steps) * s->B, fl.ctl);
        s->traj_steps++;
        if (!s->d_tracks) return check_launch(ctx);
    }
    if (s->d_tracks) return stvo::enqueue_track_update(s, plan, fl);
    return STVO_OK;
}

// Results of the LAST step (synchronises).  counts (optional, [B][4]): stereo points, stereo lines, matched
// points, matched lines of that frame; results are zeroed after the first frame (nothing to track against yet).
int stvo_seq_read(stvo_seq* s, stvo_pose_result* results, int32_t* counts) {
    if (!s) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int B = s->B;
    hipStream_t st = ctx->stream;
    const stvo::StereoSetPtrs& ls = s->set[s->prev_set()];  // the set built by the last step (cur has moved on)
    if (s->d_prof && s->frame_idx > 1) {  // STVO_POSE_PROF: mean phase ticks of the last pose launch (as stvo_time_stage_dev prints them)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        std::vector<long long> h((size_t)B * 16);
        HIP_TRY(ctx, hipMemcpy(h.data(), s->d_prof, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        double m[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int f = 0; f < B; ++f)
            for (int i = 0; i < 16; ++i) m[i] += (double)h[(size_t)f * 16 + i] / B;
        std::fprintf(stderr, "[pose prof] mean ticks/pair: evaluate %.0f  iter-algebra %.0f  cov+isgood+commit %.0f  remove_outliers %.0f  total %.0f | "
                             "eval-compute %.0f  fold %.0f  barrier+sum %.0f | prologue %.0f | wave busy %.0f %.0f | removeOutliers: residuals %.0f  statistics %.0f  re-deal %.0f\n",
                     m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[14], m[8], m[9], m[10], m[11], m[12]);
    }
    const bool track = s->frame_idx > 1;
    char* OH = s->out_host;
    const size_t res_bytes = (size_t)B * sizeof(stvo_pose_result);
    if (!s->zero_copy) {  // small batches: the kernels have written results and counts straight into OH
        if (track) HIP_TRY(ctx, hipMemcpyAsync(OH, s->results, res_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(OH + res_bytes, ls.n, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(OH + res_bytes + (size_t)B * 4, ls.nl, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    s->uploads_done = s->uploads;  // every staging copy enqueued so far has read its block
    s->st_dirty = false;           // (the line stream's work of every step was joined into this stream before its pose kernel)
    const stvo_pose_result* hr = reinterpret_cast<const stvo_pose_result*>(OH);
    const int32_t* hn = reinterpret_cast<const int32_t*>(OH + res_bytes);
    for (int b = 0; b < B; ++b) {
        if (results) {
            if (track) {
                results[b] = hr[b];
                if (results[b].path & stvo::PATH_EIG_PENDING) {  // PoseSync::lazy_eig: SelfAdjointEigenSolver(DT_cov).eigenvalues(), :379-380
                    pm::eig6_ql(results[b].cov, results[b].cov_eig);
                    results[b].path &= ~stvo::PATH_EIG_PENDING;
                }
            }
            else
                std::memset(&results[b], 0, sizeof(stvo_pose_result));
        }
        if (counts) {
            counts[4 * b + 0] = s->op.has_points ? hn[b] : 0;
            counts[4 * b + 1] = s->last_lines ? hn[B + b] : 0;
            counts[4 * b + 2] = track ? hr[b].n_matched_pt : 0;
            counts[4 * b + 3] = track ? hr[b].n_matched_ls : 0;
        }
    }
    return STVO_OK;
}

// What the last enqueued step decided on the host (STVO_SCHED_*): read from the bookkeeping, nothing is launched or awaited.
int stvo_seq_last_schedule(const stvo_seq* s, int32_t out[8]) {
    if (!s || !out) return STVO_ERR_INVALID_ARG;
    std::memcpy(out, s->last_schedule, sizeof(s->last_schedule));
    return STVO_OK;
}

int stvo_seq_strides(const stvo_seq* s, int32_t* stride_pts, int32_t* stride_lines) {
    if (!s) return STVO_ERR_INVALID_ARG;
    if (stride_pts) *stride_pts = s->K;
    if (stride_lines) *stride_lines = s->M;
    return STVO_OK;
}

int stvo_seq_enable_fetch(stvo_seq* s, int enable) {
    if (!s) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (enable && !s->fetch_host) {
        HIP_TRY(ctx, hipHostMalloc((void**)&s->fetch_host, s->fb.mirror_bytes(), hipHostMallocDefault));
        *static_cast<volatile unsigned*>(s->fetch_flag()) = 0u;  // the pose kernel's flag (fetch_by_pose)
        HIP_TRY(ctx, hipEventCreateWithFlags(&s->ev_fetch, hipEventDisableTiming));
    }
    s->fetch = enable != 0;
    return STVO_OK;
}

int stvo_seq_fetch_matches(stvo_seq* s, const int32_t** m12_stereo_pts, const int32_t** m12_stereo_lines,
                           const int32_t** m12_pts, const int32_t** m12_lines) {
    if (!s || !s->fetch || s->frame_idx == 0) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->fetch_by_pose) {
        // the pose kernel of the last step copies the indices and then publishes its number; it may still run.  Bounded poll of the
        // pinned word, then the stream (a launch that failed never publishes)
        const volatile unsigned* flag = s->fetch_flag();
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (unsigned spin = 0; !(seen = (*flag == s->fetch_value)); ++spin)
            if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!seen) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (*flag != s->fetch_value) {  // the kernel ended without publishing: it gave up waiting for the key-line stream (STVO_POSE_INTERNAL)
                std::snprintf(ctx->last_error, sizeof(ctx->last_error), "%s", "the pose kernel did not publish the match indices of the last step (no signal from the key-line stream)");
                return STVO_ERR_HIP;
            }
        }
    } else {
        HIP_TRY(ctx, hipEventSynchronize(s->ev_fetch));  // the f2f stage of the last step; its pose kernel may still run
    }
    if (m12_stereo_pts) *m12_stereo_pts = s->fetch_mirror(0);
    if (m12_stereo_lines) *m12_stereo_lines = s->fetch_mirror(s->fb.off_m12s_l);
    if (m12_pts) *m12_pts = s->fetch_mirror(s->fb.off_m12p);
    if (m12_lines) *m12_lines = s->fetch_mirror(s->fb.off_m12l);
    return STVO_OK;
}

int stvo_seq_fetch_inliers(stvo_seq* s, const int32_t** inl_pts, const int32_t** inl_lines) {
    if (!s || !s->fetch || s->frame_idx < 2) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (inl_pts) *inl_pts = s->fetch_mirror(s->fb.off_inlp);
    if (inl_lines) *inl_lines = s->fetch_mirror(s->fb.off_inll);
    return STVO_OK;
}

// Config::useMotionModel() (src/stereoFrameHandler.cpp:317-324) for every sequence of the pipeline: the rule is applied ON THE DEVICE
// by the commit of the previous step (pose_block.h: t0_commit), the first tracked frame starts from prev_frame->DT = I (:45).
int stvo_seq_set_motion_model(stvo_seq* s, int enable) {
    if (!s) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (s->line_stream) HIP_TRY(ctx, hipStreamSynchronize(s->line_stream));
    if (!enable) {
        if (s->d_motion_T) (void)hipFree(s->d_motion_T);
        s->d_motion_T = nullptr;
    } else {
        if (!s->d_motion_T) HIP_TRY(ctx, hipMalloc((void**)&s->d_motion_T, (size_t)s->B * 16 * sizeof(double)));
        std::vector<double> I((size_t)s->B * 16, 0.0);
        for (int b = 0; b < s->B; ++b)
            for (int i = 0; i < 4; ++i) I[(size_t)b * 16 + i * 5] = 1.0;
        if (!upload_now(ctx, s->d_motion_T, I.data(), I.size() * sizeof(double), "hipMemcpy motion")) return STVO_ERR_HIP;
    }
    return STVO_OK;
}

int stvo_seq_push(stvo_seq* s, const stvo_frame_features* f, stvo_pose_result* results, int32_t* counts) {
    if (!s || !f) return STVO_ERR_INVALID_ARG;
    const int slot = s->frame_idx & 1;  // (slots beyond the first two belong to callers of upload / step_dev)
    TRY(stvo_seq_upload(s, slot, f));
    TRY(stvo_seq_step_dev(s, slot));
    return stvo_seq_read(s, results, counts);
}

}  // extern "C"
