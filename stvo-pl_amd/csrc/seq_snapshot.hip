// seq_snapshot.hip — export and import of single streams of the device-resident pipeline (stvo_hip.h: snapshots).  The blob: stream_snapshot.h;
// the two kernels: stream_snapshot.hip; the state: seq_state.h.
//
// Ordering.  Both kernels are enqueued on the context's stream, between two steps.  Everything a step writes of a stream's state is
// written on that stream (point association, pose kernel's seed, control kernels, trajectory and track updates) or on the line stream
// IN FRONT of the step's join (ev_join, or the signal the pose kernel waits for): when a step has been enqueued whole, no work of the line
// stream is outstanding that is not ordered before that step's pose kernel — the key-line stage ahead of step k + 1 is enqueued with
// step k + 1.  So export, behind the last step, reads settled state.  Import writes the set the NEXT step tracks against; that step's
// line stream must not start before the unpack kernel has finished, which StepFacts::after_import (step_plan.h) makes sure of.
#include <algorithm>

#include "seq_state.h"
#include "stream_snapshot.h"

namespace stvo {
void launch_snapshot_pack(hipStream_t s, const snap::KernelArgs& a);
void launch_snapshot_unpack(hipStream_t s, const snap::KernelArgs& a);
}  // namespace stvo

namespace {

using namespace stvo;

constexpr int MAX_BLOBS_PER_LAUNCH = 65535;  // grid.y

int seq_flags(const stvo_seq* s) {
    return (s->d_motion_T ? STVO_SNAP_MOTION : 0) | (s->d_traj_state ? STVO_SNAP_TRAJ : 0) |
           ((s->d_traj_state && s->traj_prm.keyframes) ? STVO_SNAP_TRAJ_KF : 0) | (s->d_tracks ? STVO_SNAP_TRACKS : 0) |
           (s->d_kf ? STVO_SNAP_KF_SETS : 0);
}

// The arrays of the pipeline a snapshot reads or writes, section by section: the stereo set the last step built (the one the next step
// tracks against), the copy of the track state the next step reads, the key-frame sets.
void stream_arrays(const stvo_seq* s, snap::StreamArrays& a) {
    std::memset(&a, 0, sizeof(a));
    const int K = s->K, M = s->M;
    auto set_arrays = [&](int first, const StereoSetPtrs& q) {
        void* p[10] = {q.rc, q.desc, q.spl, q.epl, q.sP, q.eP, q.le, q.s2l, q.s2lm, q.ldesc};
        for (int i = 0; i < 10; ++i) a.ptr[first + i] = static_cast<char*>(p[i]);
    };
    set_arrays(snap::SEC_SET, s->set[s->prev_set()]);
    a.ptr[snap::SEC_MOTION] = reinterpret_cast<char*>(s->d_motion_T);
    a.ptr[snap::SEC_TRAJ] = reinterpret_cast<char*>(s->d_traj_state);
    if (s->d_tracks) {
        const size_t row = (size_t)((s->track_steps & 1ull) ^ 1ull);  // step k reads copy (k + 1) & 1
        a.ptr[snap::SEC_TRACKS_P] = reinterpret_cast<char*>(s->track_row_p(row));
        a.ptr[snap::SEC_TRACKS_L] = reinterpret_cast<char*>(s->track_row_l(row));
    }
    if (s->d_kf) set_arrays(snap::SEC_KF, s->kf_set);
    for (int i = 0; i < snap::NSEC; ++i) a.stride[i] = snap::cap_rows(snap::SECTIONS[i], K, M) * snap::SECTIONS[i].row_bytes;
}

// What every call needs on the device: the image sizes (once), and room for n (stream, layout) pairs on the device and in both staging blocks.
int snapshot_ensure(stvo_seq* s, int n) {
    stvo_ctx* ctx = s->ctx;
    if (!s->d_snap_img) {
        int32_t* p = nullptr;
        HIP_TRY(ctx, hipMalloc((void**)&p, s->img_size_host.size() * sizeof(int32_t)));
        if (!upload_now(ctx, p, s->img_size_host.data(), s->img_size_host.size() * sizeof(int32_t), "hipMemcpy snapshot image sizes")) {
            (void)hipFree(p);
            return STVO_ERR_HIP;
        }
        s->d_snap_img = p;
    }
    for (auto& e : s->ev_snap)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (n > s->snap_streams_cap) {
        // (a kernel or a copy of an earlier call may still use the old blocks)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        s->snap_stage_busy[0] = s->snap_stage_busy[1] = false;
        if (s->d_snap_streams) (void)hipFree(s->d_snap_streams);
        if (s->snap_stage[0]) (void)hipHostFree(s->snap_stage[0]);
        s->d_snap_streams = nullptr; s->snap_stage[0] = s->snap_stage[1] = nullptr; s->snap_streams_cap = 0;
        const int cap = std::max(n, s->B);
        const size_t span = ((size_t)cap * 2 * sizeof(int32_t) + 255) & ~size_t(255);
        HIP_TRY(ctx, hipMalloc((void**)&s->d_snap_streams, span));
        HIP_TRY(ctx, hipHostMalloc((void**)&s->snap_stage[0], 2 * span, hipHostMallocDefault));
        s->snap_stage[1] = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(s->snap_stage[0]) + span);
        s->snap_streams_cap = cap;
    }
    return STVO_OK;
}

// The (stream, layout) pairs of a call to the device, through the staging block that is free (stvo_seq_control_next_step's pattern).
int upload_stream_list(stvo_seq* s, int n, const int32_t* streams, const int32_t* layout_of) {
    stvo_ctx* ctx = s->ctx;
    const int hb = s->snap_stage_next;
    if (s->snap_stage_busy[hb]) {  // the copy that last read this block, two calls ago
        HIP_TRY(ctx, hipEventSynchronize(s->ev_snap[hb]));
        s->snap_stage_busy[hb] = false;
    }
    for (int i = 0; i < n; ++i) {
        s->snap_stage[hb][2 * i] = streams[i];
        s->snap_stage[hb][2 * i + 1] = layout_of ? layout_of[i] : 0;
    }
    HIP_TRY(ctx, hipMemcpyAsync(s->d_snap_streams, s->snap_stage[hb], (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(s->ev_snap[hb], ctx->stream));
    s->snap_stage_busy[hb] = true;
    s->snap_stage_next = hb ^ 1;
    return STVO_OK;
}

void common_args(const stvo_seq* s, snap::KernelArgs& a) {
    a.K = s->K; a.M = s->M;
    stream_arrays(s, a.arr);
    const StereoSetPtrs& q = s->set[s->prev_set()];
    a.n = q.n; a.nl = q.nl;
    a.kf_hdr = s->d_kf_hdr;
    a.cams = s->d_cams; a.img_size = s->d_snap_img;
    a.mp = s->mp; a.op = s->op;
}

template <class Launch>
int launch_sliced(stvo_seq* s, snap::KernelArgs& a, int n, char* blobs, int64_t stride, Launch&& launch) {
    for (int first = 0; first < n; first += MAX_BLOBS_PER_LAUNCH) {
        a.n_blobs = std::min(n - first, MAX_BLOBS_PER_LAUNCH);
        a.streams = s->d_snap_streams + 2 * (size_t)first;
        a.blobs = blobs + (int64_t)first * stride;
        a.blob_stride = stride;
        launch(s->ctx->stream, a);
    }
    return check_launch(s->ctx);
}

int grow_snap_buf(stvo_seq* s, size_t bytes) {
    stvo_ctx* ctx = s->ctx;
    if (bytes <= s->snap_buf_bytes) return STVO_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (s->snap_buf) (void)hipFree(s->snap_buf);
    s->snap_buf = nullptr; s->snap_buf_bytes = 0;
    HIP_TRY(ctx, hipMalloc((void**)&s->snap_buf, bytes));
    s->snap_buf_bytes = bytes;
    return STVO_OK;
}

// Everything an import decides on the host, from the n headers: the refusals, the distinct layouts and which blob has which, and what the
// stereo set will hold of key-lines.
struct ImportPlan {
    snap::KernelArgs args;
    std::vector<int32_t> layout_of;
    int max_nl = 0;
};
int plan_import(const stvo_seq* s, int n, const int32_t* streams, const snap::Header* hdr, int64_t stride, ImportPlan& p) {
    std::vector<char> named((size_t)s->B, 0);
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= s->B || named[streams[i]]) return STVO_ERR_INVALID_ARG;
        named[streams[i]] = 1;
    }
    snap::KernelArgs& a = p.args;
    std::memset(&a, 0, sizeof(a));
    p.layout_of.assign((size_t)n, 0);
    int n_lay = 0, Kmax = 0, Mmax = 0, capacity = STVO_OK;
    const int flags = seq_flags(s);
    for (int i = 0; i < n; ++i) {
        const int b = streams[i];
        snap::Target t{s->K, s->M, flags, s->cams_host[b], s->img_size_host[2 * b], s->img_size_host[2 * b + 1], s->mp, s->op};
        const int rc = snap::check_header(hdr[i], t, stride);
        if (rc == STVO_ERR_CAPACITY) capacity = rc;  // (a malformed blob further on still reads as malformed)
        else if (rc != STVO_OK) return rc;
        int k = 0;
        while (k < n_lay && (a.lay[k].K != hdr[i].K || a.lay[k].M != hdr[i].M)) ++k;
        if (k == n_lay) {
            if (n_lay == snap::MAX_LAYOUTS) return STVO_ERR_INVALID_ARG;
            snap::layout(hdr[i].K, hdr[i].M, flags, a.lay[n_lay++]);
        }
        p.layout_of[i] = k;
        Kmax = std::max(Kmax, hdr[i].K); Mmax = std::max(Mmax, hdr[i].M);
        p.max_nl = std::max(p.max_nl, hdr[i].nl);
    }
    if (capacity != STVO_OK) return capacity;
    if (!snap::make_chunks(Kmax, Mmax, flags, a)) return STVO_ERR_INVALID_ARG;
    return STVO_OK;
}

// Enqueues the unpack of n blobs in device memory (headers already checked: `p`) and moves the host's facts with it.
int enqueue_import(stvo_seq* s, int n, const int32_t* streams, const void* blobs_dev, int64_t stride, ImportPlan& p) {
    TRY(upload_stream_list(s, n, streams, p.layout_of.data()));
    common_args(s, p.args);
    TRY(launch_sliced(s, p.args, n, const_cast<char*>(static_cast<const char*>(blobs_dev)), stride, launch_snapshot_unpack));
    // what is no per-stream state but must stay true of the set the next step tracks against
    const int ps = s->prev_set();
    if (p.max_nl > 0) {
        s->set_lines[ps] = true;
        s->set_lines_cap[ps] = std::max(s->set_lines_cap[ps], std::min(s->M, std::max(64, (p.max_nl + 63) & ~63)));
    }
    if (s->frame_idx == 0) s->frame_idx = 1;  // the pipeline counts as stepped: its next step tracks
    s->imported = true;
    s->st_dirty = true;
    return STVO_OK;
}

}  // namespace

extern "C" {

int stvo_seq_snapshot_layout(int K, int M, int flags, stvo_snapshot_layout* out) {
    if (!out || !stvo::snap::layout(K, M, flags, *out)) return STVO_ERR_INVALID_ARG;
    return STVO_OK;
}

int stvo_seq_snapshot_info(const stvo_seq* s, int32_t* K, int32_t* M, int32_t* flags, int64_t* bytes_per_stream) {
    if (!s) return STVO_ERR_INVALID_ARG;
    stvo_snapshot_layout l;
    if (!stvo::snap::layout(s->K, s->M, seq_flags(s), l)) return STVO_ERR_INVALID_ARG;
    if (K) *K = s->K;
    if (M) *M = s->M;
    if (flags) *flags = l.flags;
    if (bytes_per_stream) *bytes_per_stream = l.bytes;
    return STVO_OK;
}

int stvo_seq_export_streams_dev(stvo_seq* s, int n, const int32_t* streams_host, void* blobs_dev) {
    if (!s || n < 0 || !streams_host || !blobs_dev || (reinterpret_cast<uintptr_t>(blobs_dev) & 15)) return STVO_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (streams_host[i] < 0 || streams_host[i] >= s->B) return STVO_ERR_INVALID_ARG;
    if (n == 0) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    snap::KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    const int flags = seq_flags(s);
    if (!snap::layout(s->K, s->M, flags, a.lay[0]) || !snap::make_chunks(s->K, s->M, flags, a)) return STVO_ERR_INVALID_ARG;
    TRY(snapshot_ensure(s, n));
    TRY(upload_stream_list(s, n, streams_host, nullptr));
    common_args(s, a);
    return launch_sliced(s, a, n, static_cast<char*>(blobs_dev), a.lay[0].bytes, launch_snapshot_pack);
}

int stvo_seq_export_streams(stvo_seq* s, int n, const int32_t* streams_host, void* blobs_host) {
    if (!s || n < 0 || !streams_host || !blobs_host) return STVO_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (streams_host[i] < 0 || streams_host[i] >= s->B) return STVO_ERR_INVALID_ARG;
    if (n == 0) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int64_t bytes = 0;
    TRY(stvo_seq_snapshot_info(s, nullptr, nullptr, nullptr, &bytes));
    TRY(grow_snap_buf(s, (size_t)n * (size_t)bytes));
    TRY(stvo_seq_export_streams_dev(s, n, streams_host, s->snap_buf));
    HIP_TRY(ctx, hipMemcpyAsync(blobs_host, s->snap_buf, (size_t)n * (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->snap_stage_busy[0] = s->snap_stage_busy[1] = false;  // every staging copy enqueued so far has read its block
    return STVO_OK;
}

// (synchronises the context's stream once: the n headers come to the host with one small strided copy before anything is decided)
int stvo_seq_import_streams_dev(stvo_seq* s, int n, const int32_t* streams_host, const void* blobs_dev, int64_t blob_stride) {
    if (!s || n < 0 || !streams_host || !blobs_dev || (reinterpret_cast<uintptr_t>(blobs_dev) & 15) || blob_stride < snap::HEADER_BYTES ||
        (blob_stride & 15))
        return STVO_ERR_INVALID_ARG;
    if (n == 0) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<snap::Header> hdr((size_t)n);
    HIP_TRY(ctx, hipMemcpy2DAsync(hdr.data(), sizeof(snap::Header), blobs_dev, (size_t)blob_stride, sizeof(snap::Header), (size_t)n,
                                  hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ImportPlan p;
    TRY(plan_import(s, n, streams_host, hdr.data(), blob_stride, p));
    TRY(snapshot_ensure(s, n));
    return enqueue_import(s, n, streams_host, blobs_dev, blob_stride, p);
}

int stvo_seq_import_streams(stvo_seq* s, int n, const int32_t* streams_host, const void* blobs_host, int64_t blob_stride) {
    if (!s || n < 0 || !streams_host || !blobs_host || blob_stride < snap::HEADER_BYTES || (blob_stride & 15)) return STVO_ERR_INVALID_ARG;
    if (n == 0) return STVO_OK;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<snap::Header> hdr((size_t)n);
    for (int i = 0; i < n; ++i) std::memcpy(&hdr[i], static_cast<const char*>(blobs_host) + (int64_t)i * blob_stride, sizeof(snap::Header));
    ImportPlan p;
    TRY(plan_import(s, n, streams_host, hdr.data(), blob_stride, p));
    TRY(snapshot_ensure(s, n));
    // one copy: blob i of the staging buffer starts at i * blob_stride as well (the caller's buffer ends with the last blob's bytes)
    const size_t total = (size_t)(n - 1) * (size_t)blob_stride + (size_t)hdr[(size_t)n - 1].bytes;
    TRY(grow_snap_buf(s, total));
    HIP_TRY(ctx, hipMemcpyAsync(s->snap_buf, blobs_host, total, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_import(s, n, streams_host, s->snap_buf, blob_stride, p));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller's blobs have been read
    s->snap_stage_busy[0] = s->snap_stage_busy[1] = false;
    return STVO_OK;
}

}  // extern "C"
