// track_kernel.hip — feature tracks and key-frame sets per stream on the device: one workgroup per stream runs track_update.h (the text
// the host test runs) on the stream's key-points and key-lines behind the step's pose kernel, control kernel and trajectory update, and
// at a key-frame copies the stream's current stereo set into its key-frame set.  The winner of every current feature (the largest
// previous index that names it) is found in LDS; global memory sees plain vector stores only, rows at or beyond a stream's count are
// not written, and the loops run over the counts, not the capacities.
#include "copy_words.h"
#include "ctx_internal.h"
#include "track_update.h"

namespace stvo {
namespace {

constexpr int TRACK_BLOCK = 256;

static_assert(sizeof(stvo_track) == sizeof(unsigned long long), "a track record is stored as one 8-byte word");
static_assert(sizeof(stvo_kf_header) == sizeof(int4), "the key-frame header is stored as one 16-byte word");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(TRACK_BLOCK) void track_update_kernel(TrackArgs a) {
    __shared__ int win_p[STVO_POSE_MAX_POINTS];
    __shared__ int win_l[STVO_POSE_MAX_LINES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t op = (size_t)b * a.K, ol = (size_t)b * a.M;
    const int c = a.ctl ? a.ctl[b] : STVO_STREAM_RUN;
    const int mode = (a.first || c == STVO_STREAM_RESTART) ? trk::MODE_INIT : (c == STVO_STREAM_PARK ? trk::MODE_PARK : trk::MODE_RUN);
    const int n = clampi(a.n_cur[b], a.K), nl = clampi(a.nl_cur[b], a.M);
    const bool reset = trk::track_resets(mode, (a.traj && mode == trk::MODE_RUN) ? a.traj[b].new_kf : 0);
    if (mode == trk::MODE_RUN) {
        const int n1 = clampi(a.n_prev[b], a.K), nl1 = clampi(a.nl_prev[b], a.M);
        trk::track_clear(win_p, n, tid, TRACK_BLOCK);
        trk::track_clear(win_l, nl, tid, TRACK_BLOCK);
        __syncthreads();
        trk::track_vote(win_p, a.m12p + op, n1, n, tid, TRACK_BLOCK);
        trk::track_vote(win_l, a.m12l + ol, nl1, nl, tid, TRACK_BLOCK);
        __syncthreads();
    }
    typedef unsigned long long u64;
    trk::track_write(win_p, a.inlp ? a.inlp + op : nullptr, reinterpret_cast<const u64*>(a.prev_p + op), n, mode, reset,
                     reinterpret_cast<u64*>(a.rec_p + op), reinterpret_cast<u64*>(a.next_p + op), tid, TRACK_BLOCK);
    trk::track_write(win_l, a.inll ? a.inll + ol : nullptr, reinterpret_cast<const u64*>(a.prev_l + ol), nl, mode, reset,
                     reinterpret_cast<u64*>(a.rec_l + ol), reinterpret_cast<u64*>(a.next_l + ol), tid, TRACK_BLOCK);
    if (tid == 0) *reinterpret_cast<int2*>(a.rec_counts + 2 * (size_t)b) = make_int2(n, nl);
    if (!a.kf_hdr || !reset) return;
    // the key-frame set: rows [0, n) of every array, byte for byte, then the header
    copy_words<uint4, TRACK_BLOCK>(a.cur.rc, a.kf.rc, op, n, tid);
    copy_words<uint4, TRACK_BLOCK>(a.cur.desc, a.kf.desc, op * 2, n * 2, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.spl, a.kf.spl, ol * 2, nl * 2, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.epl, a.kf.epl, ol * 2, nl * 2, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.sP, a.kf.sP, ol * 3, nl * 3, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.eP, a.kf.eP, ol * 3, nl * 3, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.le, a.kf.le, ol * 3, nl * 3, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.s2l, a.kf.s2l, ol, nl, tid);
    copy_words<u64, TRACK_BLOCK>(a.cur.s2lm, a.kf.s2lm, ol, nl, tid);
    copy_words<uint4, TRACK_BLOCK>(a.cur.ldesc, a.kf.ldesc, ol * 2, nl * 2, tid);
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int serial = mode == trk::MODE_INIT ? 1 : a.kf_hdr[b].serial + 1;
        *reinterpret_cast<int4*>(a.kf_hdr + b) = make_int4(n, nl, a.frame, serial);
    }
}

}  // namespace

void launch_track_update(hipStream_t s, const TrackArgs& a) {
    hipLaunchKernelGGL(track_update_kernel, dim3(a.B), dim3(TRACK_BLOCK), 0, s, a);
}

}  // namespace stvo
