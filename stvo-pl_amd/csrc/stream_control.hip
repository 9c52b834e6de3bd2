// stream_control.hip — the per-stream control word of the device-resident pipeline (stvo_seq_control_next_step): what a step does for the
// streams that RESTART (the frame in the slot is the first of a new sequence: StereoFrameHandler::initialize,
// the reference's src/stereoFrameHandler.cpp:35-52) or are PARKED (no sequence at the moment).  Two kernels around the frame-to-frame stage
// and one in front of the detection:
//   stream_ctl_pre_kernel    in front of the f2f stage: the stream presents NO previous features — the counts of its previous stereo set
//                            become 0 (that set is dead after this step) and its rows of the f2f match indices -1 — so that the matchers
//                            and the pose kernel take their existing path for an empty previous set;
//   stream_ctl_post_kernel   behind the pose kernel, where the result was written (device memory or the pinned zero-copy block): the
//                            stream's result record becomes all-zero bytes (what stvo_seq_read reports for a first frame), its motion-model
//                            seed the identity (prev_frame->DT = I, :45) and its inlier rows -1;
//   fast_restart_kernel      th[b] = th0 for the RESTART streams (:38 precedes the detection of :41-42);
//   cam_restart_kernel       cams[b], inv_wh[b] (and the image size a snapshot header carries) of the RESTART streams become those of the
//                            new sequence's dataset (app/imagesStVO.cpp:66 builds one PinholeStereoCamera per dataset), in front of the step.
// One wave per stream, four streams per workgroup; a wave whose stream RUNs reads its control word and leaves.  No barrier, plain
// vector stores.
#include "ctx_internal.h"

namespace stvo {
namespace {

constexpr int CTL_WAVES = 4;

__device__ __forceinline__ void fill_i32(int32_t* __restrict__ p, int n, int32_t v, int lane) {
    for (int i = lane; i < n; i += 64) p[i] = v;
}

__global__ __launch_bounds__(64 * CTL_WAVES) void stream_ctl_pre_kernel(int B, const int32_t* __restrict__ ctl, int32_t* __restrict__ n_prev,
                                                                        int32_t* __restrict__ nl_prev, int32_t* __restrict__ m12p, int K,
                                                                        int32_t* __restrict__ m12l, int M) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * CTL_WAVES + (threadIdx.x >> 6);
    if (b >= B || ctl[b] == STVO_STREAM_RUN) return;
    if (lane == 0) {
        n_prev[b] = 0;
        nl_prev[b] = 0;
    }
    fill_i32(m12p + (size_t)b * K, K, -1, lane);
    fill_i32(m12l + (size_t)b * M, M, -1, lane);
}

__global__ __launch_bounds__(64 * CTL_WAVES) void stream_ctl_post_kernel(int B, const int32_t* __restrict__ ctl, stvo_pose_result* __restrict__ results,
                                                                         double* __restrict__ motion_T, int32_t* __restrict__ inl_p, int K,
                                                                         int32_t* __restrict__ inl_l, int M) {
    static_assert(sizeof(stvo_pose_result) % sizeof(unsigned long long) == 0, "the record is zeroed in 8-byte words");
    const int lane = threadIdx.x & 63, b = blockIdx.x * CTL_WAVES + (threadIdx.x >> 6);
    if (b >= B || ctl[b] == STVO_STREAM_RUN) return;
    unsigned long long* r = reinterpret_cast<unsigned long long*>(results + b);
    for (int i = lane; i < (int)(sizeof(stvo_pose_result) / sizeof(unsigned long long)); i += 64) r[i] = 0ull;
    if (motion_T && lane < 16) motion_T[(size_t)b * 16 + lane] = (lane % 5 == 0) ? 1.0 : 0.0;
    if (inl_p) fill_i32(inl_p + (size_t)b * K, K, -1, lane);
    if (inl_l) fill_i32(inl_l + (size_t)b * M, M, -1, lane);
}

__global__ __launch_bounds__(64) void fast_restart_kernel(int B, const int32_t* __restrict__ ctl, int32_t* __restrict__ th, int th0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (ctl[b] == STVO_STREAM_RESTART) th[b] = th0;
}

__global__ __launch_bounds__(64) void cam_restart_kernel(int B, const int32_t* __restrict__ ctl, const CamRestart* __restrict__ upd,
                                                         stvo_cam* __restrict__ cams, double* __restrict__ inv_wh, int32_t* __restrict__ snap_img) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || ctl[b] != STVO_STREAM_RESTART) return;
    const CamRestart u = upd[b];
    cams[b] = u.cam;
    inv_wh[2 * b] = u.inv_w;
    inv_wh[2 * b + 1] = u.inv_h;
    if (snap_img) {
        snap_img[2 * b] = u.cols;
        snap_img[2 * b + 1] = u.rows;
    }
}

}  // namespace

void launch_stream_ctl_pre(hipStream_t s, int B, const int32_t* ctl, int32_t* n_prev, int32_t* nl_prev, int32_t* m12p, int K, int32_t* m12l, int M) {
    hipLaunchKernelGGL(stream_ctl_pre_kernel, dim3((B + CTL_WAVES - 1) / CTL_WAVES), dim3(64 * CTL_WAVES), 0, s, B, ctl, n_prev, nl_prev, m12p, K, m12l, M);
}

void launch_stream_ctl_post(hipStream_t s, int B, const int32_t* ctl, stvo_pose_result* results, double* motion_T, int32_t* inl_p, int K,
                            int32_t* inl_l, int M) {
    hipLaunchKernelGGL(stream_ctl_post_kernel, dim3((B + CTL_WAVES - 1) / CTL_WAVES), dim3(64 * CTL_WAVES), 0, s, B, ctl, results, motion_T, inl_p, K, inl_l, M);
}

void launch_fast_restart(hipStream_t s, int B, const int32_t* ctl, int32_t* th, int th0) {
    hipLaunchKernelGGL(fast_restart_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, ctl, th, th0);
}

void launch_cam_restart(hipStream_t s, int B, const int32_t* ctl, const CamRestart* upd, stvo_cam* cams, double* inv_wh, int32_t* snap_img) {
    hipLaunchKernelGGL(cam_restart_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, ctl, upd, cams, inv_wh, snap_img);
}

}  // namespace stvo
