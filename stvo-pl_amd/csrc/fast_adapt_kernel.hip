// fast_adapt_kernel.hip — the adaptive FAST threshold of StereoFrameHandler::updateFrame (/root/reference/src/stereoFrameHandler.cpp:66-86)
// for B streams on the device: one lane per stream reads the pose result its stream's step left behind and moves the threshold the next
// detection of that stream reads (orb_kernels.hip: OrbDev::th).  Nothing of it passes through the host.
#include "ctx_internal.h"

namespace stvo {
namespace {

__device__ __forceinline__ void fast_adapt_stream(const stvo_pose_result& r, const stvo_fast_adapt& p, int32_t* __restrict__ th, int b) {
    // :75 — curr_frame->DT == Matrix4d::Identity(): every element compares equal (a rejected pose is exactly I, :385)
    bool ident = true;
    for (int i = 0; i < 16; ++i) ident = ident && r.T[i] == ((i % 5 == 0) ? 1.0 : 0.0);
    const bool lost = ident || r.err > (double)p.err_th;  // err_th is a float upstream (:72): widened, not rounded again
    const int n = r.n_inliers_pt;
    int steps = 0;
    if (lost || n < p.feat_th) steps = -2;  // :76, :79
    else if (n < p.feat_th * 2) steps = -1;  // :81
    else if (n > p.feat_th * 3) steps = 1;   // :83
    else if (n > p.feat_th * 4) steps = 2;   // :85 (never reached: the row above takes every such n)
    const int cur = th[b], moved = cur + steps * p.inc_th;
    if (steps < 0) th[b] = max(p.min_th, moved);  // the clip is on the side moved towards only
    else if (steps > 0) th[b] = min(p.max_th, moved);
}

__global__ __launch_bounds__(64) void fast_adapt_kernel(int B, const stvo_pose_result* __restrict__ results, stvo_fast_adapt p, int32_t* __restrict__ th) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    fast_adapt_stream(results[b], p, th, b);
}

// behind a step that carried a control (stvo_seq_control_next_step): initialize() has no updateFrame(), and a parked stream has no frame
__global__ __launch_bounds__(64) void fast_adapt_ctl_kernel(int B, const stvo_pose_result* __restrict__ results, stvo_fast_adapt p, int32_t* __restrict__ th,
                                                            const int32_t* __restrict__ ctl) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || ctl[b] != STVO_STREAM_RUN) return;
    fast_adapt_stream(results[b], p, th, b);
}

}  // namespace

void launch_fast_adapt(hipStream_t s, int B, const stvo_pose_result* results, const stvo_fast_adapt& prm, int32_t* th, const int32_t* ctl) {
    if (ctl)
        hipLaunchKernelGGL(fast_adapt_ctl_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, results, prm, th, ctl);
    else
        hipLaunchKernelGGL(fast_adapt_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, results, prm, th);
}

}  // namespace stvo

extern "C" int stvo_fast_adapt_dev(stvo_ctx* ctx, int B, const stvo_pose_result* results_dev, const stvo_fast_adapt* prm, int32_t* th_dev) {
    if (!ctx || B <= 0 || !results_dev || !prm || !th_dev || prm->min_th > prm->max_th) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::launch_fast_adapt(ctx->stream, B, results_dev, *prm, th_dev);
    return check_launch(ctx);
}
