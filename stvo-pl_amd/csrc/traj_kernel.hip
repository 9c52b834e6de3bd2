// traj_kernel.hip — trajectory and key-frame decision for B streams on the device: one lane per stream reads the pose result its stream's
// step left behind and advances the stream's stvo_traj_state by pm::traj_update (traj_update.h: the Tfw / Tfw_cov composition of
// optimizePose's "set estimated pose" block, then needNewKF / currFrameIsKF), the text the host mirror and the CPU tests run.
// Nothing of it passes through the host.
#include "ctx_internal.h"
#include "traj_update.h"

namespace stvo {
namespace {

__global__ __launch_bounds__(64) void traj_init_kernel(int B, stvo_traj_state* __restrict__ state) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    pm::traj_init(state[b]);
}

static_assert(sizeof(stvo_traj_record) % sizeof(unsigned long long) == 0, "a record is zeroed in 8-byte words");

__global__ __launch_bounds__(64) void traj_update_kernel(int B, const stvo_pose_result* __restrict__ results, stvo_traj_params prm,
                                                         stvo_traj_state* __restrict__ state, stvo_traj_record* __restrict__ records) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const stvo_pose_result& r = results[b];
    pm::traj_update(state[b], r.T, r.cov, r.status, prm, records ? records + b : nullptr);
}

// behind a step that carried a control (stvo_seq_control_next_step): `initialize` for the RESTART streams, nothing for the parked ones
__global__ __launch_bounds__(64) void traj_update_ctl_kernel(int B, const stvo_pose_result* __restrict__ results, stvo_traj_params prm,
                                                             stvo_traj_state* __restrict__ state, stvo_traj_record* __restrict__ records,
                                                             const int32_t* __restrict__ ctl) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int c = ctl[b];
    if (c == STVO_STREAM_RUN) {
        const stvo_pose_result& r = results[b];
        pm::traj_update(state[b], r.T, r.cov, r.status, prm, records ? records + b : nullptr);
        return;
    }
    if (c == STVO_STREAM_RESTART) pm::traj_init(state[b]);
    if (records) {  // frame == 0: no pose in this step
        unsigned long long* w = reinterpret_cast<unsigned long long*>(records + b);
        for (int i = 0; i < (int)(sizeof(stvo_traj_record) / sizeof(unsigned long long)); ++i) w[i] = 0ull;
    }
}

}  // namespace

void launch_traj_init(hipStream_t s, int B, stvo_traj_state* state) {
    hipLaunchKernelGGL(traj_init_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, state);
}

void launch_traj_update(hipStream_t s, int B, const stvo_pose_result* results, const stvo_traj_params& prm, stvo_traj_state* state,
                        stvo_traj_record* records, const int32_t* ctl) {
    if (ctl)
        hipLaunchKernelGGL(traj_update_ctl_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, results, prm, state, records, ctl);
    else
        hipLaunchKernelGGL(traj_update_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, results, prm, state, records);
}

}  // namespace stvo

extern "C" int stvo_traj_init_dev(stvo_ctx* ctx, int B, stvo_traj_state* state_dev) {
    if (!ctx || B <= 0 || !state_dev) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::launch_traj_init(ctx->stream, B, state_dev);
    return check_launch(ctx);
}

extern "C" int stvo_traj_update_dev(stvo_ctx* ctx, int B, const stvo_pose_result* results_dev, const stvo_traj_params* prm,
                                    stvo_traj_state* state_dev, stvo_traj_record* records_dev) {
    if (!ctx || B <= 0 || !results_dev || !prm || !state_dev) return STVO_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stvo::launch_traj_update(ctx->stream, B, results_dev, *prm, state_dev, records_dev);
    return check_launch(ctx);
}
