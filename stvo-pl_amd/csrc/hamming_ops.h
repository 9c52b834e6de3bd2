// hamming_ops.h — the popcount operations the Hamming kernels are built from (match_kernels.hip, grid_kernels.hip).  Device only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace stvo {

// popcount-accumulate: D = popcount(x) + acc in ONE VALU op.  Written as inline asm because the
// compiler otherwise re-associates the 8-term sum into bcnt(x,0) + v_add3 trees (22 instead of
// 19 VALU ops per pair).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
__device__ __forceinline__ uint32_t bcnt0(uint32_t x) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, 0" : "=v"(r) : "v"(x));
    return r;
}

}  // namespace stvo
