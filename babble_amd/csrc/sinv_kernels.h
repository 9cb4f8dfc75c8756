// sinv_kernels.h — the two forms of k_sinv (per-lane work in verify_core.h),
// in a header of their own so that kernels.hip and the test-only device
// library tests/sinvblock/sinvblockcheck.hip compile the same kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify_core.h"

__global__ void __launch_bounds__(256) k_sinv(uint64_t n_items, uint32_t M, const uint32_t *__restrict__ s_be,
                                              const uint8_t *__restrict__ pre, uint32_t *__restrict__ w_out) {
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  sinv_thread(t, T, n_items, M, s_be, pre, w_out);
}

// BV_SINV_BLOCK: the lanes' totals meet in LDS, the block's first wave
// inverts them as one more batch (sinv_block_lane), and every lane walks back
// from the inverse of its own total.  Every lane of the block reaches both
// barriers: a lane past the batch's end holds a Montgomery one.
template <int B>
__global__ void __launch_bounds__(B) k_sinv_block(uint64_t n_items, uint32_t M, const uint32_t *__restrict__ s_be,
                                                  const uint8_t *__restrict__ pre, uint32_t *__restrict__ w_out) {
  static_assert(B % 64 == 0 && B <= 1024, "whole waves");
  __shared__ uint32_t sh_tot[8 * B], sh_inv[8 * B];
  const uint64_t T = (uint64_t)gridDim.x * B;
  const uint64_t t = (uint64_t)blockIdx.x * B + threadIdx.x;
  sc acc;
  sinv_lane_prefix(acc, t, T, n_items, M, s_be, pre, w_out);
#pragma unroll
  for (int k = 0; k < 8; k++) sh_tot[8 * threadIdx.x + k] = acc.v[k];
  __syncthreads();
  if (threadIdx.x < 64) sinv_block_lane(threadIdx.x, 64, B, sh_tot, sh_inv);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; k++) acc.v[k] = sh_inv[8 * threadIdx.x + k];
  sinv_lane_finish(acc, t, T, n_items, M, s_be, pre, w_out);
}
