// sinvblockcheck.hip — TEST INFRASTRUCTURE: launches the two forms of k_sinv
// (babble_amd/csrc/sinv_kernels.h: one inversion per lane, and the block-level
// batch of BV_SINV_BLOCK) with the launcher's geometry over items supplied by
// tests/test_gpu_sinv_block.py, which compares the two w arrays word for word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../babble_amd/csrc/sinv_kernels.h"

// Host entry: n items (s as 32 big-endian bytes each, pre one byte each), M
// items per lane; w_lane and w_block get 8 little-endian u32 limbs per item.
// Both device buffers hold exactly n items.  Returns 0, or a negative HIP
// error code.  Synchronous.
extern "C" int sinvblock_run(uint64_t n, uint32_t M, const uint8_t *s_be, const uint8_t *pre, uint32_t *w_lane,
                             uint32_t *w_block) {
  if (n == 0 || M == 0) return 0;
  void *d_s = nullptr, *d_pre = nullptr, *d_w[2] = {nullptr, nullptr};
  const size_t bytes = (size_t)n * 32;
  hipError_t e = hipMalloc(&d_s, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_pre, n);
  for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipMalloc(&d_w[k], bytes);
  if (e == hipSuccess) e = hipMemcpy(d_s, s_be, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pre, pre, n, hipMemcpyHostToDevice);
  for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipMemset(d_w[k], 0xA5, bytes);
  if (e == hipSuccess) {
    const uint64_t threads = (n + M - 1) / M;
    constexpr int B = BV_SINV_THREADS;
    hipLaunchKernelGGL(k_sinv, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, n, M, (const uint32_t *)d_s,
                       (const uint8_t *)d_pre, (uint32_t *)d_w[0]);
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_sinv_block<B>, dim3((unsigned)((threads + B - 1) / B)), dim3(B), 0, 0, n, M,
                         (const uint32_t *)d_s, (const uint8_t *)d_pre, (uint32_t *)d_w[1]);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(w_lane, d_w[0], bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(w_block, d_w[1], bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_s);
  (void)hipFree(d_pre);
  for (int k = 0; k < 2; k++) (void)hipFree(d_w[k]);
  return e == hipSuccess ? 0 : -(int)e;
}
