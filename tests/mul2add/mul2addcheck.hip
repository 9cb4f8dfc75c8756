// mul2addcheck.hip — TEST INFRASTRUCTURE: runs the device fe_mul2add (the
// generated gfx950 program of babble_amd/csrc/field_asm.h) over operand
// arrays supplied by tests/test_gpu_field_mul2add.py, which compares every
// result with Python integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../babble_amd/csrc/field.h"

__global__ void __launch_bounds__(256) k_mul2add(uint32_t n, const uint32_t *__restrict__ a,
                                                 const uint32_t *__restrict__ b, const uint32_t *__restrict__ x,
                                                 const uint32_t *__restrict__ y, uint32_t *__restrict__ r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe p, q, s, t, z;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    p.v[k] = a[8 * (uint64_t)i + k];
    q.v[k] = b[8 * (uint64_t)i + k];
    s.v[k] = x[8 * (uint64_t)i + k];
    t.v[k] = y[8 * (uint64_t)i + k];
  }
  fe_mul2add(z, p, q, s, t);
#pragma unroll
  for (int k = 0; k < 8; k++) r[8 * (uint64_t)i + k] = z.v[k];
}

// Host entry: n operand quadruples (8 little-endian u32 limbs each).
// Returns 0, or a negative HIP error code.  Synchronous.
extern "C" int m2a_run(uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *x, const uint32_t *y,
                       uint32_t *r) {
  const uint32_t *src[4] = {a, b, x, y};
  uint32_t *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t bytes = (size_t)(n ? n : 1) * 32;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipMalloc(&d[k], bytes);
  for (int k = 0; k < 4 && e == hipSuccess && n; k++) e = hipMemcpy(d[k], src[k], bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_mul2add, dim3((n + 255) / 256), dim3(256), 0, 0, n, d[0], d[1], d[2], d[3], d[4]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(r, d[4], bytes, hipMemcpyDeviceToHost);
  for (int k = 0; k < 5; k++) (void)hipFree(d[k]);
  return e == hipSuccess ? 0 : -(int)e;
}
