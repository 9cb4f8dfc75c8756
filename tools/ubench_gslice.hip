// Where k_verify_g's lost issue slots go ("lookups one window
// ahead"): the u1 G loop of verify_core.h (g_table_add: 10 signed 26-bit
// windows, XYZZ mixed additions, 256-thread blocks at 4 waves per SIMD) over
//   hbm: the whole 21.5 GB table — every gather an HBM and TLB miss, as in
//        the product;
//   l2:  the same digits with the entry index masked into a 2 MB slice, so
//        every gather hits L2;
// each with the load-then-add loop (the gather in front of the addition) and
// with the lookup requested one window ahead into LDS (entry_stage).
// Timing only: the table holds arbitrary field elements (the addition costs
// the same for any operands off its exceptional branches) and the results
// are meaningless; nothing is compared.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/ubench_gslice.hip -o tools/ubench_gslice
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../babble_amd/csrc/verify_core.h"

#define CHK(x)                                       \
  do {                                               \
    hipError_t e_ = (x);                             \
    if (e_ != hipSuccess) {                          \
      printf("%s: %s\n", #x, hipGetErrorString(e_)); \
      return 1;                                      \
    }                                                \
  } while (0)

__device__ uint32_t mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  return x ^ (x >> 16);
}

__global__ void k_fill(uint32_t *t, uint64_t n_u32) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_u32; i += (uint64_t)gridDim.x * blockDim.x)
    t[i] = mix((uint32_t)i ^ (uint32_t)(i >> 32) * 0x9E3779B9u) & 0x7FFFFFFFu;  // limbs < p: canonical entries
}

constexpr uint32_t kEnt = 1u << (BV_GW - 1);
constexpr uint64_t kEntries = (uint64_t)BV_GNWIN * kEnt + 1;

// g_table_add<BV_GW, BV_GNWIN, false, gexz, true>'s two loop forms with the
// entry index ANDed with `mask` (all ones: the product's addresses; every
// masked index is below kEntries)
template <bool PIPE>
__global__ void __launch_bounds__(256, 4) k_ug(const uint32_t *__restrict__ tab, uint64_t n_items, uint64_t mask,
                                               uint32_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  uint32_t u[8];
  for (int k = 0; k < 8; k++) u[k] = mix((uint32_t)i * 8 + k);
  u[7] &= 0x7FFFFFFFu;
  gexz R;
  bool inf = true;
  fe_set(R.X, 0);
  fe_set(R.Y, 0);
  fe_set(R.ZZ, 0);
  fe_set(R.ZZZ, 0);
  uint32_t carry = 0;
  if (PIPE) {
    entry_stage stage;
    bool dneg;
    uint32_t d = next_digit<BV_GW, 8, true>(u, carry, dneg);
    stage.request(tab + ((uint64_t)d & mask) * BV_ENTRY_U32);
#pragma unroll 1
    for (int j = 0; j < BV_GNWIN; j++) {
      fe x, y;
      stage.take(x, y);
      const uint32_t dj = d;
      const bool nj = dneg;
      if (j + 1 < BV_GNWIN) {
        d = next_digit<BV_GW, 8, true>(u, carry, dneg);
        stage.request(tab + (((uint64_t)(j + 1) * kEnt + d) & mask) * BV_ENTRY_U32);
      }
      fe_cneg_canon(y, nj);
      if (j == 1 && !inf) {
        if (dj != 0) gexz_add_ge_aff<false>(R, inf, x, y);
        continue;
      }
      pt_add_ge_step<false>(R, inf, x, y, dj != 0);
    }
  } else {
    for (int j = 0; j < BV_GNWIN; j++) {
      bool dneg;
      const uint32_t d = next_digit<BV_GW, 8, true>(u, carry, dneg);
      const uint32_t *e = tab + (((uint64_t)j * kEnt + d) & mask) * BV_ENTRY_U32;
      fe x, y;
      fe_load4(x, e);
      fe_load4(y, e + 8);
      fe_cneg_canon(y, dneg);
      if (j == 1 && !inf) {
        if (d != 0) gexz_add_ge_aff<false>(R, inf, x, y);
        continue;
      }
      pt_add_ge_step<false>(R, inf, x, y, d != 0);
    }
  }
  uint32_t h = 0;
  for (int k = 0; k < 8; k++) h ^= R.X.v[k] ^ R.Y.v[k] ^ R.ZZ.v[k] ^ R.ZZZ.v[k];
  if (h == 0x12345678u) out[0] = (uint32_t)i;
}

template <bool PIPE>
int run(const char *name, const uint32_t *tab, uint64_t n_items, uint64_t mask, uint32_t *out, float *best) {
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0));
  CHK(hipEventCreate(&e1));
  const dim3 grid((unsigned)((n_items + 255) / 256));
  float ms[7];
  for (int r = 0; r < 7; r++) {  // run 0 warms up
    CHK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_ug<PIPE>, grid, dim3(256), 0, 0, tab, n_items, mask, out);
    CHK(hipEventRecord(e1));
    CHK(hipEventSynchronize(e1));
    CHK(hipGetLastError());
    CHK(hipEventElapsedTime(&ms[r], e0, e1));
  }
  std::sort(ms + 1, ms + 7);
  *best = ms[1];
  printf("  %-22s min %.4f ms  median %.4f ms  max %.4f ms\n", name, ms[1], (ms[3] + ms[4]) / 2, ms[6]);
  return 0;
}

int main() {
  const uint64_t n_items = 1000000;
  uint32_t *tab, *out;
  CHK(hipMalloc(&tab, kEntries * BV_ENTRY_U32 * 4));
  CHK(hipMalloc(&out, 64));
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, tab, kEntries * BV_ENTRY_U32);
  CHK(hipDeviceSynchronize());
  const uint64_t all = ~0ull, slice = (2u << 20) / 64 - 1;  // 32,768 entries = 2 MB
  float t[4];
  printf("u1 G loop, 1M items, 6 timed launches each:\n");
  if (run<false>("hbm, load-then-add", tab, n_items, all, out, &t[0])) return 1;
  if (run<false>("l2,  load-then-add", tab, n_items, slice, out, &t[1])) return 1;
  if (run<true>("hbm, one window ahead", tab, n_items, all, out, &t[2])) return 1;
  if (run<true>("l2,  one window ahead", tab, n_items, slice, out, &t[3])) return 1;
  printf("gather share of the load-then-add loop: %.1f %%; of the pipelined loop: %.1f %%\n",
         100 * (t[0] - t[1]) / t[0], 100 * (t[2] - t[3]) / t[2]);
  return 0;
}
