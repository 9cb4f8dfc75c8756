// blk_kernels.hip — gfx950 kernels of bv_verify_blocks (bv_blocks.cpp drives
// them): BlockBody JSON built from the blocks' fields and hashed
// as it is built, and CheckBlock's tally per block; for a shard of
// bv_group_verify_blocks, the same over the shard's slices (k_blk_body_hash_rb)
// and its items' block indices less its first block (k_blk_item_rebase).  A
// translation unit of its
// own, so that the code object of kernels.hip (the verify kernels) is the
// same with and without this entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blkjson.h"
#include "bv_internal.h"

// BlockBody JSON serialised straight into SHA-256, one lane per block, as
// k_ev_body_hash does for events: the chaining value and the current block in
// a 25-word LDS row per lane, no body, length or offset array in HBM.  A
// block body is ~25 SHA blocks (16 x 64-B transactions) against an event's
// ~8 and a batch has 100 x fewer of them than items, so the lanes are few and
// heavy: NT lanes per workgroup spread 10,000 blocks over 157 (NT = 64) or 40
// (NT = 256) workgroups of a 256-CU part (bvk::blk_body_hash picks; DESIGN
// §11).  Blocks listed in long_idx (sorted; bodies longer than kHostHashLen,
// hashed by the host and put in by k_put_digests) are left alone.
#define BLK_ROW 25
template <int NT>
__global__ void __launch_bounds__(NT) k_blk_body_hash(bv_block_batch b, uint64_t b0, uint64_t b1,
                                                      const uint64_t *__restrict__ long_idx, uint64_t n_long,
                                                      uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[NT * BLK_ROW];
  const uint64_t k = b0 + (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= b1) return;  // no barriers below
  uint64_t lo = 0, hi = n_long;  // is k a long block?
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (long_idx[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n_long && long_idx[lo] == k) return;
  EvjSha o = evj_sha_begin(rows + threadIdx.x * BLK_ROW);
  blk_emit(b, k, o);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * k);
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// The same over a shard (bv_group_verify_blocks): `b` holds the slices of
// blocks [bs.blk, ...) of a larger batch, [b0, b1) are that batch's block
// indices, and `dig` and `long_idx` are the shard's: block k's digest is row
// k - bs.blk, which is also how the long blocks are listed (k_put_digests
// writes their rows of the same array).
template <int NT>
__global__ void __launch_bounds__(NT) k_blk_body_hash_rb(bv_block_batch b, uint64_t b0, uint64_t b1,
                                                         const uint64_t *__restrict__ long_idx, uint64_t n_long,
                                                         BlkBases bs, uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[NT * BLK_ROW];
  const uint64_t k = b0 + (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= b1) return;  // no barriers below
  const uint64_t row = k - bs.blk;
  uint64_t lo = 0, hi = n_long;  // is k a long block?
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (long_idx[mid] < row) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n_long && long_idx[lo] == row) return;
  EvjSha o = evj_sha_begin(rows + threadIdx.x * BLK_ROW);
  blk_emit(b, k, o, bs);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * row);
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// A shard's items name blocks of the whole batch; its digest and count arrays
// are its own.  One lane per item: out[i] = item_block[i] - block_base, the
// index the verify kernels and k_blk_tally use.
__global__ void __launch_bounds__(256) k_blk_item_rebase(uint64_t n, const uint32_t *__restrict__ item_block,
                                                         uint32_t block_base, uint32_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = item_block[i] - block_base;
}

// CheckBlock's tally: count[b] += the ACCEPT items of block b, one lane per
// item (count zeroed by the caller).  Items of one block usually lie next to
// each other (100 signatures per block), so each wave first sums every run
// of equal block indices among its 64 lanes from one ballot and the run's
// first lane issues ONE atomicAdd for it; items in any order stay correct
// (their runs are one lane long).  Lanes past n form empty runs.
__global__ void __launch_bounds__(256) k_blk_tally(uint64_t n, const uint32_t *__restrict__ item_block,
                                                   const uint8_t *__restrict__ status,
                                                   uint32_t *__restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t blk = i < n ? item_block[i] : 0xFFFFFFFFu;
  const bool acc = i < n && status[i] == BV_ACCEPT;
  const uint32_t prev = __shfl_up(blk, 1, 64);
  const bool head = lane == 0 || prev != blk;
  const uint64_t heads = __ballot(head), accs = __ballot(acc);
  if (!head) return;
  const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);  // the next run's head, if any
  const uint32_t len = above ? (uint32_t)__ffsll((unsigned long long)above) : 64 - lane;
  const uint64_t run = (len == 64 ? ~0ull : (1ull << len) - 1) << lane;
  const uint32_t c = (uint32_t)__popcll(accs & run);
  if (c) atomicAdd(count + blk, c);
}

namespace bvk {
static inline dim3 grid1(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }

// nt: lanes per workgroup, 64 or 256 (0: the default, BLK_NT_DEFAULT); any
// other value is hipErrorInvalidValue
#define BLK_NT_DEFAULT 64
hipError_t blk_body_hash(hipStream_t st, const bv_block_batch &b, uint64_t b0, uint64_t b1, const uint64_t *long_idx,
                         uint64_t n_long, uint32_t *dig, int nt) {
  if (b1 <= b0) return hipSuccess;
  if (nt == 0) nt = BLK_NT_DEFAULT;
  if (nt == 64)
    hipLaunchKernelGGL(k_blk_body_hash<64>, grid1(b1 - b0, 64), dim3(64), 0, st, b, b0, b1, long_idx, n_long, dig);
  else if (nt == 256)
    hipLaunchKernelGGL(k_blk_body_hash<256>, grid1(b1 - b0, 256), dim3(256), 0, st, b, b0, b1, long_idx, n_long, dig);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t blk_body_hash_rb(hipStream_t st, const bv_block_batch &b, uint64_t b0, uint64_t b1,
                            const uint64_t *long_idx, uint64_t n_long, const BlkBases &bs, uint32_t *dig, int nt) {
  if (b1 <= b0) return hipSuccess;
  if (nt == 0) nt = BLK_NT_DEFAULT;
  if (nt == 64)
    hipLaunchKernelGGL(k_blk_body_hash_rb<64>, grid1(b1 - b0, 64), dim3(64), 0, st, b, b0, b1, long_idx, n_long, bs,
                       dig);
  else if (nt == 256)
    hipLaunchKernelGGL(k_blk_body_hash_rb<256>, grid1(b1 - b0, 256), dim3(256), 0, st, b, b0, b1, long_idx, n_long,
                       bs, dig);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t blk_item_rebase(hipStream_t st, uint64_t n_items, const uint32_t *item_block, uint32_t block_base,
                           uint32_t *out) {
  if (n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(k_blk_item_rebase, grid1(n_items, 256), dim3(256), 0, st, n_items, item_block, block_base, out);
  return hipGetLastError();
}

hipError_t blk_tally(hipStream_t st, uint64_t n_items, const uint32_t *item_block, const uint8_t *status,
                     uint32_t *count) {
  if (n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(k_blk_tally, grid1(n_items, 256), dim3(256), 0, st, n_items, item_block, status, count);
  return hipGetLastError();
}
}  // namespace bvk
