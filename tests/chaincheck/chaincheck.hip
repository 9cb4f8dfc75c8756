// chaincheck.hip — TEST INFRASTRUCTURE (tests/test_gpu_chain_exceptions.py):
// runs the library's own verify dispatch over digests the TEST supplies, so
// that a valid signature can be made for chosen u1, u2 (tests/chain_vectors.py:
// the digest is e = u1 s, which no message hashes to).  Nothing of the library
// changes and no message is read: the bulk entry is verify_device_impl
// (bv_api.cpp) with the digests copied into the slot's buffer and
// bv_run_device told they are there (`hashed`), the small entry one
// bvk::verify_small launch over the test's own device buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../babble_amd/csrc/bv_internal.h"

#define HIPCHK(expr, code, what)                               \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return bv_fail(ctx, code, what, _e); \
  } while (0)

namespace {

// verify_device_impl with the digests given: lock held by the caller.  Apart
// from the digest block and `hashed` this is that function's text, and
// tests/test_chain_exceptions.py compares the two, so it cannot drift.
int bulk_impl(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult, const uint8_t *d_digests, hipStream_t st) {
  bool kc = false;
  if (bv_slot_begin(ctx, st, dbatch, dresult) != BV_OK) return BV_E_LAUNCH;
  if ((ctx->flags & BV_F_KEY_CACHE) && dbatch->n_keys && dbatch->n_keys <= kKcMaxBatchKeys) {
    const uint32_t nk = dbatch->n_keys;
    std::vector<uint64_t> hko(nk + 1);
    HIPCHK(hipMemcpyAsync(hko.data(), dbatch->key_off, (nk + 1) * 8ull, hipMemcpyDeviceToHost, st), BV_E_LAUNCH,
           "d2h key_off");
    HIPCHK(bv_host_wait(ctx, st), BV_E_LAUNCH, "sync");
    if (hko[0] != 0) return bv_fail(ctx, BV_E_ARGS, "key_off[0] != 0");
    for (uint32_t k = 0; k < nk; k++)
      if (hko[k] > hko[k + 1]) return bv_fail(ctx, BV_E_ARGS, "key_off not monotone");
    std::vector<uint8_t> hkb(hko[nk] + 1);
    if (hko[nk]) {
      HIPCHK(hipMemcpyAsync(hkb.data(), dbatch->key_bytes, hko[nk], hipMemcpyDeviceToHost, st), BV_E_LAUNCH,
             "d2h key bytes");
      HIPCHK(bv_host_wait(ctx, st), BV_E_LAUNCH, "sync");
    }
    bv_kc_items items;
    items.n_items = dbatch->n_items;
    items.d_item_key = dbatch->item_key;
    int rc = bv_kc_prepare(ctx, nk, hkb.data(), hko.data(), dbatch->key_bytes, dbatch->key_off, st, &kc, false, &items);
    if (rc != BV_OK) return rc;
  }
  // the buffer bv_out_bufs hands the kernels when `hashed` (the same size: no reallocation there)
  const uint64_t n_msgs = dbatch->n_msgs;
  HIPCHK(ctx->S().digests.ensure((n_msgs ? n_msgs : 1) * 32), BV_E_OOM, "alloc digests");
  if (n_msgs)
    HIPCHK(hipMemcpyAsync(ctx->S().digests.p, d_digests, n_msgs * 32, hipMemcpyDeviceToDevice, st), BV_E_LAUNCH,
           "copy digests");
  return bv_run_device(ctx, dbatch, dresult->msg_hash, dresult->status, dresult->accept_bits, st, true, kc);
}

}  // namespace

extern "C" {

// Bulk entry.  dbatch / dresult: device pointers, as bv_verify_batch_device
// takes them; d_digests: n_msgs x 32 bytes on the device.  Synchronous; the
// context's timing (key_path) is read as after any device call.
int cc_verify_bulk(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult, const uint8_t *d_digests) {
  if (!ctx || !dbatch || !dresult || (dbatch->n_msgs && !d_digests)) return BV_E_ARGS;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
  hipStream_t st = ctx->lane[(ctx->cur + 1) % bv_ctx::kSlots];
  ctx->last = st;
  ctx->timing = bv_timing{};
  const int rc = bulk_impl(ctx, dbatch, dresult, d_digests, st);
  if (rc != BV_OK) return bv_drain(ctx, st, rc);
  HIPCHK(hipStreamSynchronize(st), BV_E_LAUNCH, "verify sync");
  bv_read_timing(ctx);
  return BV_OK;
}

// Small entry: ONE k_small launch (the device forms every scalar: no host
// item records) over device arrays of the test: digests, keys, item arrays,
// r, s, and one status byte per item out.  kc_tabs != 0: h_key_bytes /
// h_key_off (host copies of the keys) are looked up in the context's key
// cache as bv_small_verify does, and the table addresses handed to the
// kernel; *hits = keys with a table.  At most 1024 items.
int cc_verify_small(bv_ctx *ctx, uint32_t n_items, uint32_t n_keys, const uint8_t *d_digests,
                    const uint8_t *d_key_bytes, const uint64_t *d_key_off, const uint32_t *d_item_msg,
                    const uint32_t *d_item_key, const uint8_t *d_r, const uint8_t *d_s, int kc_tabs,
                    const uint8_t *h_key_bytes, const uint64_t *h_key_off, uint8_t *d_status, uint32_t *hits) {
  if (!ctx || n_items == 0 || n_items > 1024 || n_keys == 0 || (kc_tabs && (!h_key_bytes || !h_key_off)))
    return BV_E_ARGS;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
  if (bv_wait_all(ctx) != BV_OK) return BV_E_LAUNCH;
  hipStream_t st = ctx->stream;
  uint64_t *d_tabs = nullptr, *clk = nullptr, *d_clk = nullptr;
  uint32_t h = 0;
  int rc = BV_OK;
  hipError_t e = hipSuccess;
  if (kc_tabs) {
    std::vector<uint64_t> tabs(n_keys);
    h = bv_kc_lookup(ctx, n_keys, h_key_bytes, h_key_off, tabs.data());
    e = hipMalloc((void **)&d_tabs, n_keys * 8ull);
    if (e == hipSuccess) e = hipMemcpy(d_tabs, tabs.data(), n_keys * 8ull, hipMemcpyHostToDevice);
  }
  // the kernel's clock words in mapped host memory, as bv_small_verify allocates them
  if (e == hipSuccess) e = hipHostMalloc((void **)&clk, (n_items + 1) * 8ull, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) {
    for (uint32_t i = 0; i <= n_items; i++) clk[i] = 0;
    e = hipHostGetDevicePointer((void **)&d_clk, clk, 0);
  }
  if (e == hipSuccess)
    e = bvk::verify_small(st, ctx->kc_w, n_items, d_digests, d_key_bytes, d_key_off, d_item_msg, d_item_key, d_r, d_s,
                          nullptr, d_tabs, ctx->g_table, d_status, nullptr, nullptr, d_clk);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) rc = bv_fail(ctx, BV_E_LAUNCH, "k_small (chaincheck)", e);
  if (d_tabs) (void)hipFree(d_tabs);
  if (clk) (void)hipHostFree(clk);
  if (hits) *hits = h;
  return rc;
}

}  // extern "C"
