// chaincheck.hip — TEST INFRASTRUCTURE (tests/test_gpu_chain_exceptions.py):
// runs the library's own verify dispatch over digests the TEST supplies, so
// that a valid signature can be made for chosen u1, u2 (tests/chain_vectors.py:
// the digest is e = u1 s, which no message hashes to).  Nothing of the library
// changes and no message is read: the bulk entry is verify_device_impl
// (bv_api.cpp) with the digests copied into the slot's buffer and
// bv_run_device told they are there (`hashed`); the host-order entry runs
// bv_host_launch's call sequence (bv_run_keys, bv_item_pipe: k_verify_qf, then
// k_verify_gf chunk by chunk) over the same resident batch; the small entries
// are bvk::verify_small launches over the test's own device buffers, the
// device forming every scalar or, as bv_small_verify does for a latency batch,
// reading them from bv_host_item_records' records.
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

// The host entries' order over a batch already in HBM.  Shaped as bulk_impl
// (slot begin, key-cache prepare, the digests copied into the slot's buffer),
// but on ctx->stream, where bv_host_launch runs (bv_item_pipe::key_part
// expects bv_kc_prepare's work there), and in place of bv_run_device the call
// sequence of bv_host_launch: bv_run_keys without the s^-1 stream's GLV split,
// the context's own output buffers with `hashed` digests, the key part of
// every item on the s^-1 stream, then the items in chunks [done, end) for each
// of `ends` and the rest.  tests/test_chain_exceptions.py compares that
// sequence with bv_host_launch's.  *qf: whether the key part ran first
// (k_verify_qf, then k_verify_gf per chunk); otherwise the pipe ran the device
// order chunk by chunk.  The results are copied to dresult's buffers.
int hostorder_impl(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult, const uint8_t *d_digests, hipStream_t st,
                   uint32_t n_ends, const uint64_t *ends, bool *qf) {
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
  const uint64_t n_msgs = dbatch->n_msgs, n_items = dbatch->n_items;
  HIPCHK(ctx->S().digests.ensure((n_msgs ? n_msgs : 1) * 32), BV_E_OOM, "alloc digests");
  if (n_msgs)
    HIPCHK(hipMemcpyAsync(ctx->S().digests.p, d_digests, n_msgs * 32, hipMemcpyDeviceToDevice, st), BV_E_LAUNCH,
           "copy digests");
  // the batch is resident: one event stands for the keys, s and the item arrays
  hipEvent_t resident = ctx->S().ev[E_READY];
  HIPCHK(hipEventRecord(resident, st), BV_E_LAUNCH, "event");
  int rc = bv_run_keys(ctx, dbatch, resident, resident, kc, false);
  if (rc != BV_OK) return rc;
  bv_item_pipe pipe{ctx, dbatch, {}, st, kc};
  rc = bv_out_bufs(ctx, dbatch, nullptr, nullptr, nullptr, true, &pipe.o);
  if (rc != BV_OK) return rc;
  rc = pipe.key_part(ctx->sstream, resident);
  if (rc != BV_OK) return rc;
  for (uint32_t k = 0; k < n_ends; k++) {
    rc = pipe.upto(ends[k]);
    if (rc != BV_OK) return rc;
  }
  rc = pipe.finish();
  if (rc != BV_OK) return rc;
  *qf = pipe.qf;
  if (dresult->msg_hash && n_msgs)
    HIPCHK(hipMemcpyAsync(dresult->msg_hash, pipe.o.dig, n_msgs * 32, hipMemcpyDeviceToDevice, st), BV_E_LAUNCH,
           "copy digests out");
  if (dresult->status && n_items)
    HIPCHK(hipMemcpyAsync(dresult->status, pipe.o.status, n_items, hipMemcpyDeviceToDevice, st), BV_E_LAUNCH,
           "copy statuses out");
  if (dresult->accept_bits && n_items)
    HIPCHK(hipMemcpyAsync(dresult->accept_bits, pipe.o.bits, (n_items + 63) / 64 * 8, hipMemcpyDeviceToDevice, st),
           BV_E_LAUNCH, "copy bits out");
  return BV_OK;
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

// Bulk entry in the host entries' order (hostorder_impl): as cc_verify_bulk,
// with the items launched in chunks ending at ends[0 .. n_ends) (ascending
// multiples of 64, at most n_items) and at n_items.  *qf = 1 when the key part
// ran first (k_verify_qf + k_verify_gf), 0 when the context runs the device
// order here too (BV_QFIRST=0, or no key table).
int cc_verify_hostorder(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult, const uint8_t *d_digests,
                        uint32_t n_ends, const uint64_t *ends, int *qf) {
  if (!ctx || !dbatch || !dresult || !qf || (dbatch->n_msgs && !d_digests) || (n_ends && !ends)) return BV_E_ARGS;
  for (uint32_t k = 0; k < n_ends; k++)
    if (ends[k] % 64 || ends[k] > dbatch->n_items || (k && ends[k] <= ends[k - 1])) return BV_E_ARGS;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
  if (bv_wait_all(ctx) != BV_OK) return BV_E_LAUNCH;  // as bv_host_launch: the slots' buffers are free
  hipStream_t st = ctx->stream;
  ctx->last = st;
  ctx->timing = bv_timing{};
  bool ran_qf = false;
  const int rc = hostorder_impl(ctx, dbatch, dresult, d_digests, st, n_ends, ends, &ran_qf);
  if (rc != BV_OK) return bv_drain(ctx, st, rc);
  HIPCHK(hipStreamSynchronize(st), BV_E_LAUNCH, "verify sync");
  bv_read_timing(ctx);
  *qf = ran_qf ? 1 : 0;
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

// Small entry with host item records (k_small's rec != NULL form, which
// bv_small_verify takes for a latency batch): the same device arrays, and host
// copies of the digests, item arrays, r and s, from which bv_host_item_records
// forms one record per item (u1, k1, k2 on the host) in mapped host memory,
// with the key-cache lookup's table addresses when kc_tabs.  A launch takes at
// most as many items as the product would give records: ctx->host_scalar_max
// when every item's key has a table, else 4; the items go in slices of that
// size, each slice's records made by one call and the launches synchronised
// one by one, stopping at the first error.  *launches: how many there were.
int cc_verify_small_rec(bv_ctx *ctx, uint32_t n_items, uint32_t n_keys, const uint8_t *d_digests,
                        const uint8_t *d_key_bytes, const uint64_t *d_key_off, const uint32_t *d_item_msg,
                        const uint32_t *d_item_key, const uint8_t *d_r, const uint8_t *d_s, int kc_tabs,
                        const uint8_t *h_key_bytes, const uint64_t *h_key_off, const uint8_t *h_digests,
                        const uint32_t *h_item_msg, const uint32_t *h_item_key, const uint8_t *h_r,
                        const uint8_t *h_s, uint8_t *d_status, uint32_t *hits, uint32_t *launches) {
  if (!ctx || n_items == 0 || n_items > 1024 || n_keys == 0 || !h_key_bytes || !h_key_off || !h_digests ||
      !h_item_msg || !h_item_key || !h_r || !h_s || !d_status)
    return BV_E_ARGS;
  for (uint32_t i = 0; i < n_items; i++)
    if (h_item_key[i] >= n_keys) return BV_E_ARGS;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
  if (bv_wait_all(ctx) != BV_OK) return BV_E_LAUNCH;
  hipStream_t st = ctx->stream;
  std::vector<uint64_t> tabs(n_keys, 0);
  uint32_t h = 0, n_launch = 0;
  if (kc_tabs) h = bv_kc_lookup(ctx, n_keys, h_key_bytes, h_key_off, tabs.data());
  // bv_small_verify's rule for records
  bool all_tabs = kc_tabs != 0;
  for (uint32_t i = 0; i < n_items && all_tabs; i++) all_tabs = tabs[h_item_key[i]] != 0;
  const uint32_t per = all_tabs ? ctx->host_scalar_max : std::min<uint32_t>(4, ctx->host_scalar_max);
  if (per == 0) return bv_fail(ctx, BV_E_ARGS, "host item records are switched off (BV_HOST_SCALARS=0)");
  std::vector<HostRecItem> items(n_items);
  for (uint32_t i = 0; i < n_items; i++) {
    const uint32_t k = h_item_key[i];
    items[i] = {h_digests + 32ull * h_item_msg[i], h_r + 32ull * i, h_s + 32ull * i, h_key_bytes + h_key_off[k],
                h_key_off[k + 1] - h_key_off[k], tabs[k], 0};
  }
  // records and clock words in mapped host memory, as bv_small_verify lays them out in its one buffer
  uint32_t *rec = nullptr, *d_rec = nullptr;
  uint64_t *clk = nullptr, *d_clk = nullptr;
  int rc = BV_OK;
  constexpr unsigned kMapped = hipHostMallocMapped | hipHostMallocCoherent;
  hipError_t e = hipHostMalloc((void **)&rec, (size_t)n_items * hrec::kWords * 4, kMapped);
  if (e == hipSuccess) e = hipHostMalloc((void **)&clk, (n_items + 1) * 8ull, kMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d_rec, rec, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d_clk, clk, 0);
  if (e == hipSuccess)
    for (uint32_t i = 0; i <= n_items; i++) clk[i] = 0;
  for (uint32_t lo = 0; lo < n_items && e == hipSuccess; lo += per) {
    const uint32_t cnt = std::min(per, n_items - lo);
    bv_host_item_records(rec + (size_t)hrec::kWords * lo, items.data() + lo, cnt);
    // block b of this launch is item lo + b: its record, status byte and end clock (clk[lo + 1 + b])
    e = bvk::verify_small(st, ctx->kc_w, cnt, d_digests, d_key_bytes, d_key_off, d_item_msg + lo, d_item_key + lo,
                          d_r + 32ull * lo, d_s + 32ull * lo, nullptr, nullptr, ctx->g_table, d_status + lo, nullptr,
                          d_rec + (size_t)hrec::kWords * lo, d_clk + lo);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    n_launch++;
  }
  if (e != hipSuccess) rc = bv_fail(ctx, BV_E_LAUNCH, "k_small with records (chaincheck)", e);
  if (rec) (void)hipHostFree(rec);
  if (clk) (void)hipHostFree(clk);
  if (hits) *hits = h;
  if (launches) *launches = n_launch;
  return rc;
}

}  // extern "C"
