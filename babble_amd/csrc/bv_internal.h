// bv_internal.h — ctx layout and internal entry points shared by bv_api.cpp
// (single device) and bv_group.cpp (multi-device group).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <array>

#ifndef BV_SLOTS
#define BV_SLOTS 2  // work-buffer slots: device calls that may be in flight at once (3: -4 % in a same-box A/B)
#endif
#include <vector>

#include "../../include/babbleverify.h"
#include "hostscalar.h"
#include "geometry.h"
#include "hostdag.h"
#include "copypool.h"
#include "hoststage.h"

#define KS_OK 0  // k_key_decode statuses (verify_core.h)

struct EvjBases;
struct BlkBases;
struct ItxBases;
struct BsigBases;
namespace bvk {
hipError_t sha256(hipStream_t, uint64_t, const uint8_t *, const uint64_t *, uint32_t *, uint64_t max_len = ~0ull);
hipError_t put_digests(hipStream_t, uint64_t, const uint64_t *, const uint32_t *, uint32_t *);
hipError_t key_decode(hipStream_t, uint32_t, const uint8_t *, const uint64_t *, uint8_t *, uint32_t *);
hipError_t sha256_chain(hipStream_t, uint32_t, const uint8_t *, const uint64_t *, uint8_t *, uint32_t *);
hipError_t ev_body_hash(hipStream_t st, const bv_event_batch &b, uint64_t e0, uint64_t e1, uint32_t *dig);
// the same over a shard's slices (evjson.h EvjBases): [e0, e1) are the whole batch's event indices
hipError_t ev_body_hash_rb(hipStream_t st, const bv_event_batch &b, uint64_t e0, uint64_t e1, const EvjBases &bs,
                           uint32_t *dig);
// BlockBody JSON of blocks [b0, b1) built and hashed, one lane per block (blkjson.h); the blocks in long_idx
// (sorted, n_long of them; device array) are skipped.  nt: lanes per workgroup, 64 or 256 (0: the default)
hipError_t blk_body_hash(hipStream_t st, const bv_block_batch &b, uint64_t b0, uint64_t b1, const uint64_t *long_idx,
                         uint64_t n_long, uint32_t *dig, int nt = 0);
// the same over a shard's slices (blkjson.h BlkBases): [b0, b1) are the whole batch's block indices; dig and
// long_idx are the shard's (block k is row k - bs.blk of both)
hipError_t blk_body_hash_rb(hipStream_t st, const bv_block_batch &b, uint64_t b0, uint64_t b1,
                            const uint64_t *long_idx, uint64_t n_long, const BlkBases &bs, uint32_t *dig, int nt = 0);
// out[i] = item_block[i] - block_base: a shard's items over its own digest and count arrays
hipError_t blk_item_rebase(hipStream_t st, uint64_t n_items, const uint32_t *item_block, uint32_t block_base,
                           uint32_t *out);
// count[item_block[i]] += 1 for every item whose status is BV_ACCEPT (count zeroed by the caller)
hipError_t blk_tally(hipStream_t st, uint64_t n_items, const uint32_t *item_block, const uint8_t *status,
                     uint32_t *count);
// bv_verify_events_itx (itx_kernels.hip, itxjson.h; device pointers in x): InternalTransactionBody.Marshal() of
// every ITX built and hashed, one lane per ITX, ITX i's digest at message n_ev + i
hipError_t itx_body_hash(hipStream_t st, const bv_event_itx_batch &x, uint64_t n_itx, uint64_t n_ev, uint32_t *dig);
// ev_body_hash with the InternalTransactions member built from the ITXs' fields
hipError_t ev_body_hash_itx(hipStream_t st, const bv_event_itx_batch &x, uint64_t e0, uint64_t e1, uint32_t *dig);
// Event.Verify's fold over the items (item e: event e, item n_ev + i: ITX i) and the forced-panic flags
hipError_t ev_compose(hipStream_t st, uint64_t n_ev, const uint64_t *itx_start, const uint8_t *item_status,
                      const uint8_t *force_panic, uint8_t *ev_status, uint32_t *decided_by, uint64_t *bits,
                      uint8_t *itx_status);
// ev_body_hash_itx with the BlockSignatures member built from fields too (fields_kernels.hip, bsigjson.h)
hipError_t ev_body_hash_fields(hipStream_t st, const bv_event_fields_batch &f, uint64_t e0, uint64_t e1,
                               uint32_t *dig);
// the three body-hash kernels and the fold over a shard's slices (EvjBases, ItxBases, BsigBases): [e0, e1) are
// the whole batch's event indices; dig, the ITX index and every array of the fold but itx_start are the shard's
hipError_t itx_body_hash_rb(hipStream_t st, const bv_event_itx_batch &x, uint64_t n_itx, uint64_t n_ev,
                            const ItxBases &ib, uint32_t *dig);
hipError_t ev_body_hash_itx_rb(hipStream_t st, const bv_event_itx_batch &x, uint64_t e0, uint64_t e1,
                               const EvjBases &bs, const ItxBases &ib, uint32_t *dig);
hipError_t ev_body_hash_fields_rb(hipStream_t st, const bv_event_fields_batch &f, uint64_t e0, uint64_t e1,
                                  const EvjBases &bs, const ItxBases &ib, const BsigBases &sb, uint32_t *dig);
hipError_t ev_compose_rb(hipStream_t st, uint64_t n_ev, const uint64_t *itx_start, uint64_t itx_base,
                         const uint8_t *item_status, const uint8_t *force_panic, uint8_t *ev_status,
                         uint32_t *decided_by, uint64_t *bits, uint8_t *itx_status);
hipError_t iota(hipStream_t, uint64_t, uint32_t *);
hipError_t sig_decode(hipStream_t, uint64_t n, const uint64_t *off, const uint8_t *text, uint8_t *r_be, uint8_t *s_be,
                      uint8_t *pre);
// `off` holds a larger batch's offsets and `text` starts at its byte `text_base`
hipError_t sig_decode_rb(hipStream_t, uint64_t n, const uint64_t *off, const uint8_t *text, uint64_t text_base,
                         uint8_t *r_be, uint8_t *s_be, uint8_t *pre);
hipError_t build_tables(hipStream_t, int, uint32_t, const uint32_t *, const uint8_t *, uint32_t *, uint32_t *,
                        uint32_t *, uint32_t *, uint64_t n_items);
// kw: the cached geometry, 22 (KC) or 18 (KC18); any other value is hipErrorInvalidValue
hipError_t build_kc(hipStream_t, int kw, uint32_t, const uint32_t *, const uint8_t *, uint32_t *, uint32_t *,
                    uint32_t *, const uint64_t *);
size_t kc_table_bytes(int kw);  // one cached table
size_t kc_sub_bytes(int kw);    // build scratch per key: sub-tables
size_t kc_pscr_bytes(int kw);   //   and prefix products
hipError_t sinv(hipStream_t, uint64_t, uint32_t, const uint32_t *, const uint8_t *, uint32_t *);
hipError_t glv_split(hipStream_t, uint64_t n, const uint32_t *r_be, const uint32_t *w, uint32_t *u12);
// verify kernels over items [lo, hi) of an n-item batch (lo a multiple of 64)
hipError_t verify_gq(hipStream_t, int kw, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *, const uint32_t *,
                     const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                     const uint32_t *, const uint64_t *, uint8_t *, uint64_t *);
// list: n + 1 words (the deferred items' indices, then their count)
hipError_t verify_deferred(hipStream_t, uint64_t, uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                           const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                           const uint32_t *, const uint32_t *, uint8_t *, uint64_t *);
hipError_t verify_qf(hipStream_t, int, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *,
                     const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *,
                     const uint64_t *, uint32_t *);
hipError_t verify_gf(hipStream_t, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *, const uint32_t *,
                     const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                     const uint32_t *, const uint32_t *, uint8_t *, uint64_t *);
hipError_t verify_g(hipStream_t, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *, const uint32_t *,
                    const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t *,
                    const uint32_t *, uint32_t *, bool split);
hipError_t verify_q(hipStream_t, int, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *,
                    const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *,
                    const uint64_t *, const uint32_t *, uint8_t *, uint64_t *);
// kw: the geometry of kc_tabs' and the records' tables, 22 or 18
hipError_t verify_small(hipStream_t, int kw, uint32_t n_items, const uint8_t *dig, const uint8_t *key_bytes,
                        const uint64_t *key_off, const uint32_t *item_msg, const uint32_t *item_key,
                        const uint8_t *r_be, const uint8_t *s_be, const uint8_t *pre, const uint64_t *kc_tabs,
                        const uint32_t *g_table, uint8_t *status, uint64_t *stamps, const uint32_t *rec,
                        uint64_t *clk);
hipError_t verify_generic(hipStream_t, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *,
                          const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *,
                          const uint32_t *, const uint32_t *, const uint32_t *, uint8_t *, uint64_t *);
}  // namespace bvk

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes);
  void release();
  template <class T>
  T *as() const {
    return (T *)p;
  }
};

struct PinnedBuf {
  void *p = nullptr;
  size_t cap = 0;
  unsigned flags = hipHostMallocDefault;  // hipHostMalloc flags of the next allocation
  hipError_t ensure(size_t bytes);
  void release();
};

// Host entries: a message (bv_verify_batch) or block body (bv_verify_blocks)
// longer than this is hashed on the host (hostsha.cpp, the SHA extensions)
// instead of by one GPU lane — SHA-256 of one message is a serial chain,
// ~3.2 us a block on a lone lane against ~40 ns on a CPU core: the 54 KB
// anchor Frame of C5 (853 blocks) took 2.8 ms of device time on its lane
// (profiles/r04_bench_midround.json c5_fast_sync).
constexpr uint64_t kHostHashLen = 16 << 10;

// timing / ordering events (see bv_read_timing)
enum {
  E_START, E_FORK, E_SHA, E_SCALAR, E_G, E_JOINED, E_END, E_KEYS, E_SINV,
  E_CALL, E_SMALL, E_HASH0, E_STAGED, E_HASHED, E_OUT, E_CSDONE, E_READY, E_KREADY, E_SREADY, E_RREADY, E_KCTAB, E_KDEC, E_KCDEC, E_SDEC, E_COUNT
};

constexpr uint32_t kKcMaxBatchKeys = 4096;  // key cache: batches with more keys use per-batch tables

struct KcSlot {
  std::string bytes;      // raw pubkey bytes (the cache key)
  void *table = nullptr;  // KC table (valid keys only)
  uint64_t last_use = 0;
  bool free = false;
};

// The streams a context runs on are per device and per PROCESS, shared by
// every ctx of that device (refcounted): HIP maps a process's streams onto
// GPU_MAX_HW_QUEUES hardware queues (4 by default) and two streams on one
// queue serialise.  A process holds one lane per work slot (the default
// stream of that slot's calls), the s^-1 stream and the high-priority keys
// stream — 3 normal-priority queues, so the caller's own stream (or torch's
// default) still gets a queue of its own; the copy stream is created only
// when a host-entry call first needs it.
struct bv_ctx {
  int device = 0;
  uint32_t flags = 0;
  static constexpr int kSlots = BV_SLOTS;
  hipStream_t lane[kSlots] = {};  // slot k's default stream
  hipStream_t stream = nullptr;   // lane[0]: host entry points, one-launch helpers
  hipStream_t kstream = nullptr;  // per-batch key tables (high priority)
  hipStream_t sstream = nullptr;  // batched s^-1 (+ key decode)
  hipStream_t cstream = nullptr;  // host-entry copies (bv_copy_stream: created on first use)
  hipStream_t last = nullptr;     // the stream of the last device call (bv_last_stream)
  std::mutex mu;
  std::string err;
  const uint32_t *g_table = nullptr;  // process-wide, per device (gtable_acquire)
  CopyPool *pool = nullptr;
  // host-entry staging: one layout in pinned memory and in HBM
  PinnedBuf pin_in, pin_out;
  PinnedBuf small_io;  // k_small's inputs and statuses, read / written by the kernel in place (mapped, coherent)
  uint8_t *small_io_host = nullptr, *small_io_dev = nullptr;  // small_io.p (of capacity small_io_cap) and its
  size_t small_io_cap = 0;                                      // device alias
  double wall_khz = 1e5;  // the device's constant clock (hipDeviceAttributeWallClockRate)
  DevBuf d_in;
  DevBuf d_stamps;  // BV_SMALL_STAMPS: k_small phase clocks (diagnostics)
  DevBuf d_sig;     // host entries with signature text: the decoded r, s, pre (bv_sig_bufs)
  // host entry: messages longer than kHostHashLen hashed on the host (their
  // index and digest), uploaded beside the device hashing
  PinnedBuf pin_long;
  DevBuf d_long;
  // work buffers
  // Per-call work buffers in kSlots slots: device-resident calls rotate
  // through them, so a call waits only for the last user of its slot and
  // kSlots batches can be in flight, e.g. the next batch's key tables
  // building during this batch's k_verify_q when the caller alternates
  // streams.
  struct Slot {
    DevBuf digests, kstatus, kxy, bases_jac, key_sub, key_pscr, key_table, scratch, u12, rg, status, bits;
    DevBuf kc_tabs;          // key-cache table address per batch key
    PinnedBuf pin_small;     // its host staging
    bool kc_decoded = false; // bv_kc_prepare already ran k_key_decode into kstatus / kxy on the call stream
    // key cache, partial batch: a few valid keys have no table; their items
    // are left BV_DEFERRED by the KC kernels and finished by bv_run_deferred
    bool kc_partial = false;
    bool glv_split = false;  // this call's u12 was filled by k_glv_split (k_verify_g forms only u1)
    DevBuf defer;  // the deferred items' indices, then their count
    // caller result ranges [lo, hi) of this slot's device calls that the
    // other slots' calls have not yet been ordered after (deduplicated)
    std::vector<std::array<uintptr_t, 6>> uncovered;
    hipEvent_t ev[E_COUNT] = {};  // the slot's call's fork/join and timing events
    hipEvent_t done = nullptr;  // end of the last call that used this slot
    bool has_done = false;
  };
  Slot slot[kSlots];
  int cur = 0;
  Slot &S() { return slot[cur]; }
  std::vector<hipEvent_t> chunk_ev;
  hipEvent_t ev_done = nullptr;  // end of the last call's device work (both slots: bv_wait_all)
  hipEvent_t ev_host = nullptr;  // host waits on this ctx's own work on a shared lane (bv_host_wait)
  bool has_done = false;
  bool table_mode = false;
  int key_w = 0;  // 8, 12 or kc_w (key cache) in table mode
  bv_timing timing = {};
  // key cache (BV_F_KEY_CACHE, bv_keycache.cpp)
  // The ONE cached geometry of this context, fixed at bv_create: 22 (KC, 805
  // MB per key) or, with BV_F_KC_COMPACT, 18 (KC18, 67.1 MB per key).
  int kc_w = BV_KCW;
  // bv_kc_small_tables: a compact context's small batches read its KC18
  // tables (k_small<18, 8>).  Off: they run as for keys without a table.
  // A 22-bit context's always read theirs (bv_keycache.cpp kc_small_readable).
  bool kc_small_tables = false;
  uint64_t kc_table_bytes = 0, kc_sub_bytes = 0, kc_pscr_bytes = 0;  // per key, of kc_w (bv_kc_init)
  uint32_t kc_build_group = 0;  // keys per table-build launch (bounds the build scratch)
  std::unordered_map<std::string, int> kc_index;  // keys whose table build has been enqueued
  std::vector<KcSlot> kc_slots;
  std::unordered_set<std::string> kc_registered;  // bv_kc_register: the validator set
  std::unordered_map<std::string, uint32_t> kc_seen;  // valid keys without a table: batches seen (bounded)
  std::unordered_set<std::string> kc_bad;  // 65-byte 0x04 keys off the curve (bounded)
  uint32_t kc_admit = 2;                   // batches before an unregistered valid key gets a table
  bool kc_partial_on = false;              // BV_KC_PARTIAL=1: partial mode (bv_kc_prepare; off: measured slower)
  int kc_fail_alloc = 0, kc_fail_build = 0;  // fault injection (BV_KC_FAIL), tests only
  uint64_t kc_allocs = 0, kc_build_calls = 0;
  uint64_t kc_clock = 0, kc_bytes = 0, kc_budget = 0;
  DevBuf kc_kxy, kc_btabs;
  // bv_verify_events: body lengths, parent-hex positions, offsets, bodies
  DevBuf ev_iota;
  // bv_verify_blocks: valid_count on the device; the bodies a small batch builds on the host and their offsets
  DevBuf d_blk_count;
  DevBuf d_blk_item;  // a shard's item -> block indices less its first block (k_blk_item_rebase)
  std::vector<uint8_t> blk_bodies;
  std::vector<uint64_t> blk_off;
  int blk_nt = 0;  // BV_BLK_NT (A/B knob): lanes per workgroup of k_blk_body_hash, 64 or 256 (0: the default)
  HostDagScratch dag_scratch;  // in-batch DAG batches: bodies built and hashed on the host (hostdag.cpp)
  // A/B knobs, read once at bv_create (never per call): host-entry message
  // chunk (BV_HOST_CHUNK_MB, >= 1 MB), event staging chunk (BV_EV_CHUNK_MB,
  // 0 = one chunk; chunks hold >= 256 events), bulk events' verify beside the next chunk
  // (BV_EV_VERIFY_STREAM=0: on the main stream)
  // small host batches through k_small (BV_SMALL=0: the bulk pipeline);
  // host entries sum the key part of every item before the messages land
  // (BV_QFIRST=0: G part first, as device-resident batches)
  uint64_t host_msg_chunk = 64ull << 20, ev_chunk = 64ull << 20;
  bool ev_split_verify = true, small_path = true, qfirst = true;
  // host entries' digests to the host (BV_EV_D2H): 1 = one copy per hashed
  // chunk, 0 = one copy after the last chunk, 2 = bulk events only: each
  // chunk's copy by SDMA on the copy stream behind the next chunk's H2D
  // (profiles/r05_ab_ev_qfirst.log: 5.42-5.49 against 5.16-5.28 ms; stores
  // by the hashing kernel through the pinned buffer's alias: no better)
  int ev_d2h = 1;
  int ev_tail = 0;  // bulk events' chunk plan (BV_EV_TAIL): 0 equal, 1 halving, 2 equal + one small last chunk
  uint64_t table_min_items = 8;    // per-batch tables (not the generic path) from this many items per key
  uint64_t table_min_items_many = 48;  // the same above kManyKeys keys
  uint64_t k12_min_items = 8192;  // per-batch K12 (not K8) tables from this many items per key
  bool small_stamps = false;      // BV_SMALL_STAMPS=1: print k_small's phase clocks to stderr
  bool host_stamps = false;       // BV_HOST_STAMPS=1: print the host entry's phases to stderr
  bool glv_in_sstream = true;     // BV_GLV_SSTREAM (A/B): device entry's GLV split in k_glv_split
  uint32_t host_scalar_max = 16;  // BV_HOST_SCALARS: k_small batches up to this many items may get host
                                  // item records (hostscalar.h; 0: the device inverts every item)
  std::vector<HostRecItem> rec_items;  // (their inputs, reused across calls)
  uint64_t small_max = 256;       // k_small for batches of at most this many items and messages (BV_SMALL_MAX)
  uint64_t small_warm_max = 1024;  // k_small for batches whose keys are all cached (BV_SMALL_WARM_MAX)
  uint32_t lat_table_keys = 256;  // latency rule: K8 tables for batches of <= 4096 items from up to this many keys (BV_LAT_TABLE_KEYS)
};

// one in-flight host-entry call (bv_host_launch -> bv_host_finish)
struct bv_host_call {
  std::chrono::steady_clock::time_point t0;
  float ms_prep = 0;
  uint8_t *pout = nullptr;
  size_t o_st = 0, o_bits = 0;
  bool direct_in = false;                          // message bytes DMA'd from the caller's pinned buffer
  bool direct_hash = false, direct_status = false;  // results DMA'd into the caller's pinned buffers
  double h_call = -1;                               // (BV_HOST_STAMPS) host ms when E_CALL was first seen done
};
bool bv_is_pinned(const void *p, size_t n);  // [p, p+n) inside one bv_host_alloc block

int bv_fail(bv_ctx *c, int code, const char *what, hipError_t e = hipSuccess);
// in a function with a `bv_ctx *ctx` that returns a BV_ code
#define HIPCHK(expr, code, what)                               \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return bv_fail(ctx, code, what, _e); \
  } while (0)
// the context's pool as the host DAG hasher's parallel-for (hostdag.h)
inline HostParFor bv_pool_parfor(bv_ctx *ctx) {
  return [ctx](uint64_t cnt, uint64_t grain, const std::function<void(uint64_t, uint64_t)> &fn) {
    ctx->pool->parallel_for(cnt, grain, [&fn](uint64_t lo, uint64_t hi) {
      fn(lo, hi);
      return true;
    });
  };
}
hipStream_t bv_copy_stream(bv_ctx *ctx);   // the device's copy stream (created on first use; nullptr on failure)
// A staging plan's commands (hoststage.h) between ctx->pin_in and ctx->d_in,
// in order: pool copies through CopyPool::copy_many (each run of them at
// once), the DMAs on the copy stream.  bv_stage_range / bv_stage_slices plan
// layout bytes [a0, a1) / the slices of events [e0, e1) and run them;
// bv_stage_one_copy gathers every segment, pinned or not, into the staging
// block and sends the whole layout as one copy.
int bv_stage_run(bv_ctx *ctx, const std::vector<StageOp> &ops);
int bv_stage_range(bv_ctx *ctx, const StagePlan &plan, size_t a0, size_t a1, size_t piece);
int bv_stage_slices(bv_ctx *ctx, const StagePlan &plan, uint64_t e0, uint64_t e1);
int bv_stage_one_copy(bv_ctx *ctx, const StagePlan &plan);
// After a failed call: wait until nothing the call may have enqueued on the
// ctx's streams (and on `st`) is still running, so no slot keeps orphaned
// kernels that a later call would not wait for.  Returns `rc`.
int bv_drain(bv_ctx *ctx, hipStream_t st, int rc);
int bv_wait_all(bv_ctx *ctx);              // host: every call's device work has finished
int bv_mark_done(bv_ctx *ctx, hipStream_t st);
// Wait on the host for the work this ctx has enqueued on `st` so far (an
// event, not hipStreamSynchronize: the lanes are shared with other contexts)
hipError_t bv_host_wait(bv_ctx *ctx, hipStream_t st);
// Next slot for a device call writing `res`: st waits for the slot's last
// call, and for the other slot's last call when their result ranges overlap.
int bv_slot_begin(bv_ctx *ctx, hipStream_t st, const bv_batch *b, const bv_result *res);  // record the end of this call (its slot and ev_done)
// text: the items' r / s / pre come from signature text (bv_sig_text): r_be / s_be may be null
int bv_validate_host_batch(bv_ctx *ctx, const bv_batch *b, bool text = false);
// Signature text of a host-entry call (bv_verify_batch_text; bv_verify_events
// with sig_text): item i's "r|s" is text[off[i] .. off[i+1]).  Host pointers
// for bv_host_launch, device pointers for bv_run_keys.
struct bv_sig_text {
  const uint64_t *off = nullptr;
  const uint8_t *text = nullptr;
  uint64_t base = 0;  // device pointers of a shard: `off` holds the whole batch's offsets, `text` starts at this byte
};
// The decoded r, s and pre of n signatures in ctx->d_sig (device arrays).
struct bv_sig_out {
  uint8_t *r = nullptr, *s = nullptr, *pre = nullptr;
};
int bv_sig_bufs(bv_ctx *ctx, uint64_t n, bv_sig_out *out);  // (re)allocates ctx->d_sig for n signatures
// k_sig_decode on the s^-1 stream into `out` (bv_sig_bufs), then E_SDEC.  The
// caller has ordered the s^-1 stream after the text's arrival.  text_base: a
// shard's text (the offsets are the whole batch's, the text starts there).
int bv_sig_decode_launch(bv_ctx *ctx, uint64_t n, const bv_sig_text &d_sig, const bv_sig_out &out,
                         uint64_t text_base = 0);
// Both, after `text_ready` (the text in HBM), ahead of s^-1: the s^-1 stream
// decodes r, s and pre into ctx->d_sig; E_SDEC marks them written.
int bv_sig_decode_on_device(bv_ctx *ctx, uint64_t n, const uint64_t *d_off, const uint8_t *d_text,
                            hipEvent_t text_ready, bv_sig_out *out, uint64_t text_base = 0);
int bv_run_device(bv_ctx *ctx, const bv_batch *b, uint8_t *d_msg_hash, uint8_t *d_status, uint64_t *d_bits,
                  hipStream_t st, bool hashed, bool kc);
// split_ok: r is in HBM by s_ready too, so u2's GLV split may run on the
// s^-1 stream (k_glv_split) instead of in k_verify_g (the device entry)
// d_sig (device pointers; s_ready then marks the text in HBM): b's r_be / s_be
// / pre are the arrays of bv_sig_bufs and are decoded from the text on the
// s^-1 stream after the key decode, right before k_sinv
int bv_run_keys(bv_ctx *ctx, const bv_batch *b, hipEvent_t keys_ready, hipEvent_t s_ready, bool kc,
                bool split_ok = false, const bv_sig_text *d_sig = nullptr);
struct bv_out {  // device outputs of one verify
  uint32_t *dig = nullptr;
  uint8_t *status = nullptr;
  uint64_t *bits = nullptr;
};
int bv_out_bufs(bv_ctx *ctx, const bv_batch *b, uint8_t *d_msg_hash, uint8_t *d_status, uint64_t *d_bits,
                bool hashed, bv_out *o);
int bv_launch_items(bv_ctx *ctx, const bv_batch *b, const bv_out &o, hipStream_t st, bool kc, uint64_t lo,
                    uint64_t hi, int part);
// Host entry points: items verified in order on `st` as their messages get
// hashed (after bv_run_keys); upto(end) launches items [done, end), end a
// multiple of 64 or n_items.  The first launch orders `st` after s^-1 and
// the key tables.
struct bv_item_pipe {
  bv_ctx *ctx;
  const bv_batch *b;
  bv_out o;
  hipStream_t st;
  bool kc;
  bool qf = false;  // key part launched for every item (key_part): upto runs k_verify_gf
  uint64_t done = 0;
  // table mode, BV_QFIRST: R_Q of every item on `ks` after s^-1, the key
  // tables and `ready` (r and the item keys in HBM); the first upto orders
  // `st` after it.  Key cache: also after the call's kc_prepare work on
  // ctx->stream (kc_tabs), so call it right after bv_run_keys.
  int key_part(hipStream_t ks, hipEvent_t ready);
  int upto(uint64_t end);
  int finish();  // the rest, and the timing events even when there are no items
};
int bv_run_verify(bv_ctx *ctx, const bv_batch *b, uint8_t *d_msg_hash, uint8_t *d_status, uint64_t *d_bits,
                  hipStream_t st, bool hashed, bool kc);
// key cache, partial batch (kc_partial): the BV_DEFERRED items by the
// generic per-lane path, on `st` after the call's last verify kernel
int bv_run_deferred(bv_ctx *ctx, const bv_batch *b, const bv_out &o, hipStream_t st);
// the batch's item -> key map for the partial-mode item bound (host copy,
// or the device one, copied back only when the batch has table-less keys)
struct bv_kc_items {
  uint64_t n_items = 0;
  const uint32_t *h_item_key = nullptr;
  const uint32_t *d_item_key = nullptr;
};
int bv_kc_prepare(bv_ctx *ctx, uint32_t n_keys, const uint8_t *hkb, const uint64_t *hko, const uint8_t *dkb,
                  const uint64_t *dko, hipStream_t st, bool *use, bool force_build = false,
                  const bv_kc_items *items = nullptr);
// The key-cache step of a host entry (nothing without BV_F_KEY_CACHE): `st`
// waits for the keys in HBM (E_KREADY), then bv_kc_prepare over the host keys,
// their device copy (d's key_bytes / key_off) and the items' keys on the host
int bv_kc_host_step(bv_ctx *ctx, const uint8_t *hkb, const uint64_t *hko, const bv_batch &d,
                    const uint32_t *h_item_key, hipStream_t st, bool *kc);
uint32_t bv_kc_lookup(bv_ctx *ctx, uint32_t n_keys, const uint8_t *hkb, const uint64_t *hko, uint64_t *tabs);
bool bv_kc_all_cached(bv_ctx *ctx, uint32_t n_keys, const uint8_t *hkb, const uint64_t *hko);
void bv_kc_init(bv_ctx *ctx);     // budget, admission and fault-injection settings (bv_create)
void bv_kc_release(bv_ctx *ctx);  // free every cached table (bv_destroy, after all calls finished)
// `res` (may be null): the caller's result buffers, written by DMA directly
// when they are bv_host_alloc memory (else bv_host_finish copies them).
// `sig` (may be null; host pointers, validated by the caller): the items'
// signature text, staged where s and pre are otherwise and decoded on the
// device; b's r_be / s_be / pre are then neither read nor staged.
int bv_host_launch(bv_ctx *ctx, const bv_batch *b, bv_host_call *call, const bv_result *res = nullptr,
                   const bv_sig_text *sig = nullptr);
int bv_host_finish(bv_ctx *ctx, const bv_batch *b, bv_result *res, bv_host_call *call, bool bits_out);
// The one-launch small path of the host entries (bv_api.cpp): bv_small_batch
// is the routing rule (item and message counts, message lengths, the key
// cache's state), bv_small_verify the call itself over a validated batch.
// `sig` (may be null; validated by the caller): the items' signature text.
bool bv_small_batch(bv_ctx *ctx, const bv_batch *b, bool text = false);
int bv_small_verify(bv_ctx *ctx, const bv_batch *b, bv_result *res, const bv_sig_text *sig = nullptr);
// bv_verify_batch_text's checks of sig_off / sig_text (and their bv_last_error texts)
int bv_validate_sig_text(bv_ctx *ctx, uint64_t n_items, const bv_sig_text &sig);
// bv_verify_events' bulk path over one event range of a batch (bv_events.cpp):
// events [a, z) and the parent hashes [hash_lo, hash_hi) its BV_PARENT_HASH
// parents name (bv_plan_event_shards).  bv_validate_events checks the WHOLE
// batch once; bv_events_launch enqueues the range's staging, hashing and
// verify (`res`: the range's result pointers, reached by DMA when pinned) and
// bv_events_finish collects after bv_mark_done, as bv_host_launch /
// bv_host_finish do.  An empty range launches nothing (skip its finish).
struct bv_ev_shard {
  uint64_t a, z, hash_lo, hash_hi;
};
int bv_validate_events(bv_ctx *ctx, const bv_event_batch *eb);
int bv_events_launch(bv_ctx *ctx, const bv_event_batch *eb, const bv_ev_shard &sh, const bv_result *res,
                     bv_host_call *call);
int bv_events_finish(bv_ctx *ctx, uint64_t n_events, bv_result *res, bv_host_call *call, bool bits_out);
// bv_verify_blocks' bulk pipeline over one block range of a batch
// (bv_blocks.cpp): blocks [b0, b1) and the items [i0, i1) that name them
// (bv_plan_block_shards).  bv_validate_blocks checks the WHOLE batch once
// (*text: the items' signatures come as text); bv_blocks_small is the routing
// decision of bv_verify_blocks for the whole batch (the one-launch small
// path); bv_blocks_launch enqueues the range's staging, hashing, verify and
// tally (`res`, `valid_count`: the range's result pointers, reached by DMA
// when pinned) and bv_blocks_finish collects after bv_mark_done.  An empty
// block range launches nothing (skip its finish).
struct bv_blk_shard {
  uint64_t b0, b1, i0, i1;
};
struct bv_blk_call {
  bv_host_call host;
  uint64_t n_blocks = 0, n_items = 0;  // the range's
  size_t o_cnt = 0;                    // its counts in host.pout, unless direct_cnt
  bool direct_cnt = false;
  bool lens_done = false;  // ctx->blk_off already holds the range's body offsets (the route needed them)
};
int bv_validate_blocks(bv_ctx *ctx, const bv_block_batch *blocks, bool *text);
bool bv_blocks_small(bv_ctx *ctx, const bv_block_batch *blocks, bool text);
int bv_blocks_launch(bv_ctx *ctx, const bv_block_batch *blocks, const bv_blk_shard &sh, const bv_result *res,
                     uint32_t *valid_count, bv_blk_call *call, bool text);
int bv_blocks_finish(bv_ctx *ctx, bv_result *res, uint32_t *valid_count, bv_blk_call *call, bool bits_out);
// bv_verify_events_itx / bv_verify_events_fields' bulk pipeline over one event
// range of a batch (bv_event_itx.cpp; `f`: the fields batch, x == &f->ev, or
// null for the ITX entry): events [a, z), the ITXs, block signatures and
// transactions they own and the parent hashes [hash_lo, hash_hi).
// bv_evf_validate checks the WHOLE batch once (*route: EVF_RUN, or which
// fall-back entry takes the batch: bv_evf_no_itx / bv_evf_no_bsig, called
// without a ctx locked); bv_evf_try_small is the single-context entries'
// routing decision for the whole batch (*taken: it ran on the one-launch small
// path and the results are written); bv_evf_launch builds the range's keys and
// signature text on the ctx's pool and enqueues its staging, hashing, verify
// and fold; bv_evf_finish collects after bv_mark_done (`res`, `out`: the
// range's result pointers).  An empty range launches nothing (skip its finish).
enum { EVF_RUN, EVF_NO_ITX, EVF_NO_BSIG };
struct bv_evf_call {
  bv_host_call host;
  uint64_t n = 0, m = 0;         // the range's events and ITXs
  size_t p_ist = 0, p_dby = 0;   // itx_status and decided_by in host.pout
  const void *d_bits = nullptr;  // the range's accept words on the device (k_ev_compose's)
};
int bv_evf_validate(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, int *route);
int bv_evf_try_small(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, bv_result *res,
                     bv_event_itx_out *out, bool *taken);
int bv_evf_launch(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, const bv_ev_shard &sh,
                  bv_evf_call *call);
int bv_evf_finish(bv_ctx *ctx, bv_result *res, bv_event_itx_out *out, bv_evf_call *call, bool bits_out);
int bv_evf_no_itx(const bv_event_itx_batch *x, bv_result *res, bv_event_itx_out *out,
                  const std::function<int(const bv_event_batch *, bv_result *)> &verify_events);
int bv_evf_no_bsig(const bv_event_fields_batch *f, bv_result *res, bv_event_itx_out *out,
                   const std::function<int(const bv_event_itx_batch *, bv_result *, bv_event_itx_out *)> &verify_itx,
                   const std::function<int(const bv_event_batch *, bv_result *)> &verify_events);
void bv_read_timing(bv_ctx *ctx);
