// bv_verify_blocks: canonical BlockBody JSON built from the blocks' fields,
// hashed, then the verify pipeline over the block signatures, and CheckBlock's
// tally per block (include/babbleverify.h; blkjson.h).
//
// Host work is validation, the body lengths (which bodies are too long for a
// lane, which route the batch takes) and the staging of the compact arrays, in
// the order the device can use them: the keys (key decode, key tables or the
// key cache), the signature text or s / pre (k_sig_decode, s^-1), the item
// arrays (the key part of every item, u2 Q, runs under the rest of the
// transfer), then the block fields.  Once the fields land, ONE k_blk_body_hash
// launch serialises every body straight into SHA-256 (no body is stored);
// bodies longer than kHostHashLen are built and hashed by the pool threads
// meanwhile and their digests put in place (k_put_digests); then u1 G and the
// decision for every item, and k_blk_tally.  A batch the text entry would run
// on its one-launch small path has its bodies built on the host and takes
// that path (which hashes on the host already).
//
// The bulk pipeline is split as bv_verify_events' is: bv_validate_blocks over
// the whole batch, bv_blocks_launch over one block range and its items, and
// bv_blocks_finish.  bv_verify_blocks passes the whole range with zero bases;
// bv_group_verify_blocks (bv_group.cpp) one shard per device slot.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "blkjson.h"
#include "bv_internal.h"
#include "hostsha.h"

namespace {

constexpr size_t kChunk = 64ull << 20;  // staged bytes per pinned piece (as bv_events.cpp)
constexpr size_t kSmallStage = 1ull << 20;  // a layout up to this size crosses in one copy (as bv_host_launch)
constexpr uint64_t kGrain = 1 << 17;

// fn(lo, hi) over [0, n) on the pool (when there is one) and the caller
bool par(CopyPool *pool, uint64_t n, uint64_t grain, const std::function<bool(uint64_t, uint64_t)> &fn) {
  return pool ? pool->parallel_for(n, grain, fn) : fn(0, n);
}

// The block fields (what blk_len / blk_emit read): nullptr, or what is wrong.
const char *check_fields(const bv_block_batch *k, CopyPool *pool) {
  const uint64_t n = k->n_blocks;
  if (!n) return nullptr;
  if (n > (1ull << 32)) return "more than 2^32 blocks";
  if (!k->index || !k->round_received || !k->timestamp || !k->hash_off || !k->tx_start) return "null block array";
  if (k->hash_off[0] != 0) return "hash_off[0] != 0";
  if (!monotone(pool, k->hash_off, 3 * n)) return "hash_off not monotone";
  if (k->hash_off[3 * n] && !k->hash_bytes) return "null hash bytes";
  if (k->tx_start[0] != 0) return "tx_start[0] != 0";
  if (!monotone(pool, k->tx_start, n)) return "tx_start not monotone";
  const uint64_t n_tx = k->tx_start[n];
  if (n_tx && !k->tx_off) return "null tx_off";
  if (n_tx && k->tx_off[0] != 0) return "tx_off[0] != 0";
  if (n_tx && !monotone(pool, k->tx_off, n_tx)) return "tx_off not monotone";
  if (n_tx && k->tx_off[n_tx] && !k->tx_bytes) return "null tx bytes";
  const uint64_t *offs[2] = {k->itx_off, k->rcpt_off};
  const uint8_t *json[2] = {k->itx_json, k->rcpt_json};
  for (int f = 0; f < 2; f++) {
    if (!offs[f]) continue;
    if (offs[f][0] != 0) return "fragment offsets must start at 0";
    if (!monotone(pool, offs[f], n)) return "fragment offsets not monotone";
    if (offs[f][n] && !json[f]) return "null fragment bytes";
  }
  return nullptr;
}

// blocks [b0, b1): body_off[b - b0 + 1] - body_off[b - b0] = blk_len(b), body_off[0] = 0
void body_lens(const bv_block_batch *k, CopyPool *pool, uint64_t b0, uint64_t b1, uint64_t *body_off) {
  const uint64_t n = b1 - b0;
  body_off[0] = 0;
  par(pool, n, 1 << 12, [k, b0, body_off](uint64_t lo, uint64_t hi) {
    for (uint64_t b = lo; b < hi; b++) body_off[b + 1] = blk_len(*k, b0 + b);
    return true;
  });
  for (uint64_t b = 0; b < n; b++) body_off[b + 1] += body_off[b];
}

void bodies(const bv_block_batch *k, CopyPool *pool, const uint64_t *body_off, uint8_t *out) {
  par(pool, k->n_blocks, 16, [k, body_off, out](uint64_t lo, uint64_t hi) {
    for (uint64_t b = lo; b < hi; b++) blk_write(*k, b, out + body_off[b]);
    return true;
  });
}

}  // namespace

int bv_validate_blocks(bv_ctx *ctx, const bv_block_batch *k, bool *text) {
  if (const char *why = check_fields(k, ctx->pool)) return bv_fail(ctx, BV_E_ARGS, why);
  const uint64_t n = k->n_blocks, n_items = k->n_items;
  const uint32_t n_keys = k->n_keys;
  *text = n_items && k->sig_text;
  if (n_items && (!k->item_block || !k->item_key)) return bv_fail(ctx, BV_E_ARGS, "null item array");
  if (n_items && !n_keys) return bv_fail(ctx, BV_E_ARGS, "items without keys");
  if (n_keys && !k->key_off) return bv_fail(ctx, BV_E_ARGS, "null key_off");
  if (n_keys && k->key_off[0] != 0) return bv_fail(ctx, BV_E_ARGS, "key_off[0] != 0");
  for (uint32_t i = 0; i < n_keys; i++)
    if (k->key_off[i] > k->key_off[i + 1]) return bv_fail(ctx, BV_E_ARGS, "key_off not monotone");
  if (n_keys && k->key_off[n_keys] && !k->key_bytes) return bv_fail(ctx, BV_E_ARGS, "null key bytes");
  if (n_items && !k->sig_text && !k->sig_off && (!k->r_be || !k->s_be))
    return bv_fail(ctx, BV_E_ARGS, "neither sig_text nor r_be / s_be");
  if (n_items && (k->sig_text || !k->r_be || !k->s_be)) {  // the text entry's rules for sig_off / sig_text
    const int rc = bv_validate_sig_text(ctx, n_items, bv_sig_text{k->sig_off, k->sig_text});
    if (rc != BV_OK) return rc;
    *text = true;
  }
  if (!ctx->pool->parallel_for(n_items, kGrain, [k, n, n_keys](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++)
          if (k->item_block[i] >= n || k->item_key[i] >= n_keys) return false;
        return true;
      }))
    return bv_fail(ctx, BV_E_ARGS, "item index out of range (item_block >= n_blocks or item_key >= n_keys)");
  return BV_OK;
}

namespace {

// Whether the batch is small enough that the route needs its body lengths
// before anything is staged.
bool maybe_small_batch(bv_ctx *ctx, const bv_block_batch *k) {
  return ctx->small_path && k->n_items &&
         std::max(k->n_items, k->n_blocks) <= std::max(ctx->small_max, ctx->small_warm_max);
}

// The items as bv_batch items over the bodies as messages (ctx->blk_off: the
// body offsets, filled by the caller); the route is decided from the offsets alone.
bv_batch items_over_bodies(bv_ctx *ctx, const bv_block_batch *k, bool text) {
  static const uint8_t kNoBytes[64] = {};
  bv_batch hb = {};
  hb.n_msgs = k->n_blocks;
  hb.msg_bytes = kNoBytes;
  hb.msg_off = ctx->blk_off.data();
  hb.n_keys = k->n_keys;
  hb.key_bytes = k->key_bytes;
  hb.key_off = k->key_off;
  hb.n_items = k->n_items;
  hb.item_msg = k->item_block;
  hb.item_key = k->item_key;
  if (!text) hb.r_be = k->r_be, hb.s_be = k->s_be, hb.pre = k->pre;
  return hb;
}

}  // namespace

// The routing decision bv_verify_blocks makes for a validated batch: true when
// it runs on the one-launch small path.  (bv_group_verify_blocks asks it for
// the whole batch; the batch then goes to bv_verify_blocks on slot 0.)
bool bv_blocks_small(bv_ctx *ctx, const bv_block_batch *k, bool text) {
  if (!k->n_blocks || !maybe_small_batch(ctx, k)) return false;
  ctx->blk_off.resize(k->n_blocks + 1);
  body_lens(k, ctx->pool, 0, k->n_blocks, ctx->blk_off.data());
  const bv_batch hb = items_over_bodies(ctx, k, text);
  return bv_small_batch(ctx, &hb, text);
}

static int verify_blocks_impl(bv_ctx *ctx, const bv_block_batch *k, bv_result *res, uint32_t *valid_count) {
  bv_blk_call call;
  call.host.t0 = std::chrono::steady_clock::now();
  bool text = false;
  int rc = bv_validate_blocks(ctx, k, &text);
  if (rc != BV_OK) return rc;
  hipStream_t st = ctx->stream;
  ctx->timing = bv_timing{};
  ctx->last = st;
  const uint64_t n = k->n_blocks, n_items = k->n_items;
  if (n == 0) return BV_OK;  // (validated: no items either)

  // Body lengths: the route (only a batch small enough to take the one-launch
  // path needs them before anything is staged) and the long bodies (bulk
  // batches: found in bv_blocks_launch, while the signatures cross PCIe).
  std::vector<uint64_t> &body_off = ctx->blk_off;
  body_off.resize(n + 1);
  const bool maybe_small = maybe_small_batch(ctx, k);
  if (maybe_small) body_lens(k, ctx->pool, 0, n, body_off.data());

  // Small batches: the text entry's routing decision for the same item count
  // and keys; the bodies are built here and the one-launch path hashes them
  // on the host.  Its statuses land in host memory, where they are tallied.
  bv_batch hb = items_over_bodies(ctx, k, text);
  const bv_sig_text htext{k->sig_off, k->sig_text};
  if (maybe_small && bv_small_batch(ctx, &hb, text)) {
    ctx->blk_bodies.resize(body_off[n] + 64);
    bodies(k, ctx->pool, body_off.data(), ctx->blk_bodies.data());
    memset(ctx->blk_bodies.data() + body_off[n], 0, 64);
    hb.msg_bytes = ctx->blk_bodies.data();
    rc = bv_validate_host_batch(ctx, &hb, text);
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> tmp;
    bv_result r2 = *res;
    if (valid_count && !r2.status) {
      tmp.resize(n_items);
      r2.status = tmp.data();
    }
    rc = bv_small_verify(ctx, &hb, &r2, text ? &htext : nullptr);
    if (rc != BV_OK) return rc;
    if (valid_count) {
      memset(valid_count, 0, n * 4);
      for (uint64_t i = 0; i < n_items; i++)
        if (r2.status[i] == BV_ACCEPT) valid_count[k->item_block[i]]++;
    }
    return BV_OK;
  }

  // the bulk pipeline: the whole batch as one shard with zero bases
  call.lens_done = maybe_small;
  const bv_blk_shard whole{0, n, 0, n_items};
  rc = bv_blocks_launch(ctx, k, whole, res, valid_count, &call, text);
  if (rc != BV_OK) return rc;
  rc = bv_mark_done(ctx, st);
  if (rc != BV_OK) return rc;
  return bv_blocks_finish(ctx, res, valid_count, &call, true);
}

int bv_blocks_finish(bv_ctx *ctx, bv_result *res, uint32_t *valid_count, bv_blk_call *call, bool bits_out) {
  bv_batch sizes = {};
  sizes.n_msgs = call->n_blocks;
  sizes.n_items = call->n_items;
  const int rc = bv_host_finish(ctx, &sizes, res, &call->host, bits_out);
  if (rc != BV_OK) return rc;
  if (valid_count && !call->direct_cnt) memcpy(valid_count, call->host.pout + call->o_cnt, call->n_blocks * 4);
  return BV_OK;
}

// The bulk pipeline over blocks [sh.b0, sh.b1) of a validated batch and the
// items [sh.i0, sh.i1) that name them: everything up to the call's last
// enqueued command (the caller records the end with bv_mark_done and collects
// with bv_blocks_finish).  bv_verify_blocks passes the whole batch;
// bv_group_verify_blocks one shard per device slot.  The shard's slices are
// staged from where they lie in the caller's arrays, and the values in them
// stay the whole batch's: the serialiser subtracts the bases (blkjson.h
// BlkBases), k_sig_decode the text's, and k_blk_item_rebase writes the items'
// block indices less sh.b0 for the verify kernels and the tally, whose digest
// and count arrays are the shard's.  With every base zero the un-based kernel
// runs and the items are read as staged.  The long bodies are built on the
// host from the whole batch.
int bv_blocks_launch(bv_ctx *ctx, const bv_block_batch *whole, const bv_blk_shard &sh, const bv_result *res,
                     uint32_t *valid_count, bv_blk_call *call_p, bool text_batch) {
  bv_host_call &call = call_p->host;
  int rc = BV_OK;
  hipStream_t st = ctx->stream;
  ctx->timing = bv_timing{};
  ctx->last = st;
  const uint64_t n = sh.b1 - sh.b0, n_items = sh.i1 - sh.i0;  // the shard's: b and i below are shard-local
  call_p->n_blocks = n;
  call_p->n_items = n_items;
  if (n == 0) return BV_OK;
  const uint32_t n_keys = whole->n_keys;
  BlkBases bs = {};
  bs.blk = sh.b0;
  bs.hash = whole->hash_off[3 * sh.b0];
  bs.tx = whole->tx_start[sh.b0];
  bs.txb = whole->tx_start[whole->n_blocks] ? whole->tx_off[bs.tx] : 0;
  bs.itx = whole->itx_off ? whole->itx_off[sh.b0] : 0;
  bs.rcpt = whole->rcpt_off ? whole->rcpt_off[sh.b0] : 0;
  const bool text = text_batch && n_items;  // (a shard of item-less blocks has no text to decode)
  const uint64_t sig_base = text ? whole->sig_off[sh.i0] : 0;
  const bool rebased = bs.blk || bs.hash || bs.tx || bs.txb || bs.itx || bs.rcpt;
  // the shard's view of the caller's arrays (host pointers to its first elements)
  bv_block_batch view = *whole;
  {
    auto adv = [](auto *&p, uint64_t by) {
      if (p) p += by;
    };
    view.n_blocks = n;
    view.n_items = n_items;
    adv(view.index, sh.b0), adv(view.round_received, sh.b0), adv(view.timestamp, sh.b0);
    adv(view.hash_off, 3 * sh.b0), adv(view.hash_bytes, bs.hash), adv(view.hash_nil, 3 * sh.b0);
    adv(view.tx_start, sh.b0), adv(view.tx_off, bs.tx), adv(view.tx_bytes, bs.txb);
    adv(view.tx_list_nil, sh.b0), adv(view.tx_nil, bs.tx);
    adv(view.itx_off, sh.b0), adv(view.itx_json, bs.itx), adv(view.rcpt_off, sh.b0), adv(view.rcpt_json, bs.rcpt);
    adv(view.item_block, sh.i0), adv(view.item_key, sh.i0);
    adv(view.sig_off, sh.i0), adv(view.sig_text, sig_base);
    adv(view.r_be, 32 * sh.i0), adv(view.s_be, 32 * sh.i0), adv(view.pre, sh.i0);
  }
  const bv_block_batch *k = &view;
  std::vector<uint64_t> &body_off = ctx->blk_off;  // the shard's bodies (whole batch: maybe filled for the route)
  const bool lens_done = call_p->lens_done;
  if (!lens_done) body_off.resize(n + 1);

  const uint64_t key_len = n_keys ? k->key_off[n_keys] : 0;
  const uint64_t n_tx = k->tx_start[n] - bs.tx, tx_len = n_tx ? k->tx_off[n_tx] - bs.txb : 0;
  const uint64_t hash_len = k->hash_off[3 * n] - bs.hash;
  const uint64_t itx_len = k->itx_off ? k->itx_off[n] - bs.itx : 0,
                 rcpt_len = k->rcpt_off ? k->rcpt_off[n] - bs.rcpt : 0;
  const uint64_t text_len = text ? k->sig_off[n_items] - sig_base : 0;
  StagePlan plan;
  auto add = [&](const void *src, size_t bytes, size_t pad = 0) { return plan.add(src, bytes, {}, 1, pad); };
  // the keys; the signature text or s / pre; the item arrays; the block fields
  const size_t o_koff = add(k->key_off, n_keys ? (n_keys + 1) * 8ull : 0);
  const size_t i_kb = plan.segs.size(), o_kb = add(k->key_bytes, key_len, 64);
  const size_t keys_end = plan.total;
  const size_t o_s = text ? add(k->sig_off, (n_items + 1) * 8) : add(k->s_be, n_items * 32);
  const size_t o_pre = text ? add(k->sig_text, text_len) : add(k->pre, n_items);
  const size_t s_end = plan.total;
  const size_t o_ib = add(k->item_block, n_items * 4);
  const size_t o_ik = add(k->item_key, n_items * 4);
  const size_t o_r = add(text ? nullptr : k->r_be, n_items * 32);
  const size_t r_end = plan.total;
  const size_t o_ix = add(k->index, n * 8);
  const size_t o_rr = add(k->round_received, n * 8);
  const size_t o_ts = add(k->timestamp, n * 8);
  const size_t o_ho = add(k->hash_off, (3 * n + 1) * 8);
  const size_t i_hb = plan.segs.size(), o_hb = add(k->hash_bytes, hash_len, 64);
  const size_t o_hn = add(k->hash_nil, 3 * n);
  const size_t o_txs = add(k->tx_start, (n + 1) * 8);
  const size_t o_txo = add(k->tx_off, n_tx ? (n_tx + 1) * 8 : 0);
  const size_t i_txb = plan.segs.size(), o_txb = add(k->tx_bytes, tx_len, 64);
  const size_t o_tln = add(k->tx_list_nil, n);
  const size_t o_txn = add(k->tx_nil, n_tx);
  const size_t o_io = add(k->itx_off, (n + 1) * 8);
  const size_t o_ij = add(k->itx_json, itx_len);
  const size_t o_ro = add(k->rcpt_off, (n + 1) * 8);
  const size_t o_rj = add(k->rcpt_json, rcpt_len);
  const size_t total = plan.total;

  if (bv_wait_all(ctx) != BV_OK) return BV_E_LAUNCH;  // previous calls' work buffers / staging
  HIPCHK(ctx->pin_in.ensure(total + 256), BV_E_OOM, "alloc pinned staging");
  HIPCHK(ctx->d_in.ensure(total + 256), BV_E_OOM, "alloc device staging");
  uint8_t *pin = (uint8_t *)ctx->pin_in.p, *dev = ctx->d_in.as<uint8_t>();
  hipStream_t cs = bv_copy_stream(ctx);
  if (!cs) return bv_fail(ctx, BV_E_NODEVICE, "copy stream");
  hipEvent_t *ev = ctx->S().ev;
  HIPCHK(hipEventRecord(ev[E_CALL], cs), BV_E_LAUNCH, "event");
  plan.mark_direct(bv_is_pinned);  // arrays in bv_host_alloc memory are DMA'd from where they are
  const std::vector<char> &direct = plan.direct;
  // a batch whose whole layout is at most kSmallStage crosses PCIe as ONE copy
  // (each extra small H2D costs ~20 us of DMA latency on a lone call): every
  // array, pinned or not, is gathered into the staging first
  const bool one_copy = total <= kSmallStage;
  if (one_copy) {
    memset(pin, 0, total);
    if ((rc = bv_stage_one_copy(ctx, plan)) != BV_OK) return rc;
  }
  // else layout bytes [a0, a1) in kChunk pieces: the pool fills piece c+1 while the DMA engine moves piece c
  auto cross = [&](size_t a0, size_t a1) { return one_copy ? BV_OK : bv_stage_range(ctx, plan, a0, a1, kChunk); };
  if (!one_copy && !direct[i_kb]) memset(pin + o_kb + key_len, 0, 64);
  rc = cross(0, keys_end);  // the keys: key decode and the key tables start once they land
  if (rc != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_KREADY], cs), BV_E_LAUNCH, "event");

  bv_batch d = {};  // the items over device pointers
  d.n_msgs = n;
  d.n_keys = n_keys;
  d.key_bytes = dev + o_kb;
  d.key_off = (const uint64_t *)(dev + o_koff);
  d.n_items = n_items;
  d.item_msg = (const uint32_t *)(dev + o_ib);
  if (bs.blk && n_items) {  // the shard's digest and count arrays are its own: k_blk_item_rebase, below
    HIPCHK(ctx->d_blk_item.ensure(n_items * 4), BV_E_OOM, "alloc rebased item blocks");
    d.item_msg = ctx->d_blk_item.as<uint32_t>();
  }
  d.item_key = (const uint32_t *)(dev + o_ik);
  d.r_be = dev + o_r;
  d.s_be = dev + o_s;
  d.pre = !text && k->pre ? dev + o_pre : nullptr;
  bv_sig_text dsig;
  if (text) {  // decoded on the s^-1 stream (bv_run_keys) into ctx->d_sig
    dsig.off = (const uint64_t *)(dev + o_s);
    dsig.text = dev + o_pre;
    dsig.base = sig_base;
    bv_sig_out so;
    rc = bv_sig_bufs(ctx, n_items, &so);
    if (rc != BV_OK) return rc;
    d.r_be = so.r, d.s_be = so.s, d.pre = so.pre;
  }
  bool kc = false;
  if (n_keys && n_keys <= kKcMaxBatchKeys) {  // (else `st` does not wait for the keys either)
    rc = bv_kc_host_step(ctx, k->key_bytes, k->key_off, d, k->item_key, st, &kc);
    if (rc != BV_OK) return rc;
  }
  rc = cross(keys_end, s_end);  // the signature text, or s and pre: k_sig_decode, s^-1
  if (rc != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_SREADY], cs), BV_E_LAUNCH, "event");
  rc = bv_run_keys(ctx, &d, ev[E_KREADY], ev[E_SREADY], kc, false, text ? &dsig : nullptr);
  if (rc != BV_OK) return rc;
  if (text) HIPCHK(hipStreamWaitEvent(st, ev[E_SDEC], 0), BV_E_LAUNCH, "join decoded signatures");
  rc = cross(s_end, r_end);  // item_block, item_key, r: the key part of every item
  if (rc != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_RREADY], cs), BV_E_LAUNCH, "event");
  bv_item_pipe pipe{ctx, &d, {}, st, kc};
  rc = bv_out_bufs(ctx, &d, nullptr, nullptr, nullptr, true, &pipe.o);
  if (rc != BV_OK) return rc;
  rc = pipe.key_part(ctx->sstream, ev[E_RREADY]);
  if (rc != BV_OK) return rc;

  // the block fields (the long blocks' too: they are a few); the list of the
  // long blocks goes with them, their digests follow
  // (under the transfers enqueued so far)
  if (!lens_done) body_lens(whole, ctx->pool, sh.b0, sh.b1, body_off.data());
  std::vector<uint64_t> longb;
  for (uint64_t b = 0; b < n; b++)
    if (body_off[b + 1] - body_off[b] > kHostHashLen) longb.push_back(b);
  const uint64_t nl = longb.size();
  uint64_t *lidx = nullptr;
  if (nl) {
    HIPCHK(ctx->pin_long.ensure(nl * 40), BV_E_OOM, "alloc pinned long digests");
    HIPCHK(ctx->d_long.ensure(nl * 40), BV_E_OOM, "alloc long digests");
    lidx = (uint64_t *)ctx->pin_long.p;
    memcpy(lidx, longb.data(), nl * 8);
    HIPCHK(hipMemcpyAsync(ctx->d_long.p, lidx, nl * 8, hipMemcpyHostToDevice, cs), BV_E_LAUNCH, "h2d long blocks");
  }
  if (!one_copy && hash_len && !direct[i_hb]) memset(pin + o_hb + hash_len, 0, 64);
  if (!one_copy && tx_len && !direct[i_txb]) memset(pin + o_txb + tx_len, 0, 64);
  rc = cross(r_end, total);
  if (rc != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_SMALL], cs), BV_E_LAUNCH, "event");

  bv_block_batch dk = *k;  // the same blocks over device pointers
  dk.index = (const int64_t *)(dev + o_ix);
  dk.round_received = (const int64_t *)(dev + o_rr);
  dk.timestamp = (const int64_t *)(dev + o_ts);
  dk.hash_off = (const uint64_t *)(dev + o_ho);
  dk.hash_bytes = dev + o_hb;
  dk.hash_nil = k->hash_nil ? dev + o_hn : nullptr;
  dk.tx_start = (const uint64_t *)(dev + o_txs);
  dk.tx_off = n_tx ? (const uint64_t *)(dev + o_txo) : nullptr;
  dk.tx_bytes = dev + o_txb;
  dk.tx_list_nil = k->tx_list_nil ? dev + o_tln : nullptr;
  dk.tx_nil = k->tx_nil && n_tx ? dev + o_txn : nullptr;
  dk.itx_off = k->itx_off ? (const uint64_t *)(dev + o_io) : nullptr;
  dk.itx_json = dev + o_ij;
  dk.rcpt_off = k->rcpt_off ? (const uint64_t *)(dev + o_ro) : nullptr;
  dk.rcpt_json = dev + o_rj;
  dk.key_bytes = nullptr, dk.key_off = nullptr, dk.item_block = dk.item_key = nullptr;  // (not read by the serialiser)
  dk.sig_off = nullptr, dk.sig_text = dk.r_be = dk.s_be = dk.pre = nullptr;

  // results: pinned memory, or straight into the caller's bv_host_alloc buffers
  const size_t o_st = align256(n * 32), o_bits = o_st + align256(n_items),
               o_cnt = o_bits + align256((n_items + 63) / 64 * 8);
  HIPCHK(ctx->pin_out.ensure(o_cnt + align256(n * 4) + 256), BV_E_OOM, "alloc pinned results");
  uint8_t *pout = (uint8_t *)ctx->pin_out.p;
  call.pout = pout;
  call.o_st = o_st;
  call.o_bits = o_bits;
  call.direct_hash = bv_is_pinned(res->msg_hash, n * 32);
  call.direct_status = n_items && bv_is_pinned(res->status, n_items);
  const bool direct_cnt = valid_count && bv_is_pinned(valid_count, n * 4);
  call_p->o_cnt = o_cnt;
  call_p->direct_cnt = direct_cnt;
  uint8_t *hout = call.direct_hash ? res->msg_hash : pout;

  if (ctx->has_done) HIPCHK(hipStreamWaitEvent(st, ctx->ev_done, 0), BV_E_LAUNCH, "order");
  HIPCHK(hipEventRecord(ev[E_HASH0], st), BV_E_LAUNCH, "event");
  HIPCHK(hipStreamWaitEvent(st, ev[E_SMALL], 0), BV_E_LAUNCH, "join block fields");
  // (the item arrays landed before the fields; nothing before k_verify_gf reads item_msg: the key part does not)
  if (d.item_msg != (const uint32_t *)(dev + o_ib))
    HIPCHK(bvk::blk_item_rebase(st, n_items, (const uint32_t *)(dev + o_ib), (uint32_t)bs.blk,
                                ctx->d_blk_item.as<uint32_t>()),
           BV_E_LAUNCH, "k_blk_item_rebase");
  HIPCHK(hipEventRecord(ev[E_FORK], st), BV_E_LAUNCH, "event");  // ms_sha256: the build-and-hash kernel
  HIPCHK(rebased ? bvk::blk_body_hash_rb(st, dk, sh.b0, sh.b1, ctx->d_long.as<uint64_t>(), nl, bs, pipe.o.dig,
                                         ctx->blk_nt)
                 : bvk::blk_body_hash(st, dk, 0, n, ctx->d_long.as<uint64_t>(), nl, pipe.o.dig, ctx->blk_nt),
         BV_E_LAUNCH, "k_blk_body_hash");
  HIPCHK(hipEventRecord(ev[E_HASHED], st), BV_E_LAUNCH, "event");
  if (nl) {
    // the long bodies on the host (pool threads: blk_emit into scratch, SHA
    // extensions) while the device hashes the rest; then their digests cross
    uint8_t *ldig = (uint8_t *)(lidx + nl);
    ctx->pool->parallel_for(nl, 1, [&](uint64_t lo, uint64_t hi) {
      std::vector<uint8_t> body;
      for (uint64_t i = lo; i < hi; i++) {
        const uint64_t b = longb[i], len = body_off[b + 1] - body_off[b];
        body.resize(len);
        blk_write(*whole, sh.b0 + b, body.data());  // (the host reads the caller's whole arrays: no bases)
        hsha::digest(body.data(), len, ldig + 32 * i);
      }
      return true;
    });
    HIPCHK(hipMemcpyAsync(ctx->d_long.as<uint8_t>() + nl * 8, ldig, nl * 32, hipMemcpyHostToDevice, cs), BV_E_LAUNCH,
           "h2d long digests");
    hipEvent_t e = ctx->chunk_ev[0];
    HIPCHK(hipEventRecord(e, cs), BV_E_LAUNCH, "event");
    HIPCHK(hipStreamWaitEvent(st, e, 0), BV_E_LAUNCH, "join long digests");
    HIPCHK(bvk::put_digests(st, nl, ctx->d_long.as<uint64_t>(), (const uint32_t *)(ctx->d_long.as<uint8_t>() + nl * 8),
                            pipe.o.dig),
           BV_E_LAUNCH, "k_put_digests");
    HIPCHK(hipEventRecord(ev[E_HASHED], st), BV_E_LAUNCH, "event");
  }
  HIPCHK(hipEventRecord(ev[E_SHA], st), BV_E_LAUNCH, "event");
  HIPCHK(hipEventRecord(ev[E_STAGED], cs), BV_E_LAUNCH, "event");
  call.ms_prep = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - call.t0).count();

  rc = pipe.finish();  // u1 G and the decision of every item
  if (rc != BV_OK) return rc;

  // the digests as soon as hashing ended, beside the verify kernels
  HIPCHK(hipStreamWaitEvent(cs, ev[E_HASHED], 0), BV_E_LAUNCH, "join");
  HIPCHK(hipMemcpyAsync(hout, pipe.o.dig, n * 32, hipMemcpyDeviceToHost, cs), BV_E_LAUNCH, "d2h digests");
  if (n_items && res->status)
    HIPCHK(hipMemcpyAsync(call.direct_status ? res->status : pout + o_st, pipe.o.status, n_items,
                          hipMemcpyDeviceToHost, st),
           BV_E_LAUNCH, "d2h status");
  if (n_items && res->accept_bits)
    HIPCHK(hipMemcpyAsync(pout + o_bits, pipe.o.bits, (n_items + 63) / 64 * 8, hipMemcpyDeviceToHost, st), BV_E_LAUNCH,
           "d2h bits");
  if (valid_count) {  // CheckBlock's tally, on the device
    HIPCHK(ctx->d_blk_count.ensure(n * 4), BV_E_OOM, "alloc valid counts");
    uint32_t *cnt = ctx->d_blk_count.as<uint32_t>();
    HIPCHK(hipMemsetAsync(cnt, 0, n * 4, st), BV_E_LAUNCH, "zero valid counts");
    HIPCHK(bvk::blk_tally(st, n_items, d.item_msg, pipe.o.status, cnt), BV_E_LAUNCH, "k_blk_tally");
    HIPCHK(hipMemcpyAsync(direct_cnt ? (uint8_t *)valid_count : pout + o_cnt, cnt, n * 4, hipMemcpyDeviceToHost, st),
           BV_E_LAUNCH, "d2h valid counts");
  }
  HIPCHK(hipEventRecord(ev[E_OUT], st), BV_E_LAUNCH, "event");
  HIPCHK(hipStreamWaitEvent(st, ev[E_STAGED], 0), BV_E_LAUNCH, "join");  // staging free after this point
  HIPCHK(hipEventRecord(ev[E_CSDONE], cs), BV_E_LAUNCH, "event");  // the digests' d2h precedes ev_done
  HIPCHK(hipStreamWaitEvent(st, ev[E_CSDONE], 0), BV_E_LAUNCH, "join");
  return BV_OK;
}

extern "C" int bv_verify_blocks(bv_ctx *ctx, const bv_block_batch *blocks, bv_result *res, uint32_t *valid_count) {
  if (!ctx || !blocks || !res) return BV_E_ARGS;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
  const int rc = verify_blocks_impl(ctx, blocks, res, valid_count);
  return rc == BV_OK ? rc : bv_drain(ctx, ctx->stream, rc);
}

extern "C" int bv_block_body_lens(const bv_block_batch *blocks, uint64_t *body_off) {
  if (!blocks || !body_off) return BV_E_ARGS;
  if (check_fields(blocks, nullptr)) return BV_E_ARGS;
  body_lens(blocks, nullptr, 0, blocks->n_blocks, body_off);
  return BV_OK;
}

extern "C" int bv_block_bodies(const bv_block_batch *blocks, const uint64_t *body_off, uint8_t *out) {
  if (!blocks || !body_off) return BV_E_ARGS;
  if (check_fields(blocks, nullptr)) return BV_E_ARGS;
  const uint64_t n = blocks->n_blocks;
  for (uint64_t b = 0; b < n; b++)
    if (body_off[b] > body_off[b + 1] || body_off[b + 1] - body_off[b] < blk_len(*blocks, b)) return BV_E_ARGS;
  if (n && body_off[n] > body_off[0] && !out) return BV_E_ARGS;
  bodies(blocks, nullptr, body_off, out);
  return BV_OK;
}
