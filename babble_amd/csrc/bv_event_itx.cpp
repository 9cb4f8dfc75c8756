// bv_verify_events_itx: the whole of Event.Verify in one call
// (include/babbleverify.h; itxjson.h).  The events as bv_verify_events takes
// them, and their InternalTransactions from fields: each
// InternalTransactionBody.Marshal() is built and hashed on the device
// (k_itx_body_hash), each EventBody with its InternalTransactions member too
// (k_ev_body_hash_itx; a batch with in-batch parents on the host in
// topological order, hostdag.cpp, as bv_verify_events does), then the verify
// pipeline runs over n_events + n_itx items (item e: event e under its
// creator's key; item n_events + i: ITX i under the key its PubKeyHex decodes
// to) and k_ev_compose folds the statuses per event.
//
// Host work is validation, the hex decode of every PubKeyHex into the combined
// key array (the creators' keys, then every distinct ITX key that is none of
// them; the key cache and the key path are chosen from host bytes) and
// the staging, in the order the device can use it: the keys, the signature
// text (the events' followed by the ITXs' Signature strings: k_sig_decode,
// s^-1), then the fields.  A batch without ITXs is bv_verify_events over the
// same events with nil / "[]" fragments.
//
// bv_verify_events_fields is the same driver over a bv_event_fields_batch
// (`f` below, null for bv_verify_events_itx): the BlockSignatures member comes
// from fields too (bsigjson.h), so the bodies are built by that batch's
// evj_len / evj_emit on all three routes (k_ev_body_hash_fields, the host DAG,
// the one-launch small path), the block-signature fields are staged beside the
// others, and a batch without ITX fields (ev.itx_start == NULL) or without
// ITXs runs the same pipeline over n_events items.  The block signatures are
// hashed, not verified.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bv_internal.h"
#include "hostsha.h"
#include "bsigjson.h"

namespace {

constexpr uint64_t kGrain = 1 << 15;
constexpr uint64_t kItxKeyMax = 66;  // a decoded key is stored as its first 66 bytes (any length but 0 / 65 is malformed)

bool par(CopyPool *pool, uint64_t n, uint64_t grain, const std::function<bool(uint64_t, uint64_t)> &fn) {
  return pool ? pool->parallel_for(n, grain, fn) : fn(0, n);
}

// The ITX fields (what itxjson.h reads): nullptr, or what is wrong.
const char *check_itx(const bv_event_itx_batch *x, CopyPool *pool) {
  const uint64_t n = x->events.n_events;
  if (x->events.itx_off || x->events.itx_json) return "events.itx_off / itx_json must be NULL (the ITXs come from fields)";
  if (!x->itx_start) return "null itx_start";
  if (x->itx_start[0] != 0) return "itx_start[0] != 0";
  if (!monotone(pool, x->itx_start, n, kGrain)) return "itx_start not monotone";
  const uint64_t m = x->itx_start[n];
  if (n > (1ull << 32) || m > (1ull << 32) || n + m > (1ull << 32)) return "more than 2^32 events and ITXs";
  if (!m) return nullptr;
  if (!x->itx_type) return "null itx_type";
  if (!x->itx_str_off) return "null itx_str_off";
  if (x->itx_str_off[0] != 0) return "itx_str_off[0] != 0";
  if (!monotone(pool, x->itx_str_off, 4 * m, kGrain)) return "itx_str_off not monotone";
  if (x->itx_str_off[4 * m] && !x->itx_str) return "null itx_str";
  return nullptr;
}

// bsig_check (bsigjson.h) with the offset scans spread over the pool
const char *check_bsig(const bv_event_fields_batch *f, CopyPool *pool) {
  return bsig_check(*f, [pool](const uint64_t *off, uint64_t n) { return monotone(pool, off, n, kGrain); });
}

// a fields batch stages bsig_val_off / bsig_val_bytes only when an entry reads them
bool bsig_has_bytes(const bv_event_fields_batch *f, uint64_t nb) {
  return f->bsig_val_kind && nb && memchr(f->bsig_val_kind, BV_BSIG_VAL_BYTES, nb);
}

// Event e's body by the batch's own serialiser: f's when there is one
uint64_t body_len(const bv_event_itx_batch *x, const bv_event_fields_batch *f, uint64_t e, uint32_t pp[2]) {
  return f ? evj_len(*f, e, pp) : evj_len(*x, e, pp);
}
void body_write(const bv_event_itx_batch *x, const bv_event_fields_batch *f, uint64_t e, uint8_t *o) {
  if (f) evj_write(*f, e, o);
  else evj_write(*x, e, o);
}
void dag_hash(const bv_event_itx_batch *x, const bv_event_fields_batch *f, const std::vector<uint32_t> &order,
              const std::vector<uint32_t> &level_off, const HostParFor &pf, HostDagScratch &w, uint8_t *digests) {
  if (f) bv_host_dag_hash_fields(*f, order.data(), level_off.data(), (uint32_t)level_off.size() - 1, pf, w, digests);
  else bv_host_dag_hash_itx(*x, order.data(), level_off.data(), (uint32_t)level_off.size() - 1, pf, w, digests);
}

// common.DecodeFromString of ITX i's PubKeyHex into at most kItxKeyMax bytes:
// the decoded length (capped), or -1 when the string is shorter than 2 bytes
// (the reference panics)
int64_t decode_key(const bv_event_itx_batch *x, uint64_t i, uint8_t *out, std::vector<uint8_t> &big) {
  const uint64_t len = itx_str_len(*x, i, ITX_PUBKEYHEX);
  if (len < 2) return -1;
  const char *s = (const char *)itx_str_ptr(*x, i, ITX_PUBKEYHEX);
  if ((len - 2) / 2 <= kItxKeyMax) return bv_hex_decode(s, len, out);
  big.resize((len - 2) / 2);
  const int64_t k = std::min<int64_t>(bv_hex_decode(s, len, big.data()), (int64_t)kItxKeyMax);
  memcpy(out, big.data(), (size_t)k);
  return k;
}

// What the host builds for the events [a, z) of a validated batch and the ITXs
// they own (the whole batch for the single-context entries, one shard for the
// group's): every array here is indexed from the range's first event / ITX, so
// none of them needs a base on the device.
struct EvfPrep {
  uint64_t i0 = 0, m = 0;  // the range's ITXs are the batch's [i0, i0 + m)
  // the ITX keys decoded at a fixed stride, their lengths, the forced-panic flags
  std::vector<uint8_t> kfix, klen, force;
  std::vector<uint64_t> koff;        // the combined key offsets: the creators' keys whole, then the distinct ITX keys
  std::vector<uint32_t> ikey, usrc;  // ITX i's key slot; the ITX whose bytes fill slot n_keys + u
  std::vector<uint64_t> soff;        // the signature-text offsets: the range's events', then its ITXs' Signature strings
};

// The ITX keys: decoded at a fixed stride by the pool, then packed behind the
// creators' keys, one slot per DISTINCT key: an ITX whose key equals a
// creator's or an earlier ITX's names that slot (a SyncResponse's ITXs are
// about a few peers: the batch keeps its per-key tables and key-cache hits).
// Then the signature text's offsets.
int evf_prep(bv_ctx *ctx, const bv_event_itx_batch *x, bool itx_fields, uint64_t a, uint64_t z, EvfPrep &p) {
  const bv_event_batch *eb = &x->events;
  const uint64_t n = z - a, i0 = itx_fields ? x->itx_start[a] : 0, m = itx_fields ? x->itx_start[z] - i0 : 0;
  p.i0 = i0, p.m = m;
  const uint32_t n_keys = eb->n_keys;
  if ((uint64_t)n_keys + m > 0xFFFFFFFFull) return bv_fail(ctx, BV_E_ARGS, "more than 2^32 keys");
  p.kfix.resize(m * kItxKeyMax), p.klen.resize(m), p.force.resize(m);
  if (m) par(ctx->pool, m, 4096, [&](uint64_t lo, uint64_t hi) {
    std::vector<uint8_t> big;
    for (uint64_t i = lo; i < hi; i++) {
      const int64_t k = decode_key(x, i0 + i, p.kfix.data() + i * kItxKeyMax, big);
      p.force[i] = k < 0;
      p.klen[i] = k < 0 ? 0 : (uint8_t)k;
    }
    return true;
  });
  std::vector<uint64_t> &koff = p.koff;
  koff.assign(eb->key_off, eb->key_off + n_keys + 1);
  p.ikey.resize(m);
  {
    std::unordered_map<std::string, uint32_t> slot;
    for (uint32_t k = 0; k < n_keys; k++)
      slot.emplace(koff[k + 1] > koff[k] ? std::string((const char *)eb->key_bytes + koff[k], koff[k + 1] - koff[k])
                                         : std::string(),
                   k);
    for (uint64_t i = 0; i < m; i++) {
      const auto ins = slot.emplace(std::string((const char *)p.kfix.data() + i * kItxKeyMax, p.klen[i]),
                                    (uint32_t)(n_keys + p.usrc.size()));
      if (ins.second) {
        p.usrc.push_back((uint32_t)i);
        koff.push_back(koff.back() + p.klen[i]);
      }
      p.ikey[i] = ins.first->second;
    }
  }
  // the signature text: the events', then the ITXs' Signature strings
  const uint64_t sig_base = eb->sig_off[a];
  p.soff.resize(n + m + 1);
  if (sig_base == 0) {
    memcpy(p.soff.data(), eb->sig_off + a, (n + 1) * 8);
  } else {
    for (uint64_t e = 0; e <= n; e++) p.soff[e] = eb->sig_off[a + e] - sig_base;
  }
  for (uint64_t i = 0; i < m; i++) p.soff[n + i + 1] = p.soff[n + i] + itx_str_len(*x, i0 + i, ITX_SIGNATURE);
  return BV_OK;
}

// Event.Verify's fold on the host (the small path; k_ev_compose otherwise)
void compose_host(const bv_event_itx_batch *x, const uint8_t *item_status, const uint8_t *force, bv_result *res,
                  bv_event_itx_out *out) {
  const uint64_t n = x->events.n_events;
  if (res->accept_bits) memset(res->accept_bits, 0, (n + 63) / 64 * 8);
  for (uint64_t e = 0; e < n; e++) {
    uint8_t st = item_status[e];
    uint32_t by = BV_EV_SELF;
    const uint64_t i0 = x->itx_start ? x->itx_start[e] : 0, i1 = x->itx_start ? x->itx_start[e + 1] : 0;
    for (uint64_t i = i0; i < i1; i++) {
      const uint8_t c = force[i] ? (uint8_t)BV_REF_PANIC : item_status[n + i];
      if (out && out->itx_status) out->itx_status[i] = c;
      if (by == BV_EV_SELF && c != BV_ACCEPT) {
        by = (uint32_t)(i - i0);
        st = c == BV_REJECT ? (uint8_t)BV_EV_ITX_INVALID : c;
      }
    }
    if (res->status) res->status[e] = st;
    if (out && out->decided_by) out->decided_by[e] = by;
    if (res->accept_bits && st == BV_ACCEPT) res->accept_bits[e >> 6] |= 1ull << (e & 63);
  }
}

// A batch the text entry would run on its one-launch small path (the same
// routing rule over the same item count and keys): every body, the events' and
// the ITXs', is built here (a batch with in-batch parents through hostdag.cpp,
// which leaves the bodies with their parents' hex spliced in), that path hashes
// them on the host (hostsha) and verifies the items in one launch, and the
// fold is done on the host.  *taken = false: the bulk pipeline's.
int small_route(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, bv_result *res,
                bv_event_itx_out *out, bool dag, const std::vector<uint32_t> &order,
                const std::vector<uint32_t> &level_off, const EvfPrep &p, bool *taken) {
  const std::vector<uint64_t> &koff = p.koff, &soff = p.soff;
  const std::vector<uint8_t> &kfix = p.kfix, &force = p.force;
  const std::vector<uint32_t> &ikey = p.ikey, &usrc = p.usrc;
  const bv_event_batch *eb = &x->events;
  const uint64_t n = eb->n_events, m = x->itx_start ? x->itx_start[n] : 0, N = n + m;
  const uint32_t n_keys = eb->n_keys;
  const uint64_t K = (uint64_t)n_keys + usrc.size();
  *taken = false;
  std::vector<uint64_t> moff(N + 1, 0);
  std::vector<uint8_t> bodies;
  uint32_t pp[2];
  if (dag) {
    std::vector<uint8_t> evdig(n * 32);
    dag_hash(x, f, order, level_off, bv_pool_parfor(ctx), ctx->dag_scratch, evdig.data());
    memcpy(moff.data(), ctx->dag_scratch.off.data(), (n + 1) * 8);
  } else {
    for (uint64_t e = 0; e < n; e++) moff[e + 1] = moff[e] + body_len(x, f, e, pp);
  }
  for (uint64_t i = 0; i < m; i++) moff[n + i + 1] = moff[n + i] + itx_body_len(*x, i);
  bodies.resize(moff[N] + 64);
  if (dag) {
    memcpy(bodies.data(), ctx->dag_scratch.bodies.data(), moff[n]);
  } else {
    for (uint64_t e = 0; e < n; e++) body_write(x, f, e, bodies.data() + moff[e]);
  }
  for (uint64_t i = 0; i < m; i++) {
    EvjMem o{bodies.data() + moff[n + i]};
    itx_body_emit(*x, i, o);
  }
  std::vector<uint8_t> kb(koff[K] + 64), text(soff[N] + 1);
  if (koff[n_keys]) memcpy(kb.data(), eb->key_bytes, koff[n_keys]);
  if (soff[n]) memcpy(text.data(), eb->sig_text, soff[n]);
  std::vector<uint32_t> item_msg(N), item_key(N);
  for (uint64_t e = 0; e < n; e++) item_msg[e] = (uint32_t)e, item_key[e] = eb->creator[e];
  for (size_t u = 0; u < usrc.size(); u++) {
    const uint64_t kl = koff[n_keys + u + 1] - koff[n_keys + u];
    if (kl) memcpy(kb.data() + koff[n_keys + u], kfix.data() + (size_t)usrc[u] * kItxKeyMax, kl);
  }
  for (uint64_t i = 0; i < m; i++) {
    item_msg[n + i] = (uint32_t)(n + i), item_key[n + i] = ikey[i];
    const uint64_t sl = soff[n + i + 1] - soff[n + i];
    if (sl) memcpy(text.data() + soff[n + i], itx_str_ptr(*x, i, ITX_SIGNATURE), sl);
  }
  bv_batch hb = {};
  hb.n_msgs = N;
  hb.msg_bytes = bodies.data();
  hb.msg_off = moff.data();
  hb.n_keys = (uint32_t)K;
  hb.key_bytes = kb.data();
  hb.key_off = koff.data();
  hb.n_items = N;
  hb.item_msg = item_msg.data();
  hb.item_key = item_key.data();
  const bv_sig_text htext{soff.data(), text.data()};
  if (!bv_small_batch(ctx, &hb, true)) return BV_OK;
  int rc = bv_validate_host_batch(ctx, &hb, true);
  if (rc != BV_OK) return rc;
  std::vector<uint8_t> h(N * 32), st(N);
  bv_result r2 = {h.data(), st.data(), nullptr};
  rc = bv_small_verify(ctx, &hb, &r2, &htext);
  if (rc != BV_OK) return rc;
  if (res->msg_hash) memcpy(res->msg_hash, h.data(), n * 32);
  if (out && out->itx_hash) memcpy(out->itx_hash, h.data() + n * 32, m * 32);
  compose_host(x, st.data(), force.data(), res, out);
  *taken = true;
  return BV_OK;
}

// What the entries check before anything runs, once over the whole batch (the
// group's too).  *route: EVF_RUN, or the fall-back the caller takes outside
// the lock: the batch has no ITX (bv_verify_events_itx) or no block signature
// (bv_verify_events_fields), and the entry that takes fragments validates it.
int evf_validate(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, int *route) {
  const bv_event_batch *eb = &x->events;
  const uint64_t n = eb->n_events;
  *route = EVF_RUN;
  if (eb->itx_off || eb->itx_json)
    return bv_fail(ctx, BV_E_ARGS, "events.itx_off / itx_json must be NULL (the ITXs come from fields)");
  if (n && !eb->sig_text) return bv_fail(ctx, BV_E_ARGS, "events.sig_text is required");
  if (f) {
    if (const char *why = check_bsig(f, ctx->pool)) return bv_fail(ctx, BV_E_ARGS, why);
    if (!n || !f->bsig_start[n]) {
      *route = EVF_NO_BSIG;
      return BV_OK;
    }
  }
  const bool itx_fields = !f || x->itx_start;  // (a fields batch may carry no ITX fields at all)
  if (itx_fields)
    if (const char *why = check_itx(x, ctx->pool)) return bv_fail(ctx, BV_E_ARGS, why);
  if (!f && x->itx_start[n] == 0) {
    *route = EVF_NO_ITX;
    return BV_OK;
  }
  return bv_validate_events(ctx, eb);
}

// (the fields entry asks bv_small_batch's own first question ahead of the bodies small_route builds for it:
// past small_max only a key-cache context can take the path)
bool small_candidate(bv_ctx *ctx, const bv_event_fields_batch *f, uint64_t N) {
  return ctx->small_path && N <= std::max(ctx->small_max, ctx->small_warm_max) &&
         (!f || N <= ctx->small_max || (ctx->flags & BV_F_KEY_CACHE));
}

int evf_launch(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, const bv_ev_shard &sh,
               const EvfPrep &p, const std::vector<uint32_t> *order, const std::vector<uint32_t> *level_off,
               bv_evf_call *call_p);

// f: the same batch with its block signatures as fields (x == &f->ev; at
// least one block signature), or null.  The batch is validated (evf_validate).
int verify_impl(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, bv_result *res,
                bv_event_itx_out *out, bv_evf_call &call) {
  const bv_event_batch *eb = &x->events;
  const uint64_t n = eb->n_events;
  const bool itx_fields = !f || x->itx_start;
  hipStream_t st = ctx->stream;
  ctx->timing = bv_timing{};
  ctx->last = st;

  // DAG levels over in-batch parents (refs point backwards: one pass), as bv_verify_events
  std::vector<uint32_t> order, level_off;
  const bool dag = memchr(eb->parent_kind, BV_PARENT_EVENT, 2 * n) != nullptr;
  if (dag) bv_dag_levels(*eb, order, level_off);

  EvfPrep p;
  int rc = evf_prep(ctx, x, itx_fields, 0, n, p);
  if (rc != BV_OK) return rc;
  if (small_candidate(ctx, f, n + p.m)) {
    bool taken = false;
    rc = small_route(ctx, x, f, res, out, dag, order, level_off, p, &taken);
    if (rc != BV_OK || taken) return rc;
  }
  // the bulk pipeline over the whole batch as one range with zero bases
  const bv_ev_shard whole{0, n, 0, eb->parent_hashes ? eb->n_parent_hashes : 0};
  rc = evf_launch(ctx, x, f, whole, p, dag ? &order : nullptr, &level_off, &call);
  if (rc != BV_OK) return rc;
  rc = bv_mark_done(ctx, st);
  if (rc != BV_OK) return rc;
  return bv_evf_finish(ctx, res, out, &call, true);
}

// The bulk pipeline over events [sh.a, sh.z) of a validated batch and the ITXs
// they own: everything up to the call's last enqueued command (the caller
// records the end with bv_mark_done and collects with bv_evf_finish), as
// bv_events_launch.  The single-context entries pass the whole batch (order:
// its in-batch DAG, if it has one); the group one shard per slot.  The range's
// slices are staged from where they lie in the caller's arrays and the values
// in them stay the whole batch's: the device subtracts the bases (EvjBases,
// ItxBases, BsigBases).  With every base zero the un-based kernels run.
int evf_launch(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, const bv_ev_shard &sh,
               const EvfPrep &p, const std::vector<uint32_t> *order, const std::vector<uint32_t> *level_off,
               bv_evf_call *call_p) {
  bv_host_call &call = call_p->host;
  int rc = BV_OK;
  hipStream_t st = ctx->stream;
  const uint64_t a = sh.a, n = sh.z - sh.a;  // the range's events: e below is range-local
  if (n == 0) return BV_OK;                  // (an empty shard launches nothing)
  const bv_event_batch whole_events = x->events;
  const bool itx_fields = !f || x->itx_start;
  const bool dag = order != nullptr;
  const uint64_t i0 = p.i0, m = p.m, N = n + m;
  call_p->n = n, call_p->m = m;
  const std::vector<uint64_t> &koff = p.koff, &soff = p.soff;
  const std::vector<uint8_t> &kfix = p.kfix, &force = p.force;
  const std::vector<uint32_t> &ikey = p.ikey, &usrc = p.usrc;
  const uint32_t n_keys = whole_events.n_keys;
  const uint64_t ev_key_len = whole_events.key_off[n_keys];
  const uint64_t K = (uint64_t)n_keys + usrc.size();
  const uint64_t key_len = koff[K];
  const uint64_t ev_text_len = soff[n], text_len = soff[N];

  // the bases, and the range's view of the caller's arrays (host pointers to its first elements)
  const uint64_t j0 = f ? f->bsig_start[a] : 0, nb = f ? f->bsig_start[sh.z] - j0 : 0;  // block signatures, as fields
  const bool bv_bytes = f && f->bsig_val_kind && nb && memchr(f->bsig_val_kind + j0, BV_BSIG_VAL_BYTES, nb);
  EvjBases bs = {};
  bs.ev = a;
  bs.tx = whole_events.tx_start[a];
  bs.txb = whole_events.tx_start[whole_events.n_events] ? whole_events.tx_off[bs.tx] : 0;
  bs.bsig = whole_events.bsig_off ? whole_events.bsig_off[a] : 0;
  bs.ph = sh.hash_lo;
  const ItxBases ib{i0, m ? x->itx_str_off[4 * i0] : 0};
  const BsigBases sb{j0, nb ? f->bsig_sig_off[j0] : 0, bv_bytes ? f->bsig_val_off[j0] : 0};
  const bool rebased = bs.ev || bs.tx || bs.txb || bs.bsig || bs.ph || ib.itx || ib.str || sb.bsig || sb.sig || sb.val;
  bv_event_itx_batch xv = *x;
  bv_event_fields_batch fv = {};
  if (f) fv = *f;
  {
    auto adv = [](auto *&q, uint64_t k) {
      if (q) q += k;
    };
    bv_event_batch &v = xv.events;
    v.n_events = n;
    adv(v.creator, a), adv(v.index, a), adv(v.timestamp, a);
    adv(v.parent_kind, 2 * a), adv(v.parent_ref, 2 * a);
    adv(v.parent_hashes, 32 * sh.hash_lo);
    adv(v.tx_start, a), adv(v.tx_off, bs.tx), adv(v.tx_bytes, bs.txb);
    adv(v.tx_list_nil, a), adv(v.tx_nil, bs.tx);
    adv(v.bsig_off, a), adv(v.bsig_json, bs.bsig);
    adv(v.sig_text, v.sig_off[a]);
    adv(xv.itx_start, a), adv(xv.itx_list_nil, a), adv(xv.itx_type, i0);
    adv(xv.itx_str_off, 4 * i0), adv(xv.itx_str, ib.str);
    adv(fv.bsig_start, a), adv(fv.bsig_list_nil, a), adv(fv.bsig_index, j0), adv(fv.bsig_sig_off, j0);
    adv(fv.bsig_sig, sb.sig), adv(fv.bsig_val_kind, j0), adv(fv.bsig_val_off, j0), adv(fv.bsig_val_bytes, sb.val);
  }
  const bv_event_batch *eb = &xv.events;  // (its values are the whole batch's: subtract the bases)
  const bv_event_itx_batch *xs = &xv;
  const bv_event_fields_batch *fs = f ? &fv : nullptr;

  // staging layout (pinned host and HBM)
  const uint64_t n_tx = eb->tx_start[n] - bs.tx, tx_len = n_tx ? eb->tx_off[n_tx] - bs.txb : 0;
  const uint64_t bsig_len = eb->bsig_off ? eb->bsig_off[n] - bs.bsig : 0;
  const uint64_t str_len = m ? xs->itx_str_off[4 * m] - ib.str : 0;
  const uint64_t bs_len = nb ? fs->bsig_sig_off[nb] - sb.sig : 0;
  const uint64_t bv_len = bv_bytes ? fs->bsig_val_off[nb] - sb.val : 0;
  const uint64_t n_ph = eb->parent_hashes ? sh.hash_hi - sh.hash_lo : 0;
  // The fields entry's bulk route, a batch of more than one chunk of events:
  // the arrays that are indexed by event (or by an event's transactions or
  // block signatures) cross in event-range slices, chunk by chunk, into the
  // same one-piece device layout, and each chunk's bodies are hashed and its
  // items verified while the next chunk crosses (as bv_verify_events' chunks).
  uint64_t chunk_ev = 1 << 17;
  if (const char *env = getenv("BV_FIELDS_CHUNK")) chunk_ev = std::max<uint64_t>(64, (strtoull(env, nullptr, 10) + 63) / 64 * 64);
  const bool chunked = f && !dag && n > chunk_ev;
  // The fields entry: a large array that lies in bv_host_alloc memory is not
  // copied into the staging block; the DMA engine reads it where it is (as
  // bv_verify_events does), and the staging runs around it and around the
  // sliced arrays cross as one copy each.  The ITX entry stages everything.
  StagePlan plan({f ? (size_t)256 << 10 : StagePolicy::kNever, true});
  plan.space[S_TX] = {eb->tx_start, bs.tx};
  plan.space[S_BS] = {f ? fs->bsig_start : nullptr, sb.bsig};
  const auto sl = [chunked](StageKind k) { return chunked ? k : StageKind{}; };  // sliced only on that route
  const StageKind k_ev = sl({S_ELEM, S_EV}), k_ev1 = sl({S_OFFS, S_EV}), k_tx = sl({S_ELEM, S_TX}), k_tx1 = sl({S_OFFS, S_TX});
  const StageKind k_bs = sl({S_ELEM, S_BS}), k_bs1 = sl({S_OFFS, S_BS}), k_txb = sl({S_BYTES, S_TX, eb->tx_off, bs.txb});
  const StageKind k_bsb = sl({S_BYTES, S_BS, f ? fs->bsig_sig_off : nullptr, sb.sig}),
                  k_bvb = sl({S_BYTES, S_BS, f ? fs->bsig_val_off : nullptr, sb.val});
  // (reserve: bytes the driver fills by hand, or that only the device writes)
  const size_t o_koff = plan.add(koff.data(), (K + 1) * 8), o_kb = plan.reserve(key_len, 64), keys_end = plan.total;
  const size_t o_soff = plan.add(soff.data(), (N + 1) * 8);  // the events' text, then the ITXs' (by hand) and the pad
  const size_t o_text = plan.add(eb->sig_text, ev_text_len, {}, 1, text_len - ev_text_len + 64), s_end = plan.total;
  const size_t o_ik = plan.reserve(N * 4);
  const size_t o_is = itx_fields ? plan.add(xs->itx_start, (n + 1) * 8, k_ev1, 8) : plan.reserve((n + 1) * 8);
  const size_t o_iln = plan.add(xs->itx_list_nil, n, k_ev, 1), o_ity = plan.add(xs->itx_type, m);
  const size_t o_iso = m ? plan.add(xs->itx_str_off, (4 * m + 1) * 8) : plan.reserve(8);
  const size_t o_istr = plan.add(xs->itx_str, str_len, {}, 1, 64), o_force = plan.add(force.data(), m);
  const bool bulk = !dag;  // the event fields cross only when the device builds the bodies
  const size_t o_ix = plan.add(eb->index, bulk ? n * 8 : 0, k_ev, 8), o_ts = plan.add(eb->timestamp, bulk ? n * 8 : 0, k_ev, 8);
  const size_t o_pk = plan.add(eb->parent_kind, bulk ? n * 2 : 0, k_ev, 2);
  const size_t o_pr = plan.add(eb->parent_ref, bulk ? n * 16 : 0, k_ev, 16);
  const size_t o_ph = plan.add(eb->parent_hashes, bulk ? n_ph * 32 : 0);
  const size_t o_txs = plan.add(eb->tx_start, bulk ? (n + 1) * 8 : 0, k_ev1, 8);
  const size_t o_txo = plan.add(eb->tx_off, bulk && n_tx ? (n_tx + 1) * 8 : 0, k_tx1, 8);
  const size_t o_txb = plan.add(eb->tx_bytes, bulk ? tx_len : 0, k_txb, 1, 64);
  const size_t o_tln = plan.add(eb->tx_list_nil, bulk ? n : 0, k_ev, 1), o_txn = plan.add(eb->tx_nil, bulk ? n_tx : 0, k_tx, 1);
  const size_t o_bo = plan.add(eb->bsig_off, bulk ? (n + 1) * 8 : 0), o_bj = plan.add(eb->bsig_json, bulk ? bsig_len : 0);
  const bool bf = bulk && f;
  const bv_event_fields_batch none = {}, &g = bf ? *fs : none;  // (no block-signature field crosses otherwise)
  // an array whose place does not depend on its presence: the bytes are reserved when it is absent
  const auto fld = [&](const void *src, size_t bytes, StageKind k, size_t unit, size_t pad = 0) {
    return src ? plan.add(src, bf ? bytes : 0, k, unit, pad) : plan.reserve(bf ? bytes : 0, pad);
  };
  const size_t o_fs = fld(g.bsig_start, (n + 1) * 8, k_ev1, 8), o_fln = plan.add(g.bsig_list_nil, n, k_ev, 1);
  const size_t o_fix = fld(g.bsig_index, nb * 8, k_bs, 8), o_fso = fld(g.bsig_sig_off, (nb + 1) * 8, k_bs1, 8);
  const size_t o_fsg = fld(g.bsig_sig, bs_len, k_bsb, 1, 64), o_fk = plan.add(g.bsig_val_kind, nb, k_bs, 1);
  const size_t o_fvo = plan.add(bv_bytes ? g.bsig_val_off : nullptr, (nb + 1) * 8, k_bs1, 8);
  const size_t o_fvb = fld(g.bsig_val_bytes, bv_len, k_bvb, 1, 64);
  const size_t in_end = plan.total;
  const size_t o_dig = plan.reserve(dag ? n * 32 : 0);  // (pinned side only: the host's digests)
  // device side only: k_ev_compose's outputs
  const size_t o_evst = plan.reserve(n), o_dby = plan.reserve(n * 4), o_bits = plan.reserve((n + 63) / 64 * 8);
  const size_t o_ist = plan.reserve(m), total = plan.total;

  if (bv_wait_all(ctx) != BV_OK) return BV_E_LAUNCH;  // previous calls' work buffers / staging
  HIPCHK(ctx->pin_in.ensure(total), BV_E_OOM, "alloc pinned staging");
  HIPCHK(ctx->d_in.ensure(total), BV_E_OOM, "alloc device staging");
  HIPCHK(ctx->ev_iota.ensure(N * 4), BV_E_OOM, "alloc item index");
  uint8_t *pin = (uint8_t *)ctx->pin_in.p, *dev = ctx->d_in.as<uint8_t>();
  hipStream_t cs = bv_copy_stream(ctx);
  if (!cs) return bv_fail(ctx, BV_E_NODEVICE, "copy stream");
  hipEvent_t *ev = ctx->S().ev;
  HIPCHK(hipEventRecord(ev[E_CALL], cs), BV_E_LAUNCH, "event");
  plan.mark_direct(bv_is_pinned);
  // each phase as one piece: the planned arrays into the staging block, then the copies in layout order
  auto h2d = [&](size_t b0, size_t b1) { return bv_stage_range(ctx, plan, b0, b1, b1 - b0); };

  // the keys
  if (ev_key_len) memcpy(pin + o_kb, eb->key_bytes, ev_key_len);  // (always staged: the key cache reads them here)
  for (size_t u = 0; u < usrc.size(); u++) {
    const uint64_t ka = koff[n_keys + u], len = koff[n_keys + u + 1] - ka;
    if (len) memcpy(pin + o_kb + ka, kfix.data() + (size_t)usrc[u] * kItxKeyMax, len);
  }
  memset(pin + o_kb + key_len, 0, 64);
  if ((rc = h2d(0, keys_end)) != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_KREADY], cs), BV_E_LAUNCH, "event");

  // item e: event e under its creator's key; item n + i: ITX i under its key's slot
  uint32_t *h_ik = (uint32_t *)(pin + o_ik);
  memcpy(h_ik, eb->creator, n * 4);
  for (uint64_t i = 0; i < m; i++) h_ik[n + i] = ikey[i];

  bv_batch vb = {};
  vb.n_msgs = N;
  vb.n_keys = (uint32_t)K;
  vb.key_bytes = dev + o_kb;
  vb.key_off = (const uint64_t *)(dev + o_koff);
  vb.n_items = N;
  vb.item_msg = ctx->ev_iota.as<uint32_t>();
  vb.item_key = (const uint32_t *)(dev + o_ik);
  bool kc = false;
  if (K <= kKcMaxBatchKeys) {  // (else `st` does not wait for the keys either)
    rc = bv_kc_host_step(ctx, pin + o_kb, (const uint64_t *)(pin + o_koff), vb, h_ik, st, &kc);
    if (rc != BV_OK) return rc;
  }

  // the signature text: r, s and pre of every item decoded on the device
  if (m) par(ctx->pool, m, 4096, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      const uint64_t len = soff[n + i + 1] - soff[n + i];
      if (len) memcpy(pin + o_text + soff[n + i], itx_str_ptr(*x, i0 + i, ITX_SIGNATURE), len);
    }
    return true;
  });
  memset(pin + o_text + text_len, 0, 64);
  if ((rc = h2d(keys_end, s_end)) != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_SREADY], cs), BV_E_LAUNCH, "event");
  bv_sig_out so;
  rc = bv_sig_decode_on_device(ctx, N, (const uint64_t *)(dev + o_soff), dev + o_text, ev[E_SREADY], &so);
  if (rc != BV_OK) return rc;
  vb.r_be = so.r, vb.s_be = so.s, vb.pre = so.pre;
  rc = bv_run_keys(ctx, &vb, ev[E_KREADY], ev[E_SREADY], kc);
  if (rc != BV_OK) return rc;

  // the fields (and the pads the serialisers' last reads run into)
  memset(pin + o_istr + str_len, 0, 64);
  if (bulk) memset(pin + o_txb + tx_len, 0, 64);
  if (bf) memset(pin + o_fsg + bs_len, 0, 64), memset(pin + o_fvb + bv_len, 0, 64);
  if ((rc = h2d(s_end, in_end)) != BV_OK) return rc;
  HIPCHK(hipEventRecord(ev[E_SMALL], cs), BV_E_LAUNCH, "event");
  HIPCHK(hipStreamWaitEvent(st, ev[E_SMALL], 0), BV_E_LAUNCH, "join");
  HIPCHK(hipStreamWaitEvent(st, ev[E_SDEC], 0), BV_E_LAUNCH, "join decoded signatures");
  HIPCHK(bvk::iota(st, N, ctx->ev_iota.as<uint32_t>()), BV_E_LAUNCH, "k_iota");
  if (!itx_fields)  // no itx_start crossed: k_ev_compose's view of it (no event owns an ITX) is set on the device
    HIPCHK(hipMemsetAsync(dev + o_is, 0, (n + 1) * 8, st), BV_E_LAUNCH, "zero itx_start");
  HIPCHK(hipEventRecord(ev[E_FORK], st), BV_E_LAUNCH, "event");

  // the same batch over device pointers (the serialisers read nothing else)
  bv_event_itx_batch dx = {};
  dx.events.n_events = n;
  dx.events.n_keys = n_keys;
  dx.events.key_off = (const uint64_t *)(dev + o_koff);  // (the creators' keys lead the combined array)
  dx.events.key_bytes = dev + o_kb;
  dx.events.creator = (const uint32_t *)(dev + o_ik);
  dx.itx_start = itx_fields ? (const uint64_t *)(dev + o_is) : nullptr;
  dx.itx_list_nil = x->itx_list_nil ? dev + o_iln : nullptr;
  dx.itx_type = dev + o_ity;
  dx.itx_str_off = (const uint64_t *)(dev + o_iso);
  dx.itx_str = dev + o_istr;
  if (bulk) {
    bv_event_batch &d = dx.events;
    d.index = (const int64_t *)(dev + o_ix);
    d.timestamp = (const int64_t *)(dev + o_ts);
    d.parent_kind = dev + o_pk;
    d.parent_ref = (const uint64_t *)(dev + o_pr);
    d.n_parent_hashes = n_ph;
    d.parent_hashes = n_ph ? dev + o_ph : nullptr;
    d.tx_start = (const uint64_t *)(dev + o_txs);
    d.tx_off = n_tx ? (const uint64_t *)(dev + o_txo) : nullptr;
    d.tx_bytes = dev + o_txb;
    d.tx_list_nil = eb->tx_list_nil ? dev + o_tln : nullptr;
    d.tx_nil = eb->tx_nil && n_tx ? dev + o_txn : nullptr;
    d.bsig_off = eb->bsig_off ? (const uint64_t *)(dev + o_bo) : nullptr;
    d.bsig_json = dev + o_bj;
  }
  bv_event_fields_batch df = {};
  if (bf) {
    df.ev = dx;
    df.bsig_start = (const uint64_t *)(dev + o_fs);
    df.bsig_list_nil = f->bsig_list_nil ? dev + o_fln : nullptr;
    df.bsig_index = (const int64_t *)(dev + o_fix);
    df.bsig_sig_off = (const uint64_t *)(dev + o_fso);
    df.bsig_sig = dev + o_fsg;
    df.bsig_val_kind = f->bsig_val_kind ? dev + o_fk : nullptr;
    df.bsig_val_off = bv_bytes ? (const uint64_t *)(dev + o_fvo) : nullptr;
    df.bsig_val_bytes = dev + o_fvb;
  }

  bv_item_pipe pipe{ctx, &vb, {}, st, kc};
  rc = bv_out_bufs(ctx, &vb, nullptr, nullptr, nullptr, true, &pipe.o);
  if (rc != BV_OK) return rc;
  uint32_t *dig = pipe.o.dig;
  // events [c0, c1) of the range: the batch's [a + c0, a + c1) to a rebased kernel
  const auto hash_fields = [&](uint64_t c0, uint64_t c1) {
    return rebased ? bvk::ev_body_hash_fields_rb(st, df, a + c0, a + c1, bs, ib, sb, dig)
                   : bvk::ev_body_hash_fields(st, df, c0, c1, dig);
  };
  HIPCHK(rebased ? bvk::itx_body_hash_rb(st, dx, m, n, ib, dig) : bvk::itx_body_hash(st, dx, m, n, dig), BV_E_LAUNCH,
         "k_itx_body_hash");
  if (chunked) {
    for (uint64_t c0 = 0; c0 < n; c0 += chunk_ev) {
      const uint64_t c1 = std::min(n, c0 + chunk_ev);
      // pinned arrays' slices by DMA from where they lie, the rest into pinned memory, then its DMA
      if ((rc = bv_stage_slices(ctx, plan, c0, c1)) != BV_OK) return rc;
      hipEvent_t landed = ctx->chunk_ev[(c0 / chunk_ev) % ctx->chunk_ev.size()];
      HIPCHK(hipEventRecord(landed, cs), BV_E_LAUNCH, "event");
      HIPCHK(hipStreamWaitEvent(st, landed, 0), BV_E_LAUNCH, "join chunk");
      HIPCHK(hash_fields(c0, c1), BV_E_LAUNCH, "k_ev_body_hash_fields");
      if (c1 < n && (rc = pipe.upto(c1)) != BV_OK) return rc;  // (the last chunk's items: pipe.finish below)
    }
  } else if (bf) {
    HIPCHK(hash_fields(0, n), BV_E_LAUNCH, "k_ev_body_hash_fields");
  } else if (bulk) {
    HIPCHK(rebased ? bvk::ev_body_hash_itx_rb(st, dx, a, a + n, bs, ib, dig) : bvk::ev_body_hash_itx(st, dx, 0, n, dig),
           BV_E_LAUNCH, "k_ev_body_hash_itx");
  } else {
    // the host's part, beside the device's key / s^-1 work and the ITX hashing
    dag_hash(x, f, *order, *level_off, bv_pool_parfor(ctx), ctx->dag_scratch, pin + o_dig);
    HIPCHK(hipMemcpyAsync(dig, pin + o_dig, n * 32, hipMemcpyHostToDevice, cs), BV_E_LAUNCH, "h2d digests");
  }
  HIPCHK(hipEventRecord(ev[E_STAGED], cs), BV_E_LAUNCH, "event");
  call.ms_prep = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - call.t0).count();
  HIPCHK(hipStreamWaitEvent(st, ev[E_STAGED], 0), BV_E_LAUNCH, "join digests");
  HIPCHK(hipEventRecord(ev[E_SHA], st), BV_E_LAUNCH, "event");
  HIPCHK(hipEventRecord(ev[E_HASHED], st), BV_E_LAUNCH, "event");
  rc = pipe.finish();  // every item: the events' and the ITXs'
  if (rc != BV_OK) return rc;
  const uint64_t *d_is = (const uint64_t *)(dev + o_is);
  HIPCHK(ib.itx ? bvk::ev_compose_rb(st, n, d_is, ib.itx, pipe.o.status, dev + o_force, dev + o_evst,
                                     (uint32_t *)(dev + o_dby), (uint64_t *)(dev + o_bits), dev + o_ist)
                : bvk::ev_compose(st, n, d_is, pipe.o.status, dev + o_force, dev + o_evst, (uint32_t *)(dev + o_dby),
                                  (uint64_t *)(dev + o_bits), dev + o_ist),
         BV_E_LAUNCH, "k_ev_compose");
  call_p->d_bits = dev + o_bits;

  // results: the digests (events, then ITXs), then k_ev_compose's outputs as they lie in HBM, in one copy
  const size_t p_st = align256(N * 32), p_bits = p_st + (o_bits - o_evst), p_dby = p_st + (o_dby - o_evst),
               p_ist = p_st + (o_ist - o_evst), fold_len = o_ist + align256(m) - o_evst;
  HIPCHK(ctx->pin_out.ensure(p_st + fold_len + 256), BV_E_OOM, "alloc pinned results");
  uint8_t *pout = (uint8_t *)ctx->pin_out.p;
  call.pout = pout;
  call.o_st = p_st;
  call.o_bits = p_bits;
  HIPCHK(hipMemcpyAsync(pout, dig, N * 32, hipMemcpyDeviceToHost, st), BV_E_LAUNCH, "d2h digests");
  HIPCHK(hipMemcpyAsync(pout + p_st, dev + o_evst, fold_len, hipMemcpyDeviceToHost, st), BV_E_LAUNCH,
         "d2h statuses, bits, decided_by");
  HIPCHK(hipEventRecord(ev[E_OUT], st), BV_E_LAUNCH, "event");
  call_p->p_ist = p_ist, call_p->p_dby = p_dby;
  return BV_OK;
}

void lens_scan(uint64_t n, uint64_t *off) {
  for (uint64_t i = 0; i < n; i++) off[i + 1] += off[i];
}

}  // namespace

int bv_evf_finish(bv_ctx *ctx, bv_result *res, bv_event_itx_out *out, bv_evf_call *call, bool bits_out) {
  const uint64_t n = call->n, m = call->m;
  bv_batch sizes = {};
  sizes.n_msgs = n;
  sizes.n_items = n;
  const int rc = bv_host_finish(ctx, &sizes, res, &call->host, bits_out);
  if (rc != BV_OK) return rc;
  const uint8_t *pout = call->host.pout;
  if (out) {
    if (out->itx_hash && m) memcpy(out->itx_hash, pout + n * 32, m * 32);
    if (out->itx_status && m) memcpy(out->itx_status, pout + call->p_ist, m);
    if (out->decided_by) memcpy(out->decided_by, pout + call->p_dby, n * 4);
  }
  return BV_OK;
}

int bv_evf_validate(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, int *route) {
  return evf_validate(ctx, x, f, route);
}

// (A candidate batch is prepared whole here, and again shard by shard when
// small_route declines it: a second pass over at most small_warm_max items.)
int bv_evf_try_small(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, bv_result *res,
                     bv_event_itx_out *out, bool *taken) {
  const uint64_t n = x->events.n_events;
  const bool itx_fields = !f || x->itx_start;
  *taken = false;
  if (!small_candidate(ctx, f, n + (itx_fields ? x->itx_start[n] : 0))) return BV_OK;
  ctx->timing = bv_timing{};
  ctx->last = ctx->stream;
  EvfPrep p;
  const int rc = evf_prep(ctx, x, itx_fields, 0, n, p);
  if (rc != BV_OK) return rc;
  return small_route(ctx, x, f, res, out, false, {}, {}, p, taken);
}

int bv_evf_launch(bv_ctx *ctx, const bv_event_itx_batch *x, const bv_event_fields_batch *f, const bv_ev_shard &sh,
                  bv_evf_call *call) {
  ctx->timing = bv_timing{};
  ctx->last = ctx->stream;
  if (sh.z == sh.a) return BV_OK;
  EvfPrep p;  // the shard's ITX keys and signature text, on this ctx's pool
  const int rc = evf_prep(ctx, x, !f || x->itx_start, sh.a, sh.z, p);
  return rc == BV_OK ? evf_launch(ctx, x, f, sh, p, nullptr, nullptr, call) : rc;
}

// A batch without ITXs through the entry that takes fragments (`verify_events`:
// bv_verify_events, or the group's): a nil list as the empty fragment (null)
// and an empty non-nil one as "[]"
int bv_evf_no_itx(const bv_event_itx_batch *x, bv_result *res, bv_event_itx_out *out,
                  const std::function<int(const bv_event_batch *, bv_result *)> &verify_events) {
  bv_event_batch evb = x->events;
  const uint64_t n = evb.n_events;
  std::vector<uint64_t> frag_off;
  std::vector<uint8_t> frag;
  const bool all_nil = n == 0 || (x->itx_list_nil && !memchr(x->itx_list_nil, 0, n));
  if (!all_nil) {
    frag_off.resize(n + 1);
    frag_off[0] = 0;
    for (uint64_t e = 0; e < n; e++) frag_off[e + 1] = frag_off[e] + (itx_list_is_nil(*x, e) ? 0 : 2);
    frag.resize(frag_off[n]);
    for (uint64_t i = 0; i < frag.size(); i += 2) frag[i] = '[', frag[i + 1] = ']';
    evb.itx_off = frag_off.data();
    evb.itx_json = frag.data();
  }
  const int rc = verify_events(&evb, res);
  if (rc == BV_OK && out && out->decided_by) memset(out->decided_by, 0xFF, n * 4);  // BV_EV_SELF
  return rc;
}

extern "C" int bv_verify_events_itx(bv_ctx *ctx, const bv_event_itx_batch *x, bv_result *res, bv_event_itx_out *out) {
  if (!ctx || !x || !res) return BV_E_ARGS;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
    bv_evf_call call;
    call.host.t0 = std::chrono::steady_clock::now();
    int route = EVF_RUN;
    int rc = evf_validate(ctx, x, nullptr, &route);
    if (rc == BV_OK && route == EVF_RUN) rc = verify_impl(ctx, x, nullptr, res, out, call);
    if (rc != BV_OK) return bv_drain(ctx, ctx->stream, rc);
    if (route == EVF_RUN) return BV_OK;
  }
  // no ITX at all: bv_verify_events over the same events
  return bv_evf_no_itx(x, res, out, [ctx](const bv_event_batch *eb, bv_result *r) { return bv_verify_events(ctx, eb, r); });
}

extern "C" int bv_itx_body_lens(const bv_event_itx_batch *x, uint64_t *off) {
  if (!x || !off) return BV_E_ARGS;
  if (check_itx(x, nullptr)) return BV_E_ARGS;
  const uint64_t m = x->itx_start[x->events.n_events];
  off[0] = 0;
  for (uint64_t i = 0; i < m; i++) off[i + 1] = itx_body_len(*x, i);
  lens_scan(m, off);
  return BV_OK;
}

extern "C" int bv_itx_bodies(const bv_event_itx_batch *x, const uint64_t *off, uint8_t *out) {
  if (!x || !off) return BV_E_ARGS;
  if (check_itx(x, nullptr)) return BV_E_ARGS;
  const uint64_t m = x->itx_start[x->events.n_events];
  for (uint64_t i = 0; i < m; i++)
    if (off[i] > off[i + 1] || off[i + 1] - off[i] < itx_body_len(*x, i)) return BV_E_ARGS;
  if (m && off[m] > off[0] && !out) return BV_E_ARGS;
  for (uint64_t i = 0; i < m; i++) {
    EvjMem o{out + off[i]};
    itx_body_emit(*x, i, o);
  }
  return BV_OK;
}

extern "C" int bv_event_itx_body_lens(const bv_event_itx_batch *x, uint64_t *off) {
  if (!x || !off) return BV_E_ARGS;
  if (bv_check_event_fields(&x->events, nullptr, false) || check_itx(x, nullptr)) return BV_E_ARGS;
  const uint64_t n = x->events.n_events;
  off[0] = 0;
  uint32_t pp[2];
  for (uint64_t e = 0; e < n; e++) off[e + 1] = evj_len(*x, e, pp);
  lens_scan(n, off);
  return BV_OK;
}

extern "C" int bv_event_itx_bodies(const bv_event_itx_batch *x, const uint64_t *off, uint8_t *out) {
  if (!x || !off) return BV_E_ARGS;
  if (bv_check_event_fields(&x->events, nullptr, false) || check_itx(x, nullptr)) return BV_E_ARGS;
  const uint64_t n = x->events.n_events;
  uint32_t pp[2];
  for (uint64_t e = 0; e < n; e++)
    if (off[e] > off[e + 1] || off[e + 1] - off[e] < evj_len(*x, e, pp)) return BV_E_ARGS;
  if (n && off[n] > off[0] && !out) return BV_E_ARGS;
  for (uint64_t e = 0; e < n; e++) evj_write(*x, e, out + off[e]);
  return BV_OK;
}

// nil -> the empty fragment (null), an empty non-nil list -> "[]": what an
// entry that takes fragments needs for a member without elements.  nil[e] != 0:
// event e's list is nil; a NULL array: every list is (null_is_nil) or none is.
// Leaves *o / *j NULL when every list is nil.
static void empty_list_fragments(uint64_t n, const uint8_t *nil, bool null_is_nil, std::vector<uint64_t> &off,
                                 std::vector<uint8_t> &json, const uint64_t **o, const uint8_t **j) {
  if (!n || (nil ? !memchr(nil, 0, n) : null_is_nil)) return;
  off.resize(n + 1);
  off[0] = 0;
  for (uint64_t e = 0; e < n; e++) off[e + 1] = off[e] + (nil && nil[e] ? 0 : 2);
  json.resize(off[n]);
  for (uint64_t i = 0; i < json.size(); i += 2) json[i] = '[', json[i + 1] = ']';
  *o = off.data();
  *j = json.data();
}

// A fields batch without block signatures through the entry that takes
// fragments, over the same events with nil / "[]" fragments (`verify_itx`,
// `verify_events`: bv_verify_events_itx and bv_verify_events, or the group's)
int bv_evf_no_bsig(const bv_event_fields_batch *f, bv_result *res, bv_event_itx_out *out,
                   const std::function<int(const bv_event_itx_batch *, bv_result *, bv_event_itx_out *)> &verify_itx,
                   const std::function<int(const bv_event_batch *, bv_result *)> &verify_events) {
  const uint64_t n = f->ev.events.n_events;
  std::vector<uint64_t> boff, ioff;
  std::vector<uint8_t> bjson, ijson;
  bv_event_itx_batch xi = f->ev;
  empty_list_fragments(n, f->bsig_list_nil, false, boff, bjson, &xi.events.bsig_off, &xi.events.bsig_json);
  if (xi.itx_start) return verify_itx(&xi, res, out);
  empty_list_fragments(n, f->ev.itx_list_nil, true, ioff, ijson, &xi.events.itx_off, &xi.events.itx_json);
  const int rc = verify_events(&xi.events, res);
  if (rc == BV_OK && out && out->decided_by) memset(out->decided_by, 0xFF, n * 4);  // BV_EV_SELF
  return rc;
}

extern "C" int bv_verify_events_fields(bv_ctx *ctx, const bv_event_fields_batch *f, bv_result *res,
                                       bv_event_itx_out *out) {
  if (!ctx || !f || !res) return BV_E_ARGS;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device), BV_E_NODEVICE, "hipSetDevice");
    bv_evf_call call;
    call.host.t0 = std::chrono::steady_clock::now();
    int route = EVF_RUN;
    int rc = evf_validate(ctx, &f->ev, f, &route);
    if (rc == BV_OK && route == EVF_RUN) rc = verify_impl(ctx, &f->ev, f, res, out, call);
    if (rc != BV_OK) return bv_drain(ctx, ctx->stream, rc);
    if (route == EVF_RUN) return BV_OK;
  }
  // no block signature at all: the entry that takes fragments
  return bv_evf_no_bsig(
      f, res, out,
      [ctx](const bv_event_itx_batch *xi, bv_result *r, bv_event_itx_out *o) { return bv_verify_events_itx(ctx, xi, r, o); },
      [ctx](const bv_event_batch *eb, bv_result *r) { return bv_verify_events(ctx, eb, r); });
}

// The fields the serialiser reads, without a context
static const char *check_fields_host(const bv_event_fields_batch *f) {
  if (const char *why = bv_check_event_fields(&f->ev.events, nullptr, false)) return why;
  if (f->ev.events.itx_off || f->ev.events.itx_json) return "fragment";
  if (f->ev.itx_start)
    if (const char *why = check_itx(&f->ev, nullptr)) return why;
  return check_bsig(f, nullptr);
}

extern "C" int bv_event_fields_body_lens(const bv_event_fields_batch *f, uint64_t *off) {
  if (!f || !off) return BV_E_ARGS;
  if (check_fields_host(f)) return BV_E_ARGS;
  const uint64_t n = f->ev.events.n_events;
  off[0] = 0;
  uint32_t pp[2];
  for (uint64_t e = 0; e < n; e++) off[e + 1] = evj_len(*f, e, pp);
  lens_scan(n, off);
  return BV_OK;
}

extern "C" int bv_event_fields_bodies(const bv_event_fields_batch *f, const uint64_t *off, uint8_t *out) {
  if (!f || !off) return BV_E_ARGS;
  if (check_fields_host(f)) return BV_E_ARGS;
  const uint64_t n = f->ev.events.n_events;
  uint32_t pp[2];
  for (uint64_t e = 0; e < n; e++)
    if (off[e] > off[e + 1] || off[e + 1] - off[e] < evj_len(*f, e, pp)) return BV_E_ARGS;
  if (n && off[n] > off[0] && !out) return BV_E_ARGS;
  for (uint64_t e = 0; e < n; e++) evj_write(*f, e, out + off[e]);
  return BV_OK;
}
