// ASan + UBSan fuzz driver of the whole-event serialiser
// (babble_amd/csrc/bsigjson.h): random field batches in exactly-sized heap
// arrays (so any read past an array's end is reported), with and without ITX
// fields, every Validator kind and base64 tail; evj_len and bsig_elem_len
// against the bytes their emit functions write into an exactly-sized body,
// the streaming SHA sink (a 25-word row on the stack) over the same fields,
// the in-batch parents' positions; then the same batch with one field
// malformed at a time, through bsig_check (the BV_E_ARGS table of
// bv_verify_events_fields): every case must be refused, with its own text, and
// nothing may be read past an array on the way.  Stand-alone (its own main),
// host code only; run by tests/test_event_fields.py as a subprocess.
// Every batch is refused in every way of the table (15 texts), each round.
//   fieldsfuzz <seed> <rounds>   prints "ok <bodies> <bytes> <refusals>" or aborts
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/bsigjson.h"

namespace {
uint64_t g_state;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

struct CountSink {
  uint8_t *p, *end;
  void put(uint8_t c) {
    if (p >= end) {
      fprintf(stderr, "an emit function wrote past its length function\n");
      abort();
    }
    *p++ = c;
  }
};

uint8_t fuzz_byte() {
  static const uint8_t hot[] = {0x00, 0x09, 0x0A, 0x0D, 0x1F, 0x22, 0x26, 0x3C, 0x3E, 0x5C, 0x7F, 0x80, 0x8F, 0x90,
                                0x9F, 0xA0, 0xA8, 0xA9, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE2, 0xED, 0xEF, 0xF0,
                                0xF4, 0xF5, 0xFF, '0', '9', 'a', 'F', 'z', '|'};
  return below(3) ? hot[below(sizeof hot)] : (uint8_t)rnd();
}

template <class EmitFn>
uint64_t check(uint64_t len, const EmitFn &emit, const char *what) {
  std::unique_ptr<uint8_t[]> body(new uint8_t[len ? len : 1]);
  CountSink sink{body.get(), body.get() + len};
  emit(sink);
  if (sink.p != sink.end) {
    fprintf(stderr, "%s: emitted %zu bytes, the length function says %llu\n", what, (size_t)(sink.p - body.get()),
            (unsigned long long)len);
    exit(1);
  }
  uint32_t row[25], dig[8];  // the device's sink over the same fields
  EvjSha o = evj_sha_begin(row);
  emit(o);
  if ((uint64_t)o.nblk * 64 + o.n != len) {
    fprintf(stderr, "%s: the SHA sink took another byte count\n", what);
    exit(1);
  }
  evj_sha_finish(o, dig);
  return len;
}

bool mono(const uint64_t *off, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (off[i] > off[i + 1]) return false;
  return true;
}

std::set<std::string> g_refused;
void refuse(const bv_event_fields_batch &f, const char *want) {
  const char *why = bsig_check(f, mono);
  if (!why || strcmp(why, want) != 0) {
    fprintf(stderr, "expected a refusal \"%s\", got \"%s\"\n", want, why ? why : "(accepted)");
    exit(1);
  }
  g_refused.insert(why);
}
}  // namespace

int main(int argc, char **argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 50;
  uint64_t n_bodies = 0, n_bytes = 0;
  for (int r = 0; r < rounds; r++) {
    const uint64_t n = 2 + below(9);
    std::vector<int64_t> ix(n), ts(n), bix;
    std::vector<uint32_t> cr(n);
    std::vector<uint8_t> pk(2 * n), ph, kb, txb, tln, txn, iln, ity, str, bln, bsg, bk, bvb;
    std::vector<uint64_t> pr(2 * n), koff{0}, txs{0}, txo{0}, is{0}, so{0}, bs{0}, bso{0}, bvo{0}, owner;
    const uint32_t n_keys = 1 + (uint32_t)below(3);
    for (uint32_t k = 0; k < n_keys; k++) {
      const uint64_t len = below(4) ? 65 : below(70);
      for (uint64_t i = 0; i < len; i++) kb.push_back((uint8_t)rnd());
      koff.push_back(kb.size());
    }
    const bool itx_fields = below(3) != 0;
    for (uint64_t e = 0; e < n; e++) {
      ix[e] = below(2) ? (int64_t)rnd() : (int64_t)below(100);
      ts[e] = below(2) ? (int64_t)rnd() : (int64_t)below(100);
      cr[e] = (uint32_t)below(n_keys);
      for (int p = 0; p < 2; p++) {
        const uint64_t kind = e ? below(3) : below(2);
        pk[2 * e + p] = (uint8_t)kind;
        pr[2 * e + p] = 0;
        if (kind == BV_PARENT_HASH) {
          pr[2 * e + p] = ph.size() / 32;
          for (int i = 0; i < 32; i++) ph.push_back((uint8_t)rnd());
        } else if (kind == BV_PARENT_EVENT) {
          pr[2 * e + p] = below(e);
        }
      }
      const bool list_nil = below(5) == 0;
      tln.push_back(list_nil);
      const uint64_t nt = list_nil ? 0 : below(4);
      for (uint64_t t = 0; t < nt; t++) {
        const bool nil = below(6) == 0;
        const uint64_t len = nil ? 0 : below(90);
        for (uint64_t i = 0; i < len; i++) txb.push_back((uint8_t)rnd());
        txo.push_back(txb.size());
        txn.push_back(nil);
      }
      txs.push_back(txo.size() - 1);
      const bool inil = below(4) == 0;
      iln.push_back(inil);
      const uint64_t ni = inil || !itx_fields ? 0 : below(3);
      for (uint64_t i = 0; i < ni; i++) {
        ity.push_back((uint8_t)rnd());
        for (int k = 0; k < 4; k++) {
          const uint64_t len = below(3) ? below(12) : below(160);
          for (uint64_t j = 0; j < len; j++) str.push_back(fuzz_byte());
          so.push_back(str.size());
        }
      }
      is.push_back(ity.size());
      // the block signatures: nil / empty / a few; Index over the whole int64
      // range, the Signature a random string, every Validator kind
      // (event 0 always carries two or more, the first with a non-empty Signature: every refusal below applies
      // to every batch)
      const bool bnil = e ? below(4) == 0 : false;
      bln.push_back(bnil);
      const uint64_t nbs = bnil ? 0 : e ? below(4) : 2 + below(2);
      for (uint64_t j = 0; j < nbs; j++) {
        static const int64_t edge[] = {0, -1, INT64_MAX, INT64_MIN, 9, 10, -10};
        bix.push_back(below(2) ? edge[below(7)] : (int64_t)rnd());
        const uint64_t len = (below(3) ? below(12) : below(200)) + (bix.size() == 1 ? 1 : 0);
        for (uint64_t i = 0; i < len; i++) bsg.push_back(below(2) ? fuzz_byte() : (uint8_t)('0' + below(10)));
        bso.push_back(bsg.size());
        const uint8_t kind = (uint8_t)below(3);
        bk.push_back(kind);
        const uint64_t vl = kind == BV_BSIG_VAL_BYTES ? (below(2) ? below(5) : 62 + below(6)) : 0;
        for (uint64_t i = 0; i < vl; i++) bvb.push_back((uint8_t)rnd());
        bvo.push_back(bvb.size());
        owner.push_back(e);
      }
      bs.push_back(bix.size());
    }
    auto p_ix = exact(ix), p_ts = exact(ts), p_bix = exact(bix);
    auto p_cr = exact(cr);
    auto p_pk = exact(pk), p_ph = exact(ph), p_kb = exact(kb), p_txb = exact(txb), p_tln = exact(tln),
         p_txn = exact(txn), p_iln = exact(iln), p_ity = exact(ity), p_str = exact(str), p_bln = exact(bln),
         p_bsg = exact(bsg), p_bk = exact(bk), p_bvb = exact(bvb);
    auto p_pr = exact(pr), p_koff = exact(koff), p_txs = exact(txs), p_txo = exact(txo), p_is = exact(is),
         p_so = exact(so), p_bs = exact(bs), p_bso = exact(bso), p_bvo = exact(bvo);
    bv_event_fields_batch f = {};
    bv_event_batch &b = f.ev.events;
    b.n_events = n, b.n_keys = n_keys;
    b.key_bytes = p_kb.get(), b.key_off = p_koff.get(), b.creator = p_cr.get();
    b.index = p_ix.get(), b.timestamp = p_ts.get();
    b.parent_kind = p_pk.get(), b.parent_ref = p_pr.get();
    b.n_parent_hashes = ph.size() / 32, b.parent_hashes = p_ph.get();
    b.tx_start = p_txs.get(), b.tx_off = p_txo.get(), b.tx_bytes = p_txb.get();
    b.tx_list_nil = below(4) ? p_tln.get() : nullptr;
    b.tx_nil = below(4) ? p_txn.get() : nullptr;
    if (itx_fields) {
      f.ev.itx_start = p_is.get();
      f.ev.itx_type = p_ity.get();
      f.ev.itx_str_off = p_so.get();
      f.ev.itx_str = p_str.get();
    }
    f.ev.itx_list_nil = below(4) ? p_iln.get() : nullptr;
    f.bsig_start = p_bs.get();
    f.bsig_list_nil = below(4) ? p_bln.get() : nullptr;
    f.bsig_index = p_bix.get();
    f.bsig_sig_off = p_bso.get();
    f.bsig_sig = p_bsg.get();
    const bool all_creator = std::all_of(bk.begin(), bk.end(), [](uint8_t k) { return k == BV_BSIG_VAL_CREATOR; });
    f.bsig_val_kind = all_creator && below(2) ? nullptr : p_bk.get();
    f.bsig_val_off = p_bvo.get();
    f.bsig_val_bytes = p_bvb.get();
    if (const char *why = bsig_check(f, mono)) {
      fprintf(stderr, "a well-formed batch was refused: %s\n", why);
      return 1;
    }
    const uint64_t nb = bix.size();
    for (uint64_t j = 0; j < nb; j++) {
      n_bytes += check(bsig_elem_len(f, owner[j], j), [&](auto &o) { bsig_elem_emit(f, owner[j], j, o); }, "bsig_elem");
      n_bodies++;
    }
    for (uint64_t e = 0; e < n; e++) {
      uint32_t pp[2];
      const uint64_t len = evj_len(f, e, pp);
      n_bytes += check(len, [&](auto &o) { evj_emit(f, e, o); }, "event body");
      std::unique_ptr<uint8_t[]> body(new uint8_t[len]);
      evj_write(f, e, body.get());
      for (int p = 0; p < 2; p++) {
        if ((pp[p] != EVJ_NOPOS) != (pk[2 * e + p] == BV_PARENT_EVENT)) {
          fprintf(stderr, "ppos set for a parent that is not in the batch (or not set for one that is)\n");
          return 1;
        }
        if (pp[p] == EVJ_NOPOS) continue;
        if ((uint64_t)pp[p] + 64 > len || pp[p] < 3 || memcmp(body.get() + pp[p] - 3, "\"0X", 3) != 0) {
          fprintf(stderr, "ppos does not point at a parent's hex\n");
          return 1;
        }
        for (int i = 0; i < 64; i++)
          if (body[pp[p] + i] != '0') {
            fprintf(stderr, "ppos does not point at the 64 placeholder characters\n");
            return 1;
          }
      }
      n_bodies++;
    }

    // one field malformed at a time (copies of f; the arrays stay exact)
    auto with = [&](auto &&patch) {
      bv_event_fields_batch g = f;
      patch(g);
      return g;
    };
    const uint64_t one = 1;
    const uint8_t byte = 0;
    refuse(with([&](auto &g) { g.ev.events.bsig_off = &one; }),
           "events.bsig_off / bsig_json must be NULL (the block signatures come from fields)");
    refuse(with([&](auto &g) { g.ev.events.bsig_json = &byte; }),
           "events.bsig_off / bsig_json must be NULL (the block signatures come from fields)");
    refuse(with([&](auto &g) { g.bsig_start = nullptr; }), "null bsig_start");
    {
      std::vector<uint64_t> v = bs;
      v[0] = 1;
      auto p = exact(v);
      refuse(with([&](auto &g) { g.bsig_start = p.get(); }), "bsig_start[0] != 0");
      v = bs;
      v[1] = v[n] + 1 + below(5);  // above every later entry (n >= 2), entry 0 still 0
      {
        auto q = exact(v);
        refuse(with([&](auto &g) { g.bsig_start = q.get(); }), "bsig_start not monotone");
      }
      v = bs;
      v[n] = (1ull << 32) + 1;
      auto q = exact(v);
      refuse(with([&](auto &g) { g.bsig_start = q.get(); }), "more than 2^32 block signatures");
    }
    {  // (nb >= 2 and bso[nb] >= 1: event 0's signatures)
      refuse(with([&](auto &g) { g.bsig_index = nullptr; }), "null bsig_index");
      refuse(with([&](auto &g) { g.bsig_sig_off = nullptr; }), "null bsig_sig_off");
      std::vector<uint64_t> v = bso;
      v[0] = 1;
      auto p = exact(v);
      refuse(with([&](auto &g) { g.bsig_sig_off = p.get(); }), "bsig_sig_off[0] != 0");
      v = bso;
      v[1] = v[nb] + 1;  // above every later entry (nb >= 2), entry 0 still 0
      {
        auto q = exact(v);
        refuse(with([&](auto &g) { g.bsig_sig_off = q.get(); }), "bsig_sig_off not monotone");
      }
      refuse(with([&](auto &g) { g.bsig_sig = nullptr; }), "null bsig_sig");
      std::vector<uint8_t> kk = bk;
      kk[below(nb)] = (uint8_t)(3 + below(253));
      auto pkk = exact(kk);
      refuse(with([&](auto &g) { g.bsig_val_kind = pkk.get(); }), "bad bsig_val_kind");
      // a Validator as bytes: the offsets are read, and must be there and monotone
      kk = bk;
      kk[below(nb)] = BV_BSIG_VAL_BYTES;
      auto pk1 = exact(kk);
      refuse(with([&](auto &g) { g.bsig_val_kind = pk1.get(), g.bsig_val_off = nullptr; }), "null bsig_val_off");
      v = bvo;
      v[1] = v[nb] + 1;
      {
        auto q = exact(v);
        refuse(with([&](auto &g) { g.bsig_val_kind = pk1.get(), g.bsig_val_off = q.get(); }),
               "bsig_val_off not monotone");
      }
      v = bvo;
      v[nb] += 1;
      auto q = exact(v);
      refuse(with([&](auto &g) { g.bsig_val_kind = pk1.get(), g.bsig_val_off = q.get(), g.bsig_val_bytes = nullptr; }),
             "null bsig_val_bytes");
    }
    refuse(with([&](auto &g) { g.ev.events.n_events = (1ull << 32) + 1; }), "more than 2^32 events");
  }
  printf("ok %llu %llu %zu\n", (unsigned long long)n_bodies, (unsigned long long)n_bytes, g_refused.size());
  return 0;
}
