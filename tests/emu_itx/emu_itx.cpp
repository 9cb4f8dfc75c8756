// Host build of the device's streaming InternalTransaction paths
// (babble_amd/csrc/itxjson.h): itx_body_emit and the evj_emit variant into the
// EvjSha sink over a 25-word row, what k_itx_body_hash and k_ev_body_hash_itx
// run per lane, and the length functions beside the bytes actually emitted.
// Test infrastructure only (tests/test_event_itx.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/itxjson.h"

namespace {
struct Count {
  uint64_t n = 0;
  void put(uint8_t) { n++; }
};
}  // namespace

extern "C" {

// Digests of InternalTransactionBody.Marshal() of ITXs [i0, i1)
void emui_itx_body_hash(const bv_event_itx_batch *x, uint64_t i0, uint64_t i1, uint8_t *digests) {
  for (uint64_t i = i0; i < i1; i++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    itx_body_emit(*x, i, o);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (i - i0), be, 32);
  }
}

// Digests of the bodies of events [e0, e1) (in-batch parents as 64 '0')
void emui_ev_body_hash(const bv_event_itx_batch *x, uint64_t e0, uint64_t e1, uint8_t *digests) {
  for (uint64_t e = e0; e < e1; e++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    evj_emit(*x, e, o);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (e - e0), be, 32);
  }
}

// kind 0: itx_body, 1: itx_elem (per ITX), 2: the event body (per event).
// lens[k] = the *_len function, emitted[k] = the bytes the emit function puts.
void emui_lens(const bv_event_itx_batch *x, int kind, uint64_t k0, uint64_t k1, uint64_t *lens, uint64_t *emitted) {
  for (uint64_t k = k0; k < k1; k++) {
    Count c;
    uint32_t pp[2];
    if (kind == 0) {
      lens[k - k0] = itx_body_len(*x, k);
      itx_body_emit(*x, k, c);
    } else if (kind == 1) {
      lens[k - k0] = itx_elem_len(*x, k);
      itx_elem_emit(*x, k, c);
    } else {
      lens[k - k0] = evj_len(*x, k, pp);
      evj_emit(*x, k, c);
    }
    emitted[k - k0] = c.n;
  }
}

// evj_len's parent hex positions of event e
void emui_ppos(const bv_event_itx_batch *x, uint64_t e, uint32_t *ppos) { evj_len(*x, e, ppos); }

// gojson_string of s[0..n) into out (capacity cap); returns gojson_string_len
uint64_t emui_string(const uint8_t *s, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written) {
  Count c;
  gojson_string(c, s, n);
  *written = c.n;
  if (c.n <= cap) {
    EvjMem m{out};
    gojson_string(m, s, n);
  }
  return gojson_string_len(s, n);
}

}  // extern "C"
