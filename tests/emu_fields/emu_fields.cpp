// Host build of the device's streaming whole-event path
// (babble_amd/csrc/bsigjson.h): the evj_emit variant of bv_event_fields_batch
// into the EvjSha sink over a 25-word row, what k_ev_body_hash_fields runs per
// lane, and the length functions beside the bytes actually emitted.
// Test infrastructure only (tests/test_event_fields.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/bsigjson.h"

namespace {
struct Count {
  uint64_t n = 0;
  void put(uint8_t) { n++; }
};
}  // namespace

extern "C" {

// Digests of the bodies of events [e0, e1) (in-batch parents as 64 '0')
void emuf_ev_body_hash(const bv_event_fields_batch *f, uint64_t e0, uint64_t e1, uint8_t *digests) {
  for (uint64_t e = e0; e < e1; e++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    evj_emit(*f, e, o);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (e - e0), be, 32);
  }
}

// kind 0: one list element per block signature (`owner[j]` its event), 1: the
// event body per event.  lens[k] = the *_len function, emitted[k] = the bytes
// the emit function puts.
void emuf_lens(const bv_event_fields_batch *f, int kind, uint64_t k0, uint64_t k1, const uint64_t *owner,
               uint64_t *lens, uint64_t *emitted) {
  for (uint64_t k = k0; k < k1; k++) {
    Count c;
    uint32_t pp[2];
    if (kind == 0) {
      lens[k - k0] = bsig_elem_len(*f, owner[k], k);
      bsig_elem_emit(*f, owner[k], k, c);
    } else {
      lens[k - k0] = evj_len(*f, k, pp);
      evj_emit(*f, k, c);
    }
    emitted[k - k0] = c.n;
  }
}

void emuf_ppos(const bv_event_fields_batch *f, uint64_t e, uint32_t pp[2]) { evj_len(*f, e, pp); }
}
