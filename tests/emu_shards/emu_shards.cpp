// Host build of the rebased serialiser (babble_amd/csrc/evjson.h, evj_emit
// with EvjBases): what k_ev_body_hash_rb runs per lane, given ONLY a shard's
// slices of a wire batch and the shard's bases.  Test infrastructure only
// (tests/test_event_shards.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/evjson.h"

extern "C" {

// Digests of events [e0, e1) (the whole batch's indices) of the shard whose
// slices are `b` and whose bases are `bases` (ev, tx, txb, itx, bsig, ph):
// digests + 32 * (e - ev).
void emus_body_hash(const bv_event_batch *b, uint64_t e0, uint64_t e1, const uint64_t bases[6], uint8_t *digests) {
  const EvjBases bs{bases[0], bases[1], bases[2], bases[3], bases[4], bases[5]};
  for (uint64_t e = e0; e < e1; e++) {
    uint32_t row[25];
    EvjSha o = evj_sha_begin(row);
    evj_emit(*b, e, o, bs);
    uint32_t be[8];
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (e - bs.ev), be, 32);
  }
}

}  // extern "C"
