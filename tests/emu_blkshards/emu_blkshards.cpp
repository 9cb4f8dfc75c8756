// Host build of the rebased BlockBody serialiser (babble_amd/csrc/blkjson.h,
// blk_len / blk_emit with BlkBases): what k_blk_body_hash_rb runs per lane,
// given ONLY a shard's slices of a block batch and the shard's bases.  Test
// infrastructure only (tests/test_block_shards.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/blkjson.h"

extern "C" {

// Digests and body lengths of blocks [b0, b1) (the whole batch's indices) of
// the shard whose slices are `k` and whose bases are `bases` (blk, hash, tx,
// txb, itx, rcpt): digests + 32 * (b - blk), lens[b - blk].  The SHA sink's
// byte count must equal blk_len (returns 1 otherwise).
int emubs_body_hash(const bv_block_batch *k, uint64_t b0, uint64_t b1, const uint64_t bases[6], uint8_t *digests,
                    uint64_t *lens) {
  const BlkBases bs{bases[0], bases[1], bases[2], bases[3], bases[4], bases[5]};
  for (uint64_t b = b0; b < b1; b++) {
    uint32_t row[25];
    EvjSha o = evj_sha_begin(row);
    blk_emit(*k, b, o, bs);
    lens[b - bs.blk] = blk_len(*k, b, bs);
    if ((uint64_t)o.nblk * 64 + o.n != lens[b - bs.blk]) return 1;
    uint32_t be[8];
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (b - bs.blk), be, 32);
  }
  return 0;
}

}  // extern "C"
