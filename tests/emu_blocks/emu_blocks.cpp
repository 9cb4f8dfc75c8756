// Host build of the device's streaming BlockBody path
// (babble_amd/csrc/blkjson.h): blk_emit into the EvjSha sink over a 25-word
// row, what k_blk_body_hash runs per lane.  Test infrastructure only
// (tests/test_block_fields.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/blkjson.h"

extern "C" {

// Digests of blocks [b0, b1): digests + 32 * (b - b0).
void emub_body_hash(const bv_block_batch *k, uint64_t b0, uint64_t b1, uint8_t *digests) {
  for (uint64_t b = b0; b < b1; b++) {
    uint32_t row[25];
    EvjSha o = evj_sha_begin(row);
    blk_emit(*k, b, o);
    uint32_t be[8];
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (b - b0), be, 32);
  }
}

// blk_len of blocks [b0, b1)
void emub_body_len(const bv_block_batch *k, uint64_t b0, uint64_t b1, uint64_t *lens) {
  for (uint64_t b = b0; b < b1; b++) lens[b - b0] = blk_len(*k, b);
}

}  // extern "C"
