// itx_kernels.hip — gfx950 kernels of bv_verify_events_itx (bv_event_itx.cpp
// drives them): InternalTransactionBody JSON and EventBody JSON
// with its InternalTransactions member, both built from the ITXs' fields and
// hashed as they are built, and Event.Verify's fold over the item statuses.
// A translation unit of its own, so that the code object of kernels.hip (the
// verify kernels) is the same with and without this entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bv_internal.h"
#include "itxjson.h"

// InternalTransactionBody.Marshal() serialised straight into SHA-256, one lane
// per ITX, as k_ev_body_hash does for events: the chaining value and the
// current block in a 25-word LDS row per lane (odd stride: the 64 lanes' rows
// start in distinct banks), no body, length or offset array in HBM.  The
// digest of ITX i is message n_ev + i of the call's items.
#define ITX_NT 64
#define ITX_ROW 25
__global__ void __launch_bounds__(ITX_NT) k_itx_body_hash(bv_event_itx_batch x, uint64_t n_itx, uint64_t n_ev,
                                                          uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[ITX_NT * ITX_ROW];
  const uint64_t i = (uint64_t)blockIdx.x * ITX_NT + threadIdx.x;
  if (i >= n_itx) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * ITX_ROW);
  itx_body_emit(x, i, o);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * (n_ev + i));
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// k_ev_body_hash (kernels.hip) over the evj_emit variant that builds the
// InternalTransactions member from the fields: the same LDS row sink and the
// same launch shape, one lane per event of a batch without in-batch parents.
#define EVI_NT 256
#define EVI_ROW 25
__global__ void __launch_bounds__(EVI_NT) k_ev_body_hash_itx(bv_event_itx_batch x, uint64_t e0, uint64_t e1,
                                                             uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[EVI_NT * EVI_ROW];
  const uint64_t e = e0 + (uint64_t)blockIdx.x * EVI_NT + threadIdx.x;
  if (e >= e1) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * EVI_ROW);
  evj_emit(x, e, o);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * e);
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// The two kernels above over a shard's slices (bv_group_verify_events_itx;
// evjson.h EvjBases, itxjson.h ItxBases): the arrays of `x` start at the
// shard's first event / transaction / ITX / byte and the values in them are
// the whole batch's.  The same launch shapes and LDS row sinks.  i is the
// shard's ITX index and n_ev the shard's event count; [e0, e1) are the whole
// batch's event indices and dig is the shard's (event e is row e - bs.ev).
__global__ void __launch_bounds__(ITX_NT) k_itx_body_hash_rb(bv_event_itx_batch x, uint64_t n_itx, uint64_t n_ev,
                                                             ItxBases ib, uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[ITX_NT * ITX_ROW];
  const uint64_t i = (uint64_t)blockIdx.x * ITX_NT + threadIdx.x;
  if (i >= n_itx) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * ITX_ROW);
  itx_body_emit(x, i, o, ib);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * (n_ev + i));
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

__global__ void __launch_bounds__(EVI_NT) k_ev_body_hash_itx_rb(bv_event_itx_batch x, uint64_t e0, uint64_t e1,
                                                                EvjBases bs, ItxBases ib,
                                                                uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[EVI_NT * EVI_ROW];
  const uint64_t e = e0 + (uint64_t)blockIdx.x * EVI_NT + threadIdx.x;
  if (e >= e1) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * EVI_ROW);
  evj_emit(x, e, o, bs, ib);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * (e - bs.ev));
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// Event.Verify's fold (event.go:219-247), one lane per event: item e is the
// event signature, item n_ev + i ITX i; an ITX with force_panic set is
// BV_REF_PANIC whatever its item says (PubKeyHex shorter than 2 bytes: Go
// panics before DecodeSignature).  The first ITX of the event that is not
// ACCEPT decides it, else the event signature does.  Each wave owns the 64
// events of one word of the accept bitmask and writes it from one __ballot
// (no early return: every lane of a wave that holds an event reaches it).
__global__ void __launch_bounds__(256) k_ev_compose(uint64_t n_ev, const uint64_t *__restrict__ itx_start,
                                                    const uint8_t *__restrict__ item_status,
                                                    const uint8_t *__restrict__ force_panic,
                                                    uint8_t *__restrict__ ev_status, uint32_t *__restrict__ decided_by,
                                                    uint64_t *__restrict__ bits, uint8_t *__restrict__ itx_status) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool acc = false;
  if (e < n_ev) {
    uint8_t st = item_status[e];
    uint32_t by = BV_EV_SELF;
    const uint64_t i0 = itx_start[e], i1 = itx_start[e + 1];
    for (uint64_t i = i0; i < i1; i++) {
      const uint8_t c = force_panic[i] ? (uint8_t)BV_REF_PANIC : item_status[n_ev + i];
      itx_status[i] = c;
      if (by == BV_EV_SELF && c != BV_ACCEPT) {
        by = (uint32_t)(i - i0);
        st = c == BV_REJECT ? (uint8_t)BV_EV_ITX_INVALID : c;
      }
    }
    ev_status[e] = st;
    decided_by[e] = by;
    acc = st == BV_ACCEPT;
  }
  const uint64_t word = __ballot(acc);
  if ((threadIdx.x & 63) == 0 && e < n_ev) bits[e >> 6] = word;
}

// k_ev_compose over a shard: itx_start holds the whole batch's values from the
// shard's first event on, while item_status, force_panic, itx_status and the
// outputs are the shard's own (its first ITX is the batch's ITX itx_base).
// The fold is ev_fold (itxjson.h), which the host emulator runs too;
// k_ev_compose keeps its own copy so that its code stays what it was,
// instruction for instruction.
__global__ void __launch_bounds__(256) k_ev_compose_rb(uint64_t n_ev, const uint64_t *__restrict__ itx_start,
                                                       uint64_t itx_base, const uint8_t *__restrict__ item_status,
                                                       const uint8_t *__restrict__ force_panic,
                                                       uint8_t *__restrict__ ev_status,
                                                       uint32_t *__restrict__ decided_by, uint64_t *__restrict__ bits,
                                                       uint8_t *__restrict__ itx_status) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool acc = false;
  if (e < n_ev)
    acc = ev_fold(n_ev, e, itx_start, itx_base, item_status, force_panic, ev_status, decided_by, itx_status);
  const uint64_t word = __ballot(acc);
  if ((threadIdx.x & 63) == 0 && e < n_ev) bits[e >> 6] = word;
}

namespace bvk {
static inline dim3 grid1(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }

hipError_t itx_body_hash(hipStream_t st, const bv_event_itx_batch &x, uint64_t n_itx, uint64_t n_ev, uint32_t *dig) {
  if (n_itx == 0) return hipSuccess;
  hipLaunchKernelGGL(k_itx_body_hash, grid1(n_itx, ITX_NT), dim3(ITX_NT), 0, st, x, n_itx, n_ev, dig);
  return hipGetLastError();
}

hipError_t ev_body_hash_itx(hipStream_t st, const bv_event_itx_batch &x, uint64_t e0, uint64_t e1, uint32_t *dig) {
  if (e1 <= e0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_body_hash_itx, grid1(e1 - e0, EVI_NT), dim3(EVI_NT), 0, st, x, e0, e1, dig);
  return hipGetLastError();
}

hipError_t itx_body_hash_rb(hipStream_t st, const bv_event_itx_batch &x, uint64_t n_itx, uint64_t n_ev,
                            const ItxBases &ib, uint32_t *dig) {
  if (n_itx == 0) return hipSuccess;
  hipLaunchKernelGGL(k_itx_body_hash_rb, grid1(n_itx, ITX_NT), dim3(ITX_NT), 0, st, x, n_itx, n_ev, ib, dig);
  return hipGetLastError();
}

hipError_t ev_body_hash_itx_rb(hipStream_t st, const bv_event_itx_batch &x, uint64_t e0, uint64_t e1,
                               const EvjBases &bs, const ItxBases &ib, uint32_t *dig) {
  if (e1 <= e0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_body_hash_itx_rb, grid1(e1 - e0, EVI_NT), dim3(EVI_NT), 0, st, x, e0, e1, bs, ib, dig);
  return hipGetLastError();
}

hipError_t ev_compose_rb(hipStream_t st, uint64_t n_ev, const uint64_t *itx_start, uint64_t itx_base,
                         const uint8_t *item_status, const uint8_t *force_panic, uint8_t *ev_status,
                         uint32_t *decided_by, uint64_t *bits, uint8_t *itx_status) {
  if (n_ev == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_compose_rb, grid1(n_ev, 256), dim3(256), 0, st, n_ev, itx_start, itx_base, item_status,
                     force_panic, ev_status, decided_by, bits, itx_status);
  return hipGetLastError();
}

hipError_t ev_compose(hipStream_t st, uint64_t n_ev, const uint64_t *itx_start, const uint8_t *item_status,
                      const uint8_t *force_panic, uint8_t *ev_status, uint32_t *decided_by, uint64_t *bits,
                      uint8_t *itx_status) {
  if (n_ev == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_compose, grid1(n_ev, 256), dim3(256), 0, st, n_ev, itx_start, item_status, force_panic,
                     ev_status, decided_by, bits, itx_status);
  return hipGetLastError();
}
}  // namespace bvk
