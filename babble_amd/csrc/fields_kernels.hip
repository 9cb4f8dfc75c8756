// fields_kernels.hip — the gfx950 kernel of bv_verify_events_fields
// (bv_event_itx.cpp drives it): EventBody JSON with every member
// built from fields, the BlockSignatures list included (bsigjson.h), hashed as
// it is built.  A translation unit of its own, so that the code objects of
// kernels.hip and itx_kernels.hip are the same with and without this entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsigjson.h"
#include "bv_internal.h"

// k_ev_body_hash_itx (itx_kernels.hip) over the evj_emit variant that builds
// the BlockSignatures member from fields too: the same LDS row sink (the
// chaining value and the current block in a 25-word row per lane, odd stride)
// and the same launch shape, one lane per event of a batch without in-batch
// parents; no body, length or offset array in HBM.
#define EVF_NT 256
#define EVF_ROW 25
__global__ void __launch_bounds__(EVF_NT) k_ev_body_hash_fields(bv_event_fields_batch f, uint64_t e0, uint64_t e1,
                                                                uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[EVF_NT * EVF_ROW];
  const uint64_t e = e0 + (uint64_t)blockIdx.x * EVF_NT + threadIdx.x;
  if (e >= e1) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * EVF_ROW);
  evj_emit(f, e, o);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * e);
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// The same over a shard's slices (bv_group_verify_events_fields; evjson.h
// EvjBases, itxjson.h ItxBases, bsigjson.h BsigBases): the arrays of `f` start
// at the shard's first event / transaction / ITX / block signature / byte and
// the values in them are the whole batch's.  [e0, e1) are the whole batch's
// event indices and dig is the shard's (event e is row e - bs.ev).
__global__ void __launch_bounds__(EVF_NT) k_ev_body_hash_fields_rb(bv_event_fields_batch f, uint64_t e0, uint64_t e1,
                                                                   EvjBases bs, ItxBases ib, BsigBases sb,
                                                                   uint32_t *__restrict__ dig) {
  __shared__ uint32_t rows[EVF_NT * EVF_ROW];
  const uint64_t e = e0 + (uint64_t)blockIdx.x * EVF_NT + threadIdx.x;
  if (e >= e1) return;  // no barriers below
  EvjSha o = evj_sha_begin(rows + threadIdx.x * EVF_ROW);
  evj_emit(f, e, o, bs, ib, sb);
  uint32_t be[8];
  evj_sha_finish(o, be);
  uint4 *dst = (uint4 *)(dig + 8 * (e - bs.ev));
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

namespace bvk {
hipError_t ev_body_hash_fields(hipStream_t st, const bv_event_fields_batch &f, uint64_t e0, uint64_t e1,
                               uint32_t *dig) {
  if (e1 <= e0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_body_hash_fields, dim3((uint32_t)((e1 - e0 + EVF_NT - 1) / EVF_NT)), dim3(EVF_NT), 0, st, f,
                     e0, e1, dig);
  return hipGetLastError();
}

hipError_t ev_body_hash_fields_rb(hipStream_t st, const bv_event_fields_batch &f, uint64_t e0, uint64_t e1,
                                  const EvjBases &bs, const ItxBases &ib, const BsigBases &sb, uint32_t *dig) {
  if (e1 <= e0) return hipSuccess;
  hipLaunchKernelGGL(k_ev_body_hash_fields_rb, dim3((uint32_t)((e1 - e0 + EVF_NT - 1) / EVF_NT)), dim3(EVF_NT), 0, st,
                     f, e0, e1, bs, ib, sb, dig);
  return hipGetLastError();
}
}  // namespace bvk
