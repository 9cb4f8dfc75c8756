// fieldcheck.hip — TEST INFRASTRUCTURE: runs the device field / scalar
// primitives of babble_amd/csrc/field.h (the generated gfx950 inline asm of
// field_asm.h on the device) over operand arrays supplied by the test, so
// tests/test_gpu_field.py can compare every result with Python integers
// (mod p and Montgomery mod N).  This checks the real ISA semantics of the
// hand-scheduled programs (carry-outs, hazards, rare blocks), which the
// generator's own interpreter (tests/test_field_asm.py) cannot.  Further
// down: the zipped programs in point.h's calling patterns (k_zip) and every
// point operation of point.h, one lane per case (k_point) — the device-only
// bodies that the host builds (tests/emu and its kin) never compile.  Last:
// item_scalars (k_scalars), the digest and r of an item to u1 and the GLV
// halves of u2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../babble_amd/csrc/field.h"
#include "../../babble_amd/csrc/point.h"
#include "../../babble_amd/csrc/verify_core.h"
#include "../../babble_amd/csrc/coop.h"

// OP_ZSSM + k: component k of the zipped (x^2, y^2, x y) program;
// OP_ZSSS + k: component k of the zipped (x^2, y^2, (x ^ y)^2) program
// (field_asm.h gen_zip, used by the key-table doubling chain).
// OP_CNEG: fe_cneg_canon(x, y.v[0] & 1) (branch-free conditional negate of
// a canonical element, the verify kernels' signed-digit lookup).
enum { OP_MUL = 0, OP_SQR = 1, OP_ADD = 2, OP_SUB = 3, OP_MONT = 4, OP_INV = 5, OP_ZSSM = 6, OP_ZSSS = 9,
       OP_CNEG = 12, OP_LAST = 12 };

__global__ void __launch_bounds__(256) k_field(int op, uint32_t n, const uint32_t *__restrict__ a,
                                               const uint32_t *__restrict__ b, uint32_t *__restrict__ r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe x, y, z;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    x.v[k] = a[8 * (uint64_t)i + k];
    y.v[k] = b[8 * (uint64_t)i + k];
  }
  switch (op) {
    case OP_MUL: fe_mul(z, x, y); break;
    case OP_SQR: fe_sqr(z, x); break;
    case OP_ADD: fe_add(z, x, y); break;
    case OP_SUB: fe_sub(z, x, y); break;
    case OP_MONT: {
      sc p, q, s;
#pragma unroll
      for (int k = 0; k < 8; k++) { p.v[k] = x.v[k]; q.v[k] = y.v[k]; }
      sc_mont(s, p, q);
#pragma unroll
      for (int k = 0; k < 8; k++) z.v[k] = s.v[k];
      break;
    }
    case OP_INV: fe_inv_var(z, x); break;
    case OP_CNEG: z = x; fe_cneg_canon(z, (y.v[0] & 1u) != 0); break;
    default: {
      fe w, o[3];
#pragma unroll
      for (int k = 0; k < 8; k++) w.v[k] = x.v[k] ^ y.v[k];
#if defined(__HIP_DEVICE_COMPILE__)
      if (op < OP_ZSSS) fe_sqr_sqr_mul_zip_asm(o[0], x, o[1], y, o[2], x, y);
      else fe_sqr_sqr_sqr_zip_asm(o[0], x, o[1], y, o[2], w);
#endif
      z = o[(op - OP_ZSSM) % 3];
      break;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) r[8 * (uint64_t)i + k] = z.v[k];
}

// Host entry: n operand pairs (8 little-endian u32 limbs each).  Returns 0,
// or a negative HIP error code.  Synchronous.
extern "C" int fc_run(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *r) {
  if (op < OP_MUL || op > OP_LAST) return -1000;
  uint32_t *da = nullptr, *db = nullptr, *dr = nullptr;
  const size_t bytes = (size_t)n * 32;
  hipError_t e = hipMalloc(&da, bytes ? bytes : 32);
  if (e == hipSuccess) e = hipMalloc(&db, bytes ? bytes : 32);
  if (e == hipSuccess) e = hipMalloc(&dr, bytes ? bytes : 32);
  if (e == hipSuccess && n) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_field, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, da, db, dr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(r, dr, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// XYZZ mixed additions of the verify kernels (point.h gexz_add_ge and the
// zipped gexz_add_ge_lat), exceptional cases included: acc = 33 words per
// lane (X, Y, ZZ, ZZZ, inf flag), pts = 16 words (affine x2, y2); out = the
// accumulator after acc += pt (P == Q doubles, P == -Q gives the
// identity, the identity takes the point).
__global__ void __launch_bounds__(256) k_xyzz(int lat, uint32_t n, const uint32_t *__restrict__ acc,
                                              const uint32_t *__restrict__ pts, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  gexz R;
  fe x, y;
  const uint32_t *a = acc + 33 * (uint64_t)i, *q = pts + 16 * (uint64_t)i;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    R.X.v[k] = a[k], R.Y.v[k] = a[8 + k], R.ZZ.v[k] = a[16 + k], R.ZZZ.v[k] = a[24 + k];
    x.v[k] = q[k], y.v[k] = q[8 + k];
  }
  bool inf = a[32] != 0;
  if (lat) gexz_add_ge_lat(R, inf, x, y);
  else gexz_add_ge(R, inf, x, y);
  uint32_t *o = out + 33 * (uint64_t)i;
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = R.X.v[k], o[8 + k] = R.Y.v[k], o[16 + k] = R.ZZ.v[k], o[24 + k] = R.ZZZ.v[k];
  o[32] = inf ? 1u : 0u;
}

extern "C" int fc_xyzz(int lat, uint32_t n, const uint32_t *acc, const uint32_t *pts, uint32_t *out) {
  uint32_t *da = nullptr, *dp = nullptr, *dr = nullptr;
  const size_t ab = (size_t)(n ? n : 1) * 33 * 4, pb = (size_t)(n ? n : 1) * 16 * 4;
  hipError_t e = hipMalloc(&da, ab);
  if (e == hipSuccess) e = hipMalloc(&dp, pb);
  if (e == hipSuccess) e = hipMalloc(&dr, ab);
  if (e == hipSuccess && n) e = hipMemcpy(da, acc, ab, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(dp, pts, pb, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_xyzz, dim3((n + 255) / 256), dim3(256), 0, 0, lat, n, da, dp, dr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dr, ab, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(dp);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// The wave-cooperative XYZZ point ops of k_small's cold path (coop.h), one
// wave per case: out[74 i ..] = acc + pt (33 words: X, Y, ZZ, ZZZ, identity
// flag; add_xyzz), 2 pt (33 words; dbl_xyzz) and the doubling's beta X (8
// words).  acc and pt are XYZZ (33 words each), pt finite.
__global__ void __launch_bounds__(64) k_coop_xyzz(uint32_t n, const uint32_t *acc, const uint32_t *pts, uint32_t *out) {
  const uint32_t b = blockIdx.x;
  if (b >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t c = coop::pos(), lane = __lane_id();
  const uint32_t *a = acc + 33 * (uint64_t)b, *q = pts + 33 * (uint64_t)b;
  const auto ld = [&](const uint32_t *p, int o) { return c < 8 ? p[o + c] : 0u; };
  uint32_t X1 = ld(a, 0), Y1 = ld(a, 8), ZZ1 = ld(a, 16), ZZZ1 = ld(a, 24);
  bool inf = a[32] != 0;
  const uint32_t X2 = ld(q, 0), Y2 = ld(q, 8), ZZ2 = ld(q, 16), ZZZ2 = ld(q, 24);
  coop::add_xyzz(X1, Y1, ZZ1, ZZZ1, inf, X2, Y2, ZZ2, ZZZ2);
  uint32_t DX = X2, DY = Y2, DZZ = ZZ2, DZZZ = ZZZ2, BX;
  coop::dbl_xyzz(DX, DY, DZZ, DZZZ, BX);
  uint32_t *o = out + 74 * (uint64_t)b;
  if (lane < 8) {
    o[lane] = X1, o[8 + lane] = Y1, o[16 + lane] = ZZ1, o[24 + lane] = ZZZ1;
    o[33 + lane] = DX, o[41 + lane] = DY, o[49 + lane] = DZZ, o[57 + lane] = DZZZ;
    o[66 + lane] = BX;
  }
  if (lane == 0) o[32] = inf ? 1u : 0u, o[65] = 0u;
#endif
}

extern "C" int fc_coop_xyzz(uint32_t n, const uint32_t *acc, const uint32_t *pts, uint32_t *out) {
  uint32_t *da = nullptr, *dp = nullptr, *dr = nullptr;
  const size_t ab = (size_t)(n ? n : 1) * 33 * 4, ob = (size_t)(n ? n : 1) * 74 * 4;
  hipError_t e = hipMalloc(&da, ab);
  if (e == hipSuccess) e = hipMalloc(&dp, ab);
  if (e == hipSuccess) e = hipMalloc(&dr, ob);
  if (e == hipSuccess && n) e = hipMemcpy(da, acc, ab, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(dp, pts, ab, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_coop_xyzz, dim3(n), dim3(64), 0, 0, n, da, dp, dr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dr, ob, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(dp);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// coop.h's products and reductions on hardware, four cases a wave (one a
// DPP row): op 0 mul(a, b), 1 norm(a + (M4 - b)), 2 norm(a + 8 (M4 - b)),
// 3 norm(3 a); a, b: n x 8 words, out: n x 8 words (NORMAL, < 2^256).
__global__ void __launch_bounds__(64) k_coop_ops(int op, uint32_t n, const uint32_t *a, const uint32_t *b,
                                                 uint32_t *out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t c = coop::pos(), i = 4 * blockIdx.x + coop::row();
  const bool live = i < n;  // (every lane runs the row code: the DPP reads and ballots are wave-wide)
  const uint32_t x = live && c < 8 ? a[8 * (uint64_t)i + c] : 0u, y = live && c < 8 ? b[8 * (uint64_t)i + c] : 0u;
  uint32_t r;
  if (op == 0) r = coop::mul(x, y);
  else if (op == 1) r = coop::norm((uint64_t)x + coop::negw(y));
  else if (op == 2) r = coop::norm((uint64_t)x + 8ull * coop::negw(y));
  else r = coop::norm(3ull * x);
  if (live && c < 8) out[8 * (uint64_t)i + c] = r;
#endif
}

extern "C" int fc_coop_ops(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  uint32_t *da = nullptr, *db = nullptr, *dr = nullptr;
  const size_t bytes = (size_t)(n ? n : 1) * 32;
  hipError_t e = hipMalloc(&da, bytes);
  if (e == hipSuccess) e = hipMalloc(&db, bytes);
  if (e == hipSuccess) e = hipMalloc(&dr, bytes);
  if (e == hipSuccess && n) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_coop_ops, dim3((n + 3) / 4), dim3(64), 0, 0, op, n, da, db, dr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dr, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// Key-table base chains B_j = 2^(w j) Q (j < nwin) of n affine points
// (16 words each: x, y limbs), per lane (verify_core.h table_bases_one, the
// zipped doubling) or wave-cooperative (coop.h: one wave per point, the
// doubling's products spread over the DPP rows); out: n x nwin x 24 words
// (X, Y, Z).  Both must agree mod p (same formulas).
__global__ void __launch_bounds__(64) k_bases_lane(uint32_t n, const uint32_t *xy, uint32_t *out, int w, int nwin) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n) table_bases_one<true>(b, xy, out, w, nwin);
}
__global__ void __launch_bounds__(64) k_bases_coop(uint32_t n, const uint32_t *xy, uint32_t *out, int w, int nwin) {
  const uint32_t b = blockIdx.x;
  if (b >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
  coop_bases_one(b, xy, out, w, nwin);
#endif
}

extern "C" int fc_bases(int coop, uint32_t n, const uint32_t *xy, uint32_t *out, int w, int nwin, float *ms) {
  uint32_t *dxy = nullptr, *dout = nullptr;
  const size_t ob = (size_t)n * nwin * 24 * 4;
  hipError_t e = hipMalloc(&dxy, (size_t)n * 64 + 64);
  if (e == hipSuccess) e = hipMalloc(&dout, ob + 64);
  if (e == hipSuccess) e = hipMemcpy(dxy, xy, (size_t)n * 64, hipMemcpyHostToDevice);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  for (int rep = 0; rep < 2 && e == hipSuccess; rep++) {  // the second run is timed
    (void)hipEventRecord(e0, 0);
    if (coop)
      hipLaunchKernelGGL(k_bases_coop, dim3(n), dim3(64), 0, 0, n, dxy, dout, w, nwin);
    else
      hipLaunchKernelGGL(k_bases_lane, dim3((n + 63) / 64), dim3(64), 0, 0, n, dxy, dout, w, nwin);
    e = hipGetLastError();
    (void)hipEventRecord(e1, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess && ms) e = hipEventElapsedTime(ms, e0, e1);
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(dxy);
  (void)hipFree(dout);
  return e == hipSuccess ? 0 : -(int)e;
}

// The zipped multi-product programs of the latency point operations
// (field_asm.h gen_zip) beyond the two of the doubling chain: ops = n x 8
// operands (8 limbs each), out = n x 4 results.  `pat` 0 calls the program
// with distinct registers everywhere; the others repeat, one by one, the
// shared-input and output-on-input patterns of point.h's call sites (listed
// in tests/test_gpu_field.py::test_zipped_point_programs_match_python_ints,
// which computes the same products from the same operand indices).
enum { ZP_MM = 0, ZP_MS = 1, ZP_SS = 2, ZP_MMM = 3, ZP_MMMS = 4, ZP_SSM = 5, ZP_SSS = 6, ZP_LAST = 6 };

template <int PROG>
__global__ void __launch_bounds__(256) k_zip(int pat, uint32_t n, const uint32_t *__restrict__ ops,
                                             uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe o[8], r[4];
#pragma unroll
  for (int j = 0; j < 8; j++)
#pragma unroll
    for (int k = 0; k < 8; k++) o[j].v[k] = ops[64 * (uint64_t)i + 8 * j + k];
#pragma unroll
  for (int j = 0; j < 4; j++) fe_set(r[j], 0);
#if defined(__HIP_DEVICE_COMPILE__)
  if (PROG == ZP_MM) {
    if (pat == 0) fe_mul_mul_zip_asm(r[0], o[0], o[1], r[1], o[2], o[3]);
    else if (pat == 1) fe_mul_mul_zip_asm(r[0], o[0], o[1], r[1], o[2], o[1]);  // b0 == b1
    else if (pat == 2) {  // r0 on b0
      r[0] = o[1];
      fe_mul_mul_zip_asm(r[0], o[0], r[0], r[1], o[2], o[3]);
    } else {  // r0 on b0, r1 on b1
      r[0] = o[1], r[1] = o[3];
      fe_mul_mul_zip_asm(r[0], o[0], r[0], r[1], o[2], r[1]);
    }
  } else if (PROG == ZP_MS) {
    fe_mul_sqr_zip_asm(r[0], o[0], o[1], r[1], o[2]);
  } else if (PROG == ZP_SS) {
    fe_sqr_sqr_zip_asm(r[0], o[0], r[1], o[1]);
  } else if (PROG == ZP_MMM) {
    if (pat == 0) fe_mul_mul_mul_zip_asm(r[0], o[0], o[1], r[1], o[2], o[3], r[2], o[4], o[5]);
    else if (pat == 1) fe_mul_mul_mul_zip_asm(r[0], o[0], o[1], r[1], o[2], o[1], r[2], o[4], o[1]);  // one b
    else if (pat == 2) {  // r0 on b0, b1 == b2
      r[0] = o[1];
      fe_mul_mul_mul_zip_asm(r[0], o[0], r[0], r[1], o[2], o[3], r[2], o[4], o[3]);
    } else {  // b0 == a2
      fe_mul_mul_mul_zip_asm(r[0], o[0], o[1], r[1], o[2], o[3], r[2], o[1], o[5]);
    }
  } else if (PROG == ZP_MMMS) {
    if (pat == 0) fe_mul_mul_mul_sqr_zip_asm(r[0], o[0], o[1], r[1], o[2], o[3], r[2], o[4], o[5], r[3], o[6]);
    else fe_mul_mul_mul_sqr_zip_asm(r[0], o[0], o[1], r[1], o[2], o[1], r[2], o[4], o[0], r[3], o[6]);  // b0 == b1, a0 == b2
  } else if (PROG == ZP_SSM) {
    fe_sqr_sqr_mul_zip_asm(r[0], o[0], r[1], o[1], r[2], o[1], o[2]);  // a1 == a2 (gej_double_lat)
  } else {
    r[1] = o[1];
    fe_sqr_sqr_sqr_zip_asm(r[0], o[0], r[1], r[1], r[2], o[2]);  // r1 on a1 (gej_double_lat)
  }
#endif
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 8; k++) out[32 * (uint64_t)i + 8 * j + k] = r[j].v[k];
}

extern "C" int fc_zip(int prog, int pat, uint32_t n, const uint32_t *ops, uint32_t *out) {
  static const int npat[ZP_LAST + 1] = {4, 1, 1, 4, 2, 1, 1};
  if (prog < 0 || prog > ZP_LAST || pat < 0 || pat >= npat[prog]) return -1000;
  uint32_t *dop = nullptr, *dr = nullptr;
  const size_t ib = (size_t)(n ? n : 1) * 256, ob = (size_t)(n ? n : 1) * 128;
  hipError_t e = hipMalloc(&dop, ib);
  if (e == hipSuccess) e = hipMalloc(&dr, ob);
  if (e == hipSuccess && n) e = hipMemcpy(dop, ops, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    const dim3 g((n + 255) / 256), b(256);
    switch (prog) {
      case ZP_MM: hipLaunchKernelGGL(k_zip<ZP_MM>, g, b, 0, 0, pat, n, dop, dr); break;
      case ZP_MS: hipLaunchKernelGGL(k_zip<ZP_MS>, g, b, 0, 0, pat, n, dop, dr); break;
      case ZP_SS: hipLaunchKernelGGL(k_zip<ZP_SS>, g, b, 0, 0, pat, n, dop, dr); break;
      case ZP_MMM: hipLaunchKernelGGL(k_zip<ZP_MMM>, g, b, 0, 0, pat, n, dop, dr); break;
      case ZP_MMMS: hipLaunchKernelGGL(k_zip<ZP_MMMS>, g, b, 0, 0, pat, n, dop, dr); break;
      case ZP_SSM: hipLaunchKernelGGL(k_zip<ZP_SSM>, g, b, 0, 0, pat, n, dop, dr); break;
      default: hipLaunchKernelGGL(k_zip<ZP_SSS>, g, b, 0, 0, pat, n, dop, dr); break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dr, ob, hipMemcpyDeviceToHost);
  (void)hipFree(dop);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// Every point operation of point.h as a unit, one lane per case: a, b and out
// are 33 words each (four field elements and the identity flag).  XYZZ
// operands are (X, Y, ZZ, ZZZ), Jacobian ones (X, Y, Z, -), affine ones
// (x, y, -, -).  b's flag is the second operand's identity flag where the
// operation takes one, and "this lane adds nothing" (take == false) for the
// alternating-Y forms of gexz_add_ge.
enum {
  PO_XZ_ADD = 0, PO_XZ_ADD_LAT = 1, PO_XZ_SUM_GE_LAT = 2, PO_XZ_DOUBLE = 3,
  PO_XZ_AFF_YALT = 4,  // gexz_add_ge_aff<false, true, true>: the throughput loops' second window
  PO_XZ_AFF_LAT = 5,   // gexz_add_ge_aff<true>: the latency loops' second window
  PO_XZ_AFF = 6,       // gexz_add_ge_aff<false>
  PO_XZ_GE_XZONLY = 7, PO_XZ_GE_YALT = 8, PO_XZ_GE_YALT_XZONLY = 9,
  PO_J_DOUBLE = 10, PO_J_DOUBLE_LAT = 11, PO_J_DOUBLE_LAT_INPLACE = 12, PO_J_ADD_GE = 13, PO_J_ADD_GE_LAT = 14,
  PO_J_ADD = 15, PO_LAST = 15
};

template <int OP>
__global__ void __launch_bounds__(256) k_point(uint32_t n, const uint32_t *__restrict__ a,
                                               const uint32_t *__restrict__ b, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe A[4], B[4];
  const uint32_t *pa = a + 33 * (uint64_t)i, *pb = b + 33 * (uint64_t)i;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 8; k++) A[j].v[k] = pa[8 * j + k], B[j].v[k] = pb[8 * j + k];
  bool ainf = pa[32] != 0;
  const bool bflag = pb[32] != 0;
  if (OP >= PO_J_DOUBLE) {
    gej R = {A[0], A[1], A[2]};
    const gej S = {B[0], B[1], B[2]};
    if (OP == PO_J_DOUBLE) {
      gej D;
      gej_double(D, R);
      R = D;
    } else if (OP == PO_J_DOUBLE_LAT) {
      gej D;
      gej_double_lat(D, R);
      R = D;
    } else if (OP == PO_J_DOUBLE_LAT_INPLACE) gej_double_lat(R, R);
    else if (OP == PO_J_ADD_GE) gej_add_ge(R, ainf, B[0], B[1]);
    else if (OP == PO_J_ADD_GE_LAT) gej_add_ge_lat(R, ainf, B[0], B[1]);
    else gej_add(R, ainf, S, bflag);
    A[0] = R.X, A[1] = R.Y, A[2] = R.Z;
    fe_set(A[3], 0);
  } else {
    gexz R = {A[0], A[1], A[2], A[3]};
    const gexz S = {B[0], B[1], B[2], B[3]};
    if (OP == PO_XZ_ADD) gexz_add(R, ainf, S, bflag);
    else if (OP == PO_XZ_ADD_LAT) gexz_add_lat(R, ainf, S, bflag);
    else if (OP == PO_XZ_SUM_GE_LAT) {
      gexz D = {A[0], A[1], A[2], A[3]};  // (stale where the result is the identity)
      bool dinf;
      gexz_sum_ge_lat(D, dinf, A[0], A[1], ainf, B[0], B[1], bflag);
      R = D, ainf = dinf;
    } else if (OP == PO_XZ_DOUBLE) {
      gexz D;
      gexz_double(D, R);
      R = D;
    } else if (OP == PO_XZ_AFF_YALT) gexz_add_ge_aff<false, true, true>(R, ainf, B[0], B[1]);
    else if (OP == PO_XZ_AFF_LAT) gexz_add_ge_aff<true>(R, ainf, B[0], B[1]);
    else if (OP == PO_XZ_AFF) gexz_add_ge_aff<false>(R, ainf, B[0], B[1]);
    else if (OP == PO_XZ_GE_XZONLY) gexz_add_ge(R, ainf, B[0], B[1], true);
    else if (OP == PO_XZ_GE_YALT) gexz_add_ge<true, true>(R, ainf, B[0], B[1], false, false, !bflag);
    else gexz_add_ge<true, true>(R, ainf, B[0], B[1], true, false, !bflag);
    A[0] = R.X, A[1] = R.Y, A[2] = R.ZZ, A[3] = R.ZZZ;
  }
  uint32_t *o = out + 33 * (uint64_t)i;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 8; k++) o[8 * j + k] = A[j].v[k];
  o[32] = ainf ? 1u : 0u;
}

extern "C" int fc_point(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  if (op < 0 || op > PO_LAST) return -1000;
  uint32_t *da = nullptr, *db = nullptr, *dr = nullptr;
  const size_t bytes = (size_t)(n ? n : 1) * 33 * 4;
  hipError_t e = hipMalloc(&da, bytes);
  if (e == hipSuccess) e = hipMalloc(&db, bytes);
  if (e == hipSuccess) e = hipMalloc(&dr, bytes);
  if (e == hipSuccess && n) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    const dim3 g((n + 255) / 256), t(256);
#define FC_POINT_CASE(OP) \
  case OP: hipLaunchKernelGGL(k_point<OP>, g, t, 0, 0, n, da, db, dr); break;
    switch (op) {
      FC_POINT_CASE(0) FC_POINT_CASE(1) FC_POINT_CASE(2) FC_POINT_CASE(3) FC_POINT_CASE(4) FC_POINT_CASE(5)
      FC_POINT_CASE(6) FC_POINT_CASE(7) FC_POINT_CASE(8) FC_POINT_CASE(9) FC_POINT_CASE(10) FC_POINT_CASE(11)
      FC_POINT_CASE(12) FC_POINT_CASE(13) FC_POINT_CASE(14) FC_POINT_CASE(15)
    }
#undef FC_POINT_CASE
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dr, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dr);
  return e == hipSuccess ? 0 : -(int)e;
}

// verify_core.h's item_scalars as it stands, one item per lane: u1 = e s^-1
// mod N from the UNREDUCED 256-bit digest e, and the GLV split of
// u2 = r s^-1.  dig and r_be: 8 words per item, the 32 big-endian bytes as the
// kernels read them (sc_load_be_words); w: s^-1 2^256 mod N in 8 limbs, what
// k_sinv leaves; item i reads digest i.  out: 17 words per item, u1[8],
// k1[4], k2[4] and the sign word.
__global__ void __launch_bounds__(256) k_scalars(uint32_t n, const uint32_t *__restrict__ dig,
                                                 const uint32_t *__restrict__ r_be,
                                                 const uint32_t *__restrict__ w,
                                                 const uint32_t *__restrict__ item_msg, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t u1[8], k1[4], k2[4], signs;
  item_scalars(i, r_be, item_msg, dig, w, u1, k1, k2, signs);
  uint32_t *o = out + 17 * (uint64_t)i;
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = u1[k];
#pragma unroll
  for (int k = 0; k < 4; k++) o[8 + k] = k1[k], o[12 + k] = k2[k];
  o[16] = signs;
}

extern "C" int fc_scalars(uint32_t n, const uint32_t *dig, const uint32_t *r_be, const uint32_t *w, uint32_t *out) {
  uint32_t *dd = nullptr, *dr = nullptr, *dw = nullptr, *dm = nullptr, *dout = nullptr;
  const size_t bytes = (size_t)(n ? n : 1) * 32;
  hipError_t e = hipMalloc(&dd, bytes);  // (hipMalloc's alignment covers item_scalars' uint4 loads of w)
  if (e == hipSuccess) e = hipMalloc(&dr, bytes);
  if (e == hipSuccess) e = hipMalloc(&dw, bytes);
  if (e == hipSuccess) e = hipMalloc(&dm, (size_t)(n ? n : 1) * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)(n ? n : 1) * 17 * 4);
  if (e == hipSuccess && n) e = hipMemcpy(dd, dig, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(dr, r_be, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(dw, w, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    uint32_t *im = new uint32_t[n];
    for (uint32_t i = 0; i < n; i++) im[i] = i;
    e = hipMemcpy(dm, im, (size_t)n * 4, hipMemcpyHostToDevice);
    delete[] im;
  }
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_scalars, dim3((n + 255) / 256), dim3(256), 0, 0, n, dd, dr, dw, dm, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && n) e = hipMemcpy(out, dout, (size_t)n * 17 * 4, hipMemcpyDeviceToHost);
  (void)hipFree(dd);
  (void)hipFree(dr);
  (void)hipFree(dw);
  (void)hipFree(dm);
  (void)hipFree(dout);
  return e == hipSuccess ? 0 : -(int)e;
}
