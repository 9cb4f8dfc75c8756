// verify_core.h — the per-unit work of every kernel, as __host__ __device__
// functions.  kernels.hip maps them onto the grid; tests/emu compiles the
// same source for the host so index logic and arithmetic are exercised on
// the CPU (with sanitizers) before a GPU run.  Nothing here is a CPU path of
// the product: libbabbleverify.so only ever runs these on gfx950.
#pragma once
#include <type_traits>
#include <stdint.h>

#include "../../include/babbleverify.h"
#include "geometry.h"
#include "coop.h"
#include "point.h"
#include "sha256.h"

// key status (k_key_decode output)
#define KS_OK 0
#define KS_EMPTY 1
#define KS_BAD 2

// p - N: r + N < p  <=>  r < p - N
static constexpr uint32_t P_MINUS_N[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u,
                                          0x00000001u, 0u, 0u, 0u};

// ---------------------------------------------------------------------------
// loads / stores
// ---------------------------------------------------------------------------
DEV void fe_load_be(fe &r, const uint8_t *b) {  // 32 big-endian bytes, any alignment
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t *q = b + 4 * (7 - i);
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}
DEV void fe_load_be_words(fe &r, const uint32_t *w) {  // 8 dwords holding 32 BE bytes
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = bswap32(w[7 - i]);
}
DEV void sc_load_be_words(sc &r, const uint32_t *w) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = bswap32(w[7 - i]);
}
DEV void fe_store(uint32_t *p, const fe &a) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
DEV void fe_load(fe &a, const uint32_t *p) {
#pragma unroll
  for (int i = 0; i < 8; i++) a.v[i] = p[i];
}
DEV void fe_load4(fe &a, const uint32_t *p) {  // 16-byte aligned: 2 x dwordx4
#if defined(__HIP_DEVICE_COMPILE__)
  // table entries live in global memory: global_load, not flat_load (a flat
  // access also counts against lgkmcnt and takes the aperture check)
  typedef const __attribute__((address_space(1))) uint4 *gptr;
  const gptr q = (gptr)p;
#else
  const uint4 *q = (const uint4 *)p;
#endif
  uint4 l = q[0], h = q[1];
  a.v[0] = l.x; a.v[1] = l.y; a.v[2] = l.z; a.v[3] = l.w;
  a.v[4] = h.x; a.v[5] = h.y; a.v[6] = h.z; a.v[7] = h.w;
}
DEV void store16(uint32_t *p, const uint32_t *v) {  // 64 bytes, 16-byte aligned
  uint4 *q = (uint4 *)p;
#pragma unroll
  for (int c = 0; c < 4; c++) q[c] = make_uint4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
}
DEV bool u256_lt(const uint32_t *a, const uint32_t *b) {
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] < b[i];
  }
  return false;
}
DEV bool u256_is_zero(const uint32_t *a) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a[i];
  return x == 0;
}

// ---------------------------------------------------------------------------
// SHA-256 of message m -> 8 dwords holding the 32 big-endian digest bytes
// (crypto.SHA256, src/crypto/hash.go:8)
// ---------------------------------------------------------------------------
DEV void sha256_one(uint64_t m, const uint8_t *bytes, const uint64_t *off, uint32_t *digest_words) {
  const uint64_t o = off[m];
  const uint64_t len = off[m + 1] - o;
  uint32_t h[8];
  sha256_msg(h, bytes, o, len);
  uint32_t be[8];
#pragma unroll
  for (int i = 0; i < 8; i++) be[i] = bswap32(h[i]);
  uint4 *dst = (uint4 *)(digest_words + 8 * m);
  dst[0] = make_uint4(be[0], be[1], be[2], be[3]);
  dst[1] = make_uint4(be[4], be[5], be[6], be[7]);
}

// ---------------------------------------------------------------------------
// elliptic.Unmarshal(btcec.S256(), b) (src/crypto/keys/public_key.go:14-20):
// len 65, prefix 0x04, x < p, y < p, y^2 == x^3 + 7.  len 0 -> ToPublicKey
// returns nil (KS_EMPTY: ecdsa.Verify panics at pub.Curve).
// ---------------------------------------------------------------------------
DEV void key_decode_point(const uint8_t *kbytes, uint64_t o, uint64_t len, uint8_t &st, fe &x, fe &y) {
  st = KS_BAD;
  fe_set(x, 0);
  fe_set(y, 0);
  if (len == 0) {
    st = KS_EMPTY;
  } else if (len == 65 && kbytes[o] == 4) {
#if defined(__HIP_DEVICE_COMPILE__)
    // 17 aligned dword loads issued together (bytewise loads of an unaligned
    // key serialise on memory latency: 80 us for one wave of 64 keys); the
    // last dword may extend <= 7 bytes past the key (key_bytes is padded)
    const uint32_t *w = (const uint32_t *)(kbytes + (o & ~(uint64_t)3));
    const uint32_t sh = (uint32_t)(o & 3);
    uint32_t d[18];
#pragma unroll
    for (int i = 0; i < 18; i++) d[i] = w[i];
#pragma unroll
    for (int i = 0; i < 8; i++) {  // big-endian bytes 1 + 4 (7 - i) .. and 33 + 4 (7 - i) ..
      const uint32_t bx = 1 + 4 * (7 - i) + sh, by = 33 + 4 * (7 - i) + sh;
      x.v[i] = bswap32(alignbyte(d[bx / 4 + 1], d[bx / 4], bx % 4));
      y.v[i] = bswap32(alignbyte(d[by / 4 + 1], d[by / 4], by % 4));
    }
#else
    fe_load_be(x, kbytes + o + 1);
    fe_load_be(y, kbytes + o + 33);
#endif
    if (!fe_ge_p(x) && !fe_ge_p(y)) {
      fe y2, x3, seven;
      fe_sqr(y2, y);
      fe_sqr(x3, x);
      fe_mul(x3, x3, x);
      fe_set(seven, 7);
      fe_add(x3, x3, seven);
      if (fe_eq(y2, x3)) st = KS_OK;
    }
  }
}

DEV void key_decode_one(uint32_t k, const uint8_t *kbytes, const uint64_t *koff, uint8_t *kstatus, uint32_t *kxy) {
  uint8_t st;
  fe x, y;
  key_decode_point(kbytes, koff[k], koff[k + 1] - koff[k], st, x, y);
  kstatus[k] = st;
  fe_store(kxy + 16 * k, x);
  fe_store(kxy + 16 * k + 8, y);
}

// ---------------------------------------------------------------------------
// Fixed-base tables
// ---------------------------------------------------------------------------
// B_j = 2^(w j) P_b (Jacobian, 24 words each), j < nwin: a serial doubling
// chain per base.
template <bool LAT = false>
DEV void table_bases_one(uint32_t b, const uint32_t *bxy, uint32_t *bases_jac, int w, int nwin) {
  gej P;
  fe_load(P.X, bxy + 16 * b);
  fe_load(P.Y, bxy + 16 * b + 8);
  fe_set(P.Z, 1);
  uint32_t *out = bases_jac + (uint64_t)b * nwin * 24;
  for (int j = 0; j < nwin; j++) {
    fe_store(out + 24 * j, P.X);
    fe_store(out + 24 * j + 8, P.Y);
    fe_store(out + 24 * j + 16, P.Z);
    if (j + 1 < nwin) {
      for (int k = 0; k < w; k++) gej_double_sel<LAT>(P, P);  // one wave per 64 keys: latency bound
    }
  }
}

#if defined(__HIPCC__)
// The same chain, wave-cooperative (coop.h): ONE wave per base, the
// doubling's three product levels spread over the wave's DPP rows; lanes
// 0..7 (row 0) store.  Same formulas, so the same Jacobian representatives
// as table_bases_one.
__device__ __forceinline__ void coop_bases_one(uint32_t b, const uint32_t *bxy, uint32_t *bases_jac, int w, int nwin) {
  const uint32_t k = coop::pos(), lane = __lane_id();
  uint32_t X = k < 8 ? bxy[16 * (uint64_t)b + k] : 0u, Y = k < 8 ? bxy[16 * (uint64_t)b + 8 + k] : 0u;
  uint32_t Z = k == 0 ? 1u : 0u;
  uint32_t *out = bases_jac + (uint64_t)b * nwin * 24;
  for (int j = 0; j < nwin; j++) {
    if (lane < 8) {
      out[24 * j + lane] = X;
      out[24 * j + 8 + lane] = Y;
      out[24 * j + 16 + lane] = Z;
    }
    if (j + 1 < nwin)
      for (int i = 0; i < w; i++) coop::dbl(X, Y, Z);
  }
}
#endif

// d * B (B affine), MSB-first double-and-add over `bits` bits of d.  The
// returned Z is 1 for d == 0 so it can join a batch inversion.
template <bool LAT = false>
DEV void table_point(gej &R, bool &inf, fe &Z, const fe &bx, const fe &by, uint32_t d, int bits) {
  pt_set_identity(R, inf);
  for (int bit = bits - 1; bit >= 0; bit--) {
    if (!inf) gej_double_sel<LAT>(R, R);
    if ((d >> bit) & 1) gej_add_ge_sel<LAT>(R, inf, bx, by);
  }
  if (inf) fe_set(Z, 1);
  else Z = R.Z;
}

// Store one entry given Z^-1 (canonical affine; d == 0 stored as zeros).
// With `phi` != null also store phi(entry) = (beta x, y) there.
DEV void table_store(uint32_t *entry, uint32_t *phi, uint32_t d, const gej &R, bool inf, const fe &zi) {
  fe zi2, zi3, x, y;
  fe_sqr(zi2, zi);
  fe_mul(zi3, zi2, zi);
  fe_mul(x, R.X, zi2);
  fe_mul(y, R.Y, zi3);
  fe_canon(x);
  fe_canon(y);
  if (d == 0 || inf) {
    fe_set(x, 0);
    fe_set(y, 0);
  }
  uint32_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = x.v[i];
    v[8 + i] = y.v[i];
  }
  store16(entry, v);
  if (phi) {
    fe beta, bx;
    fe_load(beta, FE_BETA);
    fe_mul(bx, x, beta);
    fe_canon(bx);
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = bx.v[i];
    store16(phi, v);
  }
}

// K12 entry (j, d) = S_2j[lo] + S_2j+1[hi], lo = d mod 2^L, hi = d >> L,
// with S_k[x] = x 2^(Lk) Q affine (zeros for x == 0).  The two points are
// distinct multiples lo 2^(Wj) Q and hi 2^(Wj+L) Q of Q with
// 0 < lo < 2^L <= hi 2^L and lo + hi 2^L < 2^W << N, so they are neither
// equal nor opposite and the affine chord formula applies:
//   lambda = (y2 - y1) / (x2 - x1), x3 = lambda^2 - x1 - x2,
//   y3 = lambda (x1 - x3) - y1.
// The denominators H = x2 - x1 of a block are inverted together
// (Montgomery's trick, k_table_pair).  kind: 0 zero entry, 1 copy S_lo,
// 2 copy S_hi, 3 chord sum.
DEV int pair_kind(uint32_t lo, uint32_t hi) { return (lo ? 1 : 0) | (hi ? 2 : 0); }

// K12 builder slot -> digit: slot 0 of a window block builds the window's
// top digit 2^(W-1) = ENT (stored at window j+1's unused slot 0).
DEV uint32_t k12_digit(uint32_t d, uint32_t ent) { return d ? d : ent; }

DEV void pair_load(const uint32_t *s_lo, const uint32_t *s_hi, uint32_t lo, uint32_t hi, fe &x1, fe &y1, fe &x2,
                   fe &y2) {
  fe_load(x1, s_lo + BV_ENTRY_U32 * lo);
  fe_load(y1, s_lo + BV_ENTRY_U32 * lo + 8);
  fe_load(x2, s_hi + BV_ENTRY_U32 * hi);
  fe_load(y2, s_hi + BV_ENTRY_U32 * hi + 8);
}

// the value joining the batch inversion (1 unless the entry is a sum)
DEV void pair_denominator(fe &H, int kind, const fe &x1, const fe &x2) {
  if (kind == 3) fe_sub(H, x2, x1);
  else fe_set(H, 1);
}

DEV void pair_store(uint32_t *entry, uint32_t *phi, int kind, const fe &x1, const fe &y1, const fe &x2, const fe &y2,
                    const fe &Hinv) {
  fe x, y;
  if (kind == 3) {
    fe lam, t;
    fe_sub(t, y2, y1);
    fe_mul(lam, t, Hinv);
    fe_sqr(x, lam);
    fe_sub(x, x, x1);
    fe_sub(x, x, x2);
    fe_sub(t, x1, x);
    fe_mul(y, lam, t);
    fe_sub(y, y, y1);
  } else if (kind == 1) {
    x = x1;
    y = y1;
  } else {
    x = x2;  // kind 2, or kind 0 with S_hi[0] = zeros
    y = y2;
  }
  fe_canon(x);
  fe_canon(y);
  uint32_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = x.v[i];
    v[8 + i] = y.v[i];
  }
  store16(entry, v);
  if (!phi) return;
  fe beta, bx;
  fe_load(beta, FE_BETA);
  fe_mul(bx, x, beta);
  fe_canon(bx);
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = bx.v[i];
  store16(phi, v);
}

// ---------------------------------------------------------------------------
// K12 sub-tables from shared multiples (BV_FILL_SHARED, compile-time; 0
// restores the per-entry double-and-add of k_table_fill for the throughput
// instantiation, so tools/build_variant.sh builds A/B pairs from one tree).
// k_table_fill forms every S_k[x] = x B_k, x < 2^L, by its own L-bit
// double-and-add: ~5 doublings and ~3 additions per entry, and the chord
// sums never read x > 2^(W-L-1) of the odd sub-tables (hi = d >> L of a
// signed digit d <= 2^(W-1)).  Here, for L = 6:
//   1. k_fill_multiples: per sub-table the 14 points m B_k, m = 1..7 and
//      8, 16, .., 56 (one lane each, the same double-and-add; the tasks are
//      ordered so that a wave holds multiples of one size), Jacobian on B_k's
//      isomorphic curve as in k_table_fill, kept in the prefix scratch (free
//      until k_table_pair);
//   2. k_table_fill_shared: only the live entries, packed densely (64 per
//      even sub-table, 33 per odd one), each ONE Jacobian addition
//      (x & 7) B_k + (x >> 3) 8 B_k — distinct small multiples of a point of
//      prime order, so never the doubling or the identity case — or a copy
//      where one part is zero; then the same block_inverse and table_store.
// The entries are canonical affine, so every byte k_table_pair reads is the
// byte k_table_fill wrote (tests/test_fill_shared.py).
// ---------------------------------------------------------------------------
#ifndef BV_FILL_SHARED
#define BV_FILL_SHARED 1
#endif
#define BV_FS_MULTS 14  // multiples per sub-table
#define BV_FS_ODD_LIVE(W, L) ((1u << ((W) - (L) - 1)) + 1u)  // live entries of an odd sub-table

// words of multiples scratch per key
template <int NSUB>
DEV constexpr uint64_t fs_mult_u32() { return (uint64_t)NSUB * BV_FS_MULTS * 24; }
// live entries per key: all of the even sub-tables, ODD of the odd ones
template <int L, int NSUB, uint32_t ODD>
DEV constexpr uint32_t fs_live() { return (uint32_t)((NSUB + 1) / 2) * (1u << L) + (uint32_t)(NSUB / 2) * ODD; }

// task u < 14 NSUB of key b: u < 7 NSUB the multiples 1..7, then 8..56
template <int NSUB>
DEV void fill_multiple_one(uint32_t b, uint32_t u, const uint32_t *bases_jac, uint32_t *mult) {
  const bool big = u >= 7u * NSUB;
  const uint32_t v = big ? u - 7u * NSUB : u, k = v / 7u, i = v % 7u;
  const uint32_t *bj = bases_jac + ((uint64_t)b * NSUB + k) * 24;
  fe bx, by, Z;
  fe_load(bx, bj);
  fe_load(by, bj + 8);
  gej R;
  bool inf;
  table_point<false>(R, inf, Z, bx, by, big ? 8u * (i + 1) : i + 1, 6);
  uint32_t *o = mult + (uint64_t)b * fs_mult_u32<NSUB>() + ((uint64_t)k * BV_FS_MULTS + (big ? 7u : 0u) + i) * 24;
  fe_store(o, R.X);
  fe_store(o + 8, R.Y);
  fe_store(o + 16, Z);
}

// live entry f < fs_live() of a key -> sub-table k and entry x
template <int L, int NSUB, uint32_t ODD>
DEV void fill_shared_slot(uint32_t f, uint32_t &k, uint32_t &x) {
  constexpr uint32_t EVEN = (uint32_t)((NSUB + 1) / 2) << L;
  if (f < EVEN) {
    k = 2u * (f >> L);
    x = f & ((1u << L) - 1u);
  } else {
    k = 2u * ((f - EVEN) / ODD) + 1u;
    x = (f - EVEN) % ODD;
  }
}

// x B_k (Jacobian on B_k's isomorphic curve; inf for x == 0) from the multiples
template <int NSUB>
DEV void fill_shared_point(gej &R, bool &inf, fe &Z, uint32_t b, uint32_t k, uint32_t x, const uint32_t *mult) {
  const uint32_t l = x & 7u, h = x >> 3;
  const uint32_t *mk = mult + (uint64_t)b * fs_mult_u32<NSUB>() + (uint64_t)k * BV_FS_MULTS * 24;
  inf = x == 0;
  fe_set(R.X, 0);
  fe_set(R.Y, 0);
  fe_set(R.Z, 1);
  if (l) {
    const uint32_t *p = mk + (l - 1u) * 24;
    fe_load(R.X, p);
    fe_load(R.Y, p + 8);
    fe_load(R.Z, p + 16);
  }
  if (h) {
    const uint32_t *p = mk + (7u + h - 1u) * 24;
    gej H;
    fe_load(H.X, p);
    fe_load(H.Y, p + 8);
    fe_load(H.Z, p + 16);
    if (l) {
      bool ri = false;
      gej_add(R, ri, H, false);
      inf = ri;  // (cannot happen: see above)
    } else {
      R = H;
    }
  }
  Z = R.Z;
}

// ---------------------------------------------------------------------------
// Scalars: u1 = e * s^-1, u2 = r * s^-1 (mod N)  (ecdsa.Verify steps 4-6)
// ---------------------------------------------------------------------------
DEV void sc_sqrn(sc &a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) sc_mont(a, a, a);
}

// x^(N-2) in the Montgomery domain (xR -> x^-1 R): 255 S + 45 M.
// The top 128 bits of N-2 are 2^128 - 2 (runs of ones, built from
// x^(2^k - 1)); the low 128 bits use a 4-bit sliding window (chain generated
// offline; tests/test_emu.py checks inverses against Python ints).
DEV void sc_inverse(sc &r, const sc &x) {
  sc x2, x3, x5, x7, x9, x11, x13, x15;
  sc_mont(x2, x, x);
  sc_mont(x3, x2, x);
  sc_mont(x5, x3, x2);
  sc_mont(x7, x5, x2);
  sc_mont(x9, x7, x2);
  sc_mont(x11, x9, x2);
  sc_mont(x13, x11, x2);
  sc_mont(x15, x13, x2);
  sc a2 = x3, a4, a8, a16, a32, a64, t;
  a4 = a2; sc_sqrn(a4, 2); sc_mont(a4, a4, a2);
  a8 = a4; sc_sqrn(a8, 4); sc_mont(a8, a8, a4);
  a16 = a8; sc_sqrn(a16, 8); sc_mont(a16, a16, a8);
  a32 = a16; sc_sqrn(a32, 16); sc_mont(a32, a32, a16);
  a64 = a32; sc_sqrn(a64, 32); sc_mont(a64, a64, a32);
  t = a64;
  sc_sqrn(t, 32); sc_mont(t, t, a32);
  sc_sqrn(t, 16); sc_mont(t, t, a16);
  sc_sqrn(t, 8); sc_mont(t, t, a8);
  sc_sqrn(t, 4); sc_mont(t, t, a4);
  sc_sqrn(t, 2); sc_mont(t, t, a2);
  sc_sqrn(t, 1); sc_mont(t, t, x);  // x^(2^127 - 1)
  sc_sqrn(t, 1);                    // x^(2^128 - 2)
#define SQM(n, m) sc_sqrn(t, n); sc_mont(t, t, m);
  SQM(4, x11) SQM(3, x5) SQM(4, x5) SQM(4, x7) SQM(5, x13) SQM(2, x3) SQM(5, x7) SQM(6, x13)
  SQM(5, x11) SQM(4, x13) SQM(3, x) SQM(6, x5) SQM(10, x7) SQM(4, x7) SQM(5, x15) SQM(4, x15)
  SQM(5, x9) SQM(6, x11) SQM(4, x13) SQM(5, x3) SQM(6, x13) SQM(10, x13) SQM(4, x9) SQM(9, x9)
  SQM(4, x15) SQM(1, x)
#undef SQM
  r = t;
}

DEV bool s_usable(const uint8_t *pre, uint64_t i, const sc &s) {
  return (pre == nullptr || pre[i] == 0) && !u256_is_zero(s.v) && u256_lt(s.v, SC_N);
}

// k_sinv, thread t of T: w_i = s_i^-1 R mod N (Montgomery form) for items
// t, t+T, ..., t+(M-1)T with one inversion (Montgomery's trick).
// Needs only s and pre, so it runs on its own stream concurrently with
// SHA-256 and the key tables; the digest-dependent products u1 = e w and
// u2 = r w are formed by k_verify_g (item_scalars).  Unusable items
// contribute s = 1 and get a w that is never read.
//
// The raw s_k enter the Montgomery products unconverted (no s R^2 -> s R
// step): after k items the prefix is acc_k = R^(1-k) prod_{i<=k} s_i, the
// inverse of the total (xR -> x^-1 R) is R^(1+K) / prod s, one extra
// product by 1 makes it R^K / prod s, and walking back w_k = inv acc_(k-1)
// / R = R / s_k while inv loses one s_k and one R per step.
// The two halves of a lane's walk, split so that k_sinv_block can put the
// block stage between them: the prefix products go to w_out and the lane's
// total acc_K comes back; the walk back takes inv = R / acc_K = R^K / prod s.
DEV void sinv_lane_prefix(sc &acc, uint64_t t, uint64_t T, uint64_t n_items, uint32_t M, const uint32_t *s_be,
                          const uint8_t *pre, uint32_t *w_out) {
  sc one;
#pragma unroll
  for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u;
  sc_load_const(acc, SC_R1);
  for (uint32_t m = 0; m < M; m++) {
    const uint64_t i = t + (uint64_t)m * T;
    if (i >= n_items) break;
    sc s;
    sc_load_be_words(s, s_be + 8 * i);
    if (!s_usable(pre, i, s)) s = one;
    uint4 *q = (uint4 *)(w_out + 8 * i);
    q[0] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    q[1] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
    sc_mont(acc, acc, s);
  }
}

DEV void sinv_lane_finish(sc inv, uint64_t t, uint64_t T, uint64_t n_items, uint32_t M, const uint32_t *s_be,
                          const uint8_t *pre, uint32_t *w_out) {
  sc one;
#pragma unroll
  for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u;
  for (int m = (int)M - 1; m >= 0; m--) {
    const uint64_t i = t + (uint64_t)m * T;
    if (i >= n_items) continue;
    sc s, pfx, w;
    sc_load_be_words(s, s_be + 8 * i);
    if (!s_usable(pre, i, s)) s = one;
    uint4 *q = (uint4 *)(w_out + 8 * i);
    const uint4 a = q[0], b = q[1];
    pfx.v[0] = a.x; pfx.v[1] = a.y; pfx.v[2] = a.z; pfx.v[3] = a.w;
    pfx.v[4] = b.x; pfx.v[5] = b.y; pfx.v[6] = b.z; pfx.v[7] = b.w;
    sc_mont(w, inv, pfx);  // s^-1 R
    sc_mont(inv, inv, s);
    q[0] = make_uint4(w.v[0], w.v[1], w.v[2], w.v[3]);
    q[1] = make_uint4(w.v[4], w.v[5], w.v[6], w.v[7]);
  }
}

DEV void sinv_thread(uint64_t t, uint64_t T, uint64_t n_items, uint32_t M, const uint32_t *s_be, const uint8_t *pre,
                     uint32_t *w_out) {
  sc acc, inv, one;
#pragma unroll
  for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u;
  sinv_lane_prefix(acc, t, T, n_items, M, s_be, pre, w_out);
  sc_inverse_var(inv, acc);
  sc_mont(inv, inv, one);
  sinv_lane_finish(inv, t, T, n_items, M, s_be, pre, w_out);
}

// BV_SINV_BLOCK (compile-time; 0 restores one inversion per lane): a second
// level of Montgomery's trick inside the block.  Every lane's total A_t =
// acc_K is a canonical non-zero residue (a lane with no items holds R, a
// Montgomery one), and all the lane needs back is R / A_t.  That is the
// invariant above once more with the A_t in the place of the s_k: lane j of
// the L lanes of one wave takes the totals j, j + L, ... below B, forms
// their prefix products R^(1-k) prod A, inverts once, and walks back
// out_k = R / A_k.  So a block of B lanes runs L inversion sequences on one
// wave instead of B on B / 64 waves, for 3 B / L extra products on that wave.
// `tot` and `out` hold B scalars of 8 words (LDS on the device, between two
// barriers); sc_mont results are canonical, so w is bit for bit the per-lane
// form's.
#ifndef BV_SINV_BLOCK
#define BV_SINV_BLOCK 1
#endif
#ifndef BV_SINV_THREADS  // lanes per k_sinv_block block (a multiple of 64)
#define BV_SINV_THREADS 256
#endif

DEV void sinv_block_lane(uint32_t j, uint32_t L, uint32_t B, const uint32_t *tot, uint32_t *out) {
  if (j >= B) return;
  sc acc, inv, one;
#pragma unroll
  for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u;
  sc_load_const(acc, SC_R1);
  uint32_t last = j;
  for (uint32_t k = j; k < B; k += L) {
    sc a;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      a.v[i] = tot[8 * k + i];
      out[8 * k + i] = acc.v[i];
    }
    sc_mont(acc, acc, a);
    last = k;
  }
  sc_inverse_var(inv, acc);
  sc_mont(inv, inv, one);
  for (uint32_t k = last;; k -= L) {
    sc a, pfx, w;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      a.v[i] = tot[8 * k + i];
      pfx.v[i] = out[8 * k + i];
    }
    sc_mont(w, inv, pfx);  // R / A_k
    sc_mont(inv, inv, a);
#pragma unroll
    for (int i = 0; i < 8; i++) out[8 * k + i] = w.v[i];
    if (k < L) break;
  }
}

// The scalars of an item that reaches the math (ecdsa.Verify steps 4-6).
// w = s^-1 R of item i, as k_sinv stored it
DEV void sc_load_w(sc &w, const uint32_t *w_in, uint64_t i) {
  const uint4 *q = (const uint4 *)(w_in + 8 * i);
  const uint4 x = q[0], y = q[1];
  w.v[0] = x.x; w.v[1] = x.y; w.v[2] = x.z; w.v[3] = x.w;
  w.v[4] = y.x; w.v[5] = y.y; w.v[6] = y.z; w.v[7] = y.w;
}
// u1 = e s^-1 mod N (e = the 256-bit digest, unreduced: e < 2^256 = R, w < N)
DEV void u1_from(const sc &e, const sc &w, uint32_t u[8]) {
  sc a;
  sc_mont(a, e, w);
#pragma unroll
  for (int k = 0; k < 8; k++) u[k] = a.v[k];
}
DEV void u1_of(uint64_t i, const uint32_t *item_msg, const uint32_t *digest_words, const sc &w, uint32_t u[8]) {
  sc e;
  sc_load_be_words(e, digest_words + 8 * (uint64_t)item_msg[i]);
  u1_from(e, w, u);
}
// the GLV split of u2 = r s^-1 mod N
DEV void u2_split_from(const sc &r, const sc &w, uint32_t k1[4], uint32_t k2[4], uint32_t &signs) {
  sc b;
  sc_mont(b, r, w);
  glv_split(k1, k2, signs, b);
}
DEV void u2_split_of(uint64_t i, const uint32_t *r_be, const sc &w, uint32_t k1[4], uint32_t k2[4], uint32_t &signs) {
  sc r;
  sc_load_be_words(r, r_be + 8 * i);
  u2_split_from(r, w, k1, k2, signs);
}
// both, from the batch arrays; the three loads stand in front of the two
// products (through u1_of / u2_split_of the non-split k_verify_g needs 136
// VGPRs instead of 123 and loses its fourth wave per SIMD)
DEV void item_scalars(uint64_t i, const uint32_t *r_be, const uint32_t *item_msg, const uint32_t *digest_words,
                      const uint32_t *w_in, uint32_t u1[8], uint32_t k1[4], uint32_t k2[4], uint32_t &signs) {
  sc w, e, r;
  sc_load_w(w, w_in, i);
  sc_load_be_words(e, digest_words + 8 * (uint64_t)item_msg[i]);
  sc_load_be_words(r, r_be + 8 * i);
  u1_from(e, w, u1);
  u2_split_from(r, w, k1, k2, signs);
}

// Key-cache batches with a few keys that have no table yet (bv_kc_prepare's
// partial mode): their items reach the math without a table; the
// KC kernels leave them as BV_DEFERRED (accept bit 0) and k_verify_deferred
// finishes them by the generic path.  Never returned to a caller.
#define BV_DEFERRED 0xFE

// ---------------------------------------------------------------------------
// Item decision table.  Returns 0xFF when the item must run
// the math, else its final status.  The host pre-class is re-checked against
// the r/s bytes so an inconsistent pre byte cannot skip a range check.
// ---------------------------------------------------------------------------
DEV uint8_t classify(uint8_t pre, uint8_t ks, const fe &r, const fe &s) {
  if (pre & BV_PRE_PARTS_BAD) return BV_REJECT_ERR;
  if (ks == KS_EMPTY) return BV_REF_PANIC;
  uint32_t rc = pre & 3u, scl = (pre >> 2) & 3u;
  if (rc == BV_SC_OK) rc = u256_is_zero(r.v) ? BV_SC_NONPOS : (u256_lt(r.v, SC_N) ? BV_SC_OK : BV_SC_GE_N);
  if (scl == BV_SC_OK) scl = u256_is_zero(s.v) ? BV_SC_NONPOS : (u256_lt(s.v, SC_N) ? BV_SC_OK : BV_SC_GE_N);
  if (rc == BV_SC_NIL) return BV_REF_PANIC;
  if (rc == BV_SC_NONPOS) return BV_REJECT;
  if (scl == BV_SC_NIL) return BV_REF_PANIC;
  if (scl == BV_SC_NONPOS) return BV_REJECT;
  if (rc == BV_SC_GE_N || scl == BV_SC_GE_N) return BV_REJECT;
  if (ks != KS_OK) return BV_REF_PANIC;
  return 0xFF;
}

DEV uint8_t classify_item(uint64_t i, const uint32_t *item_key, const uint32_t *r_be, const uint32_t *s_be,
                          const uint8_t *pre, const uint8_t *kstatus, fe &r) {
  fe s;
  fe_load_be_words(r, r_be + 8 * i);
  fe_load_be_words(s, s_be + 8 * i);
  return classify(pre ? pre[i] : 0, kstatus[item_key[i]], r, s);
}

// x(R) mod N == r, projectively: X == r Z^2, or (r + N < p and X == (r+N) Z^2)
DEV bool final_check(const gej &R, bool inf, const fe &r) {
  if (inf) return false;
  fe z2, t;
  fe_sqr(z2, R.Z);
  fe_mul(t, r, z2);
  if (fe_eq(t, R.X)) return true;
  if (u256_lt(r.v, P_MINUS_N)) {
    fe rn;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) rn.v[i] = addc32(r.v[i], SC_N[i], c);
    fe_mul(t, rn, z2);
    if (fe_eq(t, R.X)) return true;
  }
  return false;
}

// The same check on an XYZZ accumulator: x = X / ZZ, so X == r ZZ (or
// (r + N) ZZ): one multiply, no squaring.
DEV bool final_check(const gexz &R, bool inf, const fe &r) {
  if (inf) return false;
  fe t;
  fe_mul(t, r, R.ZZ);
  if (fe_eq(t, R.X)) return true;
  if (u256_lt(r.v, P_MINUS_N)) {
    fe rn;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) rn.v[i] = addc32(r.v[i], SC_N[i], c);
    fe_mul(t, rn, R.ZZ);
    if (fe_eq(t, R.X)) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// Table lookups one window ahead (throughput kernels).
// BV_LOOKUP_PIPE (compile-time; bit 0: generator-table lookups, bit 1:
// key-table lookups; default 3, 0 restores the load-then-add loops, so
// tools/build_variant.sh builds A/B pairs from one tree): window j+1's
// digit and entry address are formed, and its 64-byte entry requested,
// before window j's addition starts, so the gather's latency runs under
// ~1,800 VALU instructions instead of in front of them.
// The entry lands in LDS, not in registers (the kernels sit at the 128 VGPRs
// of 4 waves per SIMD): four 16-byte LDS-DMA loads per lane with a per-lane
// source address; a wave-instruction writes its 64 lanes' chunks to 1 KiB at
// a wave-uniform base, so chunk c of thread t is slot [c][t] of the block's
// 16 KiB, and every lane reads back only what its own request wrote (no
// barrier).  A lane requests only addresses its own loop will consume:
// lanes that returned before the loop are masked off and issue nothing.
// ---------------------------------------------------------------------------
#ifndef BV_LOOKUP_PIPE
#define BV_LOOKUP_PIPE 3
#endif
#define BV_STAGE_LANES 256  // threads per block of every throughput verify kernel

// ---------------------------------------------------------------------------
// One exception test per item (BV_DEFER_EXC, compile-time; 0 keeps the test
// of P in every addition).  With 1 the pipelined throughput loops below add
// with gexz_add_ge<false>: no fe_is_zero(P), no doubling or P + (-P) branch.
// Lemma: ZZ_final == 0 (mod p)  <=>  some step of the item had P == 0.
//   Every non-identity step multiplies ZZ by P^2 (ZZ3 = ZZ1 P^2, the affine
//   step: ZZ3 = P^2); F_p has no zero divisors; and every chain starts from
//   ZZ = 1 (the first entry taken by an identity accumulator) or from a
//   stored partial sum that passed this same test before it was stored.
// A step with P == 0 is exactly a doubling (R == 0 as well) or P + (-P): the
// lane's later values are finite garbage (table addresses come from the
// digits, never from the accumulator).  The one test after the item's last
// loop sends a flagged lane round again, under a wave-uniform "any lane
// flagged" branch: it reloads the item from memory and runs the same loops
// with `chk` set, which is the per-step-checked code BV_DEFER_EXC = 0 runs.
// `chk` is uniform (every lane still in the loop has it set), one SGPR.
// The `inf` flag needs no test of its own: in the unchecked chain it only
// goes from true to false (the identity taking an entry, which is exact);
// the only way a checked chain sets it mid-chain is P + (-P), a P == 0
// step, so the item is flagged and the second pass replays that step.
// ---------------------------------------------------------------------------
// Default 0: measured on MI355X the deferred form loses (DESIGN.md section 4,
// round 9: the second pass's live ranges cost the throughput kernels spills
// inside the addition loop and k_verify_g its fourth wave per SIMD); the
// knob, its tests and the A/B stay.
#ifndef BV_DEFER_EXC
#define BV_DEFER_EXC 0
#endif
// BV_Y_ALT (point.h: the additions store S and -S in turn and form no
// negation for the fused Y3) in the pipelined throughput loops.  The state —
// whether the accumulator holds the opposite of the sum — is a function of
// the step index alone: a loop entered in state y0 runs window j in state
// y0 ^ (j & 1) and leaves y0 ^ (NWIN & 1), all wave-uniform; the callers
// below carry it from loop to loop in one bool and put a true Y back
// (y_true) wherever an accumulator is stored or handed to code that does not
// alternate.  The deferred exception test (above) has no alternating form.
static_assert(!(BV_Y_ALT && BV_DEFER_EXC), "BV_Y_ALT and BV_DEFER_EXC are alternatives");
constexpr bool y_alt(bool lat, int pipe_bit) {
  return BV_Y_ALT != 0 && BV_FUSED_Y3 != 0 && (BV_LOOKUP_PIPE & pipe_bit) != 0 && !lat;
}
DEV void y_true(gexz &R, bool &yn) {
  if (yn) fe_neg(R.Y, R.Y);
  yn = false;
}
#if !defined(__HIP_DEVICE_COMPILE__)
// host builds (tests): items that took the second, checked pass
inline uint64_t &bv_defer_redo_count() {
  static uint64_t n = 0;
  return n;
}
#endif
// true for the whole wave when any of its lanes must redo its item
DEV bool defer_any_flagged(bool bad) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(bad) != 0;
#else
  if (bad) __atomic_fetch_add(&bv_defer_redo_count(), 1, __ATOMIC_RELAXED);
  return bad;
#endif
}
DEV bool defer_flagged(const gexz &R, bool inf) { return !inf && fe_is_zero(R.ZZ); }
// the pass flag as a scalar (it is uniform by construction)
DEV bool defer_uniform(bool chk) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(chk ? 1 : 0) != 0;
#else
  return chk;
#endif
}
// after an item's last loop: true for the lane that goes round again, checked
template <bool DEFER>
DEV bool defer_redo(const gexz &R, bool inf, bool chk) {
  if constexpr (DEFER) {
    if (!chk) {
      const bool bad = defer_flagged(R, inf);
      if (defer_any_flagged(bad)) return bad;
    }
  }
  return false;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint4 *entry_stage_slots() {
  __shared__ uint4 slots[4 * BV_STAGE_LANES];
  return slots;
}
#endif

struct entry_stage {
#if defined(__HIP_DEVICE_COMPILE__)
  DEV void request(const uint32_t *e) {
    typedef __attribute__((address_space(1))) uint4 *gptr;
    typedef __attribute__((address_space(3))) uint4 *lptr;
    // the slot's previous entry has left LDS (its ds_reads have returned)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const gptr g = (gptr)e;
    const lptr w = (lptr)entry_stage_slots() + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
#pragma unroll
    for (int c = 0; c < 4; c++)
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(g + c),
                                       (__attribute__((address_space(3))) void *)(w + c * BV_STAGE_LANES), 16, 0, 0);
  }
  DEV void take(fe &x, fe &y) {
    // the four loads of the one request in flight; nothing else is
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint4 *s = entry_stage_slots() + threadIdx.x;
    const uint4 a = s[0], b = s[BV_STAGE_LANES], c = s[2 * BV_STAGE_LANES], d = s[3 * BV_STAGE_LANES];
    x.v[0] = a.x; x.v[1] = a.y; x.v[2] = a.z; x.v[3] = a.w;
    x.v[4] = b.x; x.v[5] = b.y; x.v[6] = b.z; x.v[7] = b.w;
    y.v[0] = c.x; y.v[1] = c.y; y.v[2] = c.z; y.v[3] = c.w;
    y.v[4] = d.x; y.v[5] = d.y; y.v[6] = d.z; y.v[7] = d.w;
  }
#else
  // host build (tests/emu): the same request / take order, the entry copied
  // when it is requested
  uint32_t buf[BV_ENTRY_U32];
  DEV void request(const uint32_t *e) {
    for (int k = 0; k < BV_ENTRY_U32; k++) buf[k] = e[k];
  }
  DEV void take(fe &x, fe &y) {
    for (int k = 0; k < 8; k++) x.v[k] = buf[k], y.v[k] = buf[8 + k];
  }
#endif
};

// The second GLV half's magnitude waits in LDS while the first half is
// summed (16 bytes per lane, read back by the lane that wrote them): four
// VGPRs fewer live through the first half's additions, which pays for the
// pipeline's own state (the next digit, the LDS address) within 128 VGPRs.
struct lane_park {
#if defined(__HIP_DEVICE_COMPILE__)
  DEV uint4 *slot() {
    __shared__ uint4 park[BV_STAGE_LANES];
    return park + threadIdx.x;
  }
  DEV void put(const uint32_t v[4]) { *slot() = make_uint4(v[0], v[1], v[2], v[3]); }
  DEV void get(uint32_t v[4]) {
    const uint4 a = *slot();
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
#else
  uint32_t buf[4];
  DEV void put(const uint32_t v[4]) {
    for (int c = 0; c < 4; c++) buf[c] = v[c];
  }
  DEV void get(uint32_t v[4]) {
    for (int c = 0; c < 4; c++) v[c] = buf[c];
  }
#endif
};

// kk = the magnitude of GLV half h (uniform): k1, or k2 (parked by the
// caller with park.put(k2) when PARK).
template <bool PARK>
DEV void glv_half(uint32_t kk[4], int h, const uint32_t k1[4], const uint32_t k2[4], lane_park &park) {
  if (PARK) {
    if (h) park.get(kk);
    else
#pragma unroll
      for (int c = 0; c < 4; c++) kk[c] = k1[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) kk[c] = h ? k2[c] : k1[c];
  }
}

// The next W-bit digit off the bottom of u (NL limbs, consumed).  SIGNED:
// carry recoding into (-2^(W-1), 2^(W-1)]: returns |d| (0 when d == 2^W)
// and dneg.
template <int W, int NL, bool SIGNED>
DEV uint32_t next_digit(uint32_t *u, uint32_t &carry, bool &dneg) {
  constexpr uint32_t ENT = 1u << (W - 1);
  uint32_t d = (u[0] & ((1u << W) - 1u)) + carry;
#pragma unroll
  for (int c = 0; c < NL - 1; c++) u[c] = (u[c] >> W) | (u[c + 1] << (32 - W));
  u[NL - 1] >>= W;
  dneg = false;
  if (SIGNED) {
    carry = d > ENT ? 1u : 0u;
    dneg = carry != 0;
    if (dneg) d = (1u << W) - d;
  }
  return d;
}

// R += sum_j T[j][digit_j(u)] over the 256-bit u1 (8 limbs, consumed:
// shifted right W bits per window, so digits never straddle limbs) with
// SIGNED digits in (-2^(W-1), 2^(W-1)] by carry recoding: T[j][|d|], y
// negated for d < 0 (geometry.h).  u < N < 2^256 and W NWIN >= 257, so no
// carry is left after the top window.
// FROM_INF (XYZZ only): R enters as the identity, so after window 0 it is
// that window's affine entry and window 1 adds with the 4M + 2S affine step
// (gexz_add_ge_aff) — 4 multiplies fewer per item.
// FINAL: only X and ZZ of the sum are read afterwards (final_check), so the
// top window's addition is the trimmed one (gexz_add_ge xz_only).
// DEFER (pipelined XYZZ loop only): the additions test P only when `chk`
// (BV_DEFER_EXC above); the caller tests ZZ after its last loop.
// YALT (pipelined XYZZ loop only; BV_Y_ALT above): *ys is the accumulator's
// state, read on entry and updated on return.
template <int W, int NWIN, bool LAT = false, class PT = gej, bool FROM_INF = false, bool FINAL = false,
          bool DEFER = false, bool YALT = false>
DEV void g_table_add(PT &R, bool &inf, const uint32_t *tab, uint32_t u[8], bool chk = false, bool *ys = nullptr) {
  constexpr uint32_t ENT = 1u << (W - 1);
  static_assert(W * NWIN >= 257 && W < 32, "signed G windows must absorb the last carry");
  static_assert(!YALT || (y_alt(LAT, 1) && std::is_same<PT, gexz>::value),
                "alternating Y only in the pipelined throughput loop");
  static_assert(!DEFER || ((BV_LOOKUP_PIPE & 1) && !LAT && std::is_same<PT, gexz>::value),
                "deferred additions only in the pipelined throughput loop");
  uint32_t carry = 0;
  if constexpr ((BV_LOOKUP_PIPE & 1) && !LAT && std::is_same<PT, gexz>::value) {
    entry_stage stage;
    bool dneg;
    uint32_t d = next_digit<W, 8, true>(u, carry, dneg);
    stage.request(tab + (uint64_t)d * BV_ENTRY_U32);  // d == 0: the window's slot 0, valid and not added
    bool y0 = false;
    if constexpr (YALT) {
      y0 = *ys;
      *ys = y0 != ((NWIN & 1) != 0);
    }
#pragma unroll 1
    for (int j = 0; j < NWIN; j++) {
      fe x, y;
      stage.take(x, y);
      const uint32_t dj = d;
      // YALT: the opposite entry in the -S state, and for a lane at the
      // identity the entry of the state it enters (gexz_add_ge)
      const bool nj = YALT ? (dneg != (y0 != ((j & 1) != 0))) != inf : dneg;
      if (j + 1 < NWIN) {  // the same recoding as the entry consumed next: never an address off the table
        d = next_digit<W, 8, true>(u, carry, dneg);
        stage.request(tab + ((uint64_t)(j + 1) * ENT + d) * BV_ENTRY_U32);
      }
      fe_cneg_canon(y, nj);
      if constexpr (FROM_INF) {
        if (j == 1 && !inf) {  // R = window 0's entry (affine)
          if (dj != 0) {
            gexz_add_ge_aff<LAT, !DEFER, YALT>(R, inf, x, y, chk);
          } else {
            BV_STEP_COUNT(skip);
            if (YALT) fe_neg(R.Y, R.Y);
          }
          continue;
        }
      }
      pt_add_ge_step<LAT, !DEFER, YALT>(R, inf, x, y, dj != 0, FINAL && j == NWIN - 1, chk);
    }
    return;
  }
  for (int j = 0; j < NWIN; j++) {
    bool dneg;
    const uint32_t d = next_digit<W, 8, true>(u, carry, dneg);
    // loaded unconditionally (d == 0 reads the window's slot 0, a valid
    // entry that is then not added): no per-lane branch around the lookup
    const uint32_t *e = tab + ((uint64_t)j * ENT + d) * BV_ENTRY_U32;
    fe x, y;
    fe_load4(x, e);
    fe_load4(y, e + 8);
    fe_cneg_canon(y, dneg);
    if constexpr (FROM_INF) {
      if (j == 1 && !inf) {  // R = window 0's entry (affine)
        if (d != 0) gexz_add_ge_aff<LAT>(R, inf, x, y);
        continue;
      }
    }
    pt_add_ge_step<LAT>(R, inf, x, y, d != 0, FINAL && j == NWIN - 1);
  }
}

// k1 magnitude, k2 magnitude (4 limbs each) and the sign word
DEV void load_k(uint32_t k1[4], uint32_t k2[4], uint32_t &signs, const uint32_t *u12, uint64_t i) {
  const uint4 *q = (const uint4 *)(u12 + (uint64_t)BV_U_STRIDE * i);
  uint4 a = q[0], b = q[1], c = q[2];
  k1[0] = a.x; k1[1] = a.y; k1[2] = a.z; k1[3] = a.w;
  k2[0] = b.x; k2[1] = b.y; k2[2] = b.z; k2[3] = b.w;
  signs = c.x;
}
DEV void store_k(uint32_t *u12, uint64_t i, const uint32_t k1[4], const uint32_t k2[4], uint32_t signs) {
  uint4 *q = (uint4 *)(u12 + (uint64_t)BV_U_STRIDE * i);
  q[0] = make_uint4(k1[0], k1[1], k1[2], k1[3]);
  q[1] = make_uint4(k2[0], k2[1], k2[2], k2[3]);
  q[2] = make_uint4(signs, 0u, 0u, 0u);
}

// Partial point R_G = u1 G (XYZZ), kept in HBM between k_verify_g and
// k_verify_q as 33 SoA words per item (X, Y, ZZ, ZZZ limbs, inf flag) for
// coalesced access.
#define RG_WORDS 33
DEV void rg_store(uint32_t *rg, uint64_t n, uint64_t i, const gexz &R, bool inf) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    rg[(uint64_t)k * n + i] = R.X.v[k];
    rg[(uint64_t)(8 + k) * n + i] = R.Y.v[k];
    rg[(uint64_t)(16 + k) * n + i] = R.ZZ.v[k];
    rg[(uint64_t)(24 + k) * n + i] = R.ZZZ.v[k];
  }
  rg[(uint64_t)32 * n + i] = inf ? 1u : 0u;
}
DEV void rg_load(const uint32_t *rg, uint64_t n, uint64_t i, gexz &R, bool &inf) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    R.X.v[k] = rg[(uint64_t)k * n + i];
    R.Y.v[k] = rg[(uint64_t)(8 + k) * n + i];
    R.ZZ.v[k] = rg[(uint64_t)(16 + k) * n + i];
    R.ZZZ.v[k] = rg[(uint64_t)(24 + k) * n + i];
  }
  inf = rg[(uint64_t)32 * n + i] != 0;
}

// Phase 1 (overlaps the key-table build): R_G = u1 G for items that reach
// the math.
// k_glv_split, item i (per-batch key tables, device entry): u2 = r s^-1 and
// its GLV split into u12 as soon as s^-1 is known — on the s^-1 stream,
// beside SHA-256 and the key tables — so k_verify_g forms only u1 = e s^-1
// (the digest's product).  Items whose s is unusable get a split of a
// dummy w that k_verify_q never reads (it classifies first).
DEV void glv_split_item(uint64_t i, const uint32_t *r_be, const uint32_t *w_in, uint32_t *u12) {
  sc w;
  uint32_t k1[4], k2[4], signs;
  sc_load_w(w, w_in, i);
  u2_split_of(i, r_be, w, k1, k2, signs);
  store_k(u12, i, k1, k2, signs);
}

// SPLIT: u12 already holds the GLV split (k_glv_split); else it is formed
// here with u1.
template <bool LAT = false, bool SPLIT = false>
DEV void verify_item_g(uint64_t i, uint64_t n, const uint32_t *item_key, const uint32_t *r_be, const uint32_t *s_be,
                       const uint8_t *pre, const uint8_t *kstatus, const uint32_t *item_msg,
                       const uint32_t *digest_words, const uint32_t *w_in, uint32_t *u12, const uint32_t *g_table,
                       uint32_t *rg) {
  constexpr bool DEFER = BV_DEFER_EXC != 0 && (BV_LOOKUP_PIPE & 1) != 0 && !LAT;
  fe r;
  if (classify_item(i, item_key, r_be, s_be, pre, kstatus, r) != 0xFF) return;
  for (bool chk = false;; chk = true) {  // a second pass only for a flagged item (BV_DEFER_EXC)
    chk = defer_uniform(chk);
    uint32_t u[8];
    if (SPLIT) {
      sc w;
      sc_load_w(w, w_in, i);
      u1_of(i, item_msg, digest_words, w, u);
    } else {
      uint32_t k1[4], k2[4], signs;
      item_scalars(i, r_be, item_msg, digest_words, w_in, u, k1, k2, signs);
      store_k(u12, i, k1, k2, signs);
    }
    gexz R;
    bool inf;
    pt_set_identity(R, inf);
    bool yn = false;  // BV_Y_ALT: R holds the opposite of the sum
    g_table_add<BV_GW, BV_GNWIN, LAT, gexz, true, false, DEFER, y_alt(LAT, 1)>(R, inf, g_table, u, chk, &yn);
    y_true(R, yn);  // R_G is stored with its true Y
    // ZZ == 0 <=> some step had P == 0 (the lemma at BV_DEFER_EXC).  On this
    // chain it cannot happen (the partial sums
    // of the signed digits are smaller than the next entry's scalar and the
    // total is u1 in (0, N)); the test stays, so that the stored R_G, from
    // which k_verify_q's chain starts, provably has ZZ != 0.
    if (defer_redo<DEFER>(R, inf, chk)) continue;
    rg_store(rg, n, i, R, inf);
    return;
  }
}

// R += sum_j T[j][digit_j(k)] over a 128-bit GLV half k (4 limbs; consumed:
// shifted right W bits per window, so digits never straddle limbs).
// SIGNED (K12): digits in (-2^(W-1), 2^(W-1)] by carry recoding, T[j][|d|]
// with y negated for d < 0; a window holds ENT = 2^(W-1) slots.  k < 2^128
// and W NWIN >= 129 bits, so no carry is left after the top window.
// `phi`: the table holds T (the k1 half) and this half needs phi(T) =
// (beta x, y): one multiply per lookup instead of a stored phi half (KC).
// `from_inf` (uniform; XYZZ only): R enters as the identity, so window 1
// adds to window 0's affine entry with the 4M + 2S step (as g_table_add).
// `neg` (the half's sign) is folded into each entry's sign: adding the
// negated entries to R gives the group element that negating R, adding the
// entries and negating back gives, without the two field negations.
// `last` (uniform; XYZZ throughput form): only X and ZZ of the sum are read
// afterwards, so the top window's addition is the trimmed one.
// DEFER / chk, YALT / ys: as g_table_add.
template <int W, int NWIN, bool SIGNED, bool LAT = false, class PT = gexz, bool DEFER = false, bool YALT = false>
DEV void key_table_add(PT &R, bool &inf, const uint32_t *tab, uint32_t k[4], bool neg, bool phi = false,
                       bool from_inf = false, bool last = false, bool chk = false, bool *ys = nullptr) {
  constexpr uint32_t ENT = SIGNED ? (1u << (W - 1)) : (1u << W);
  static_assert(!YALT || (y_alt(LAT, 2) && std::is_same<PT, gexz>::value),
                "alternating Y only in the pipelined throughput loop");
  static_assert(!SIGNED || W * NWIN >= 129, "signed windows must absorb the last carry");
  static_assert(!DEFER || ((BV_LOOKUP_PIPE & 2) && !LAT && std::is_same<PT, gexz>::value),
                "deferred additions only in the pipelined throughput loop");
  uint32_t carry = 0;
  if constexpr ((BV_LOOKUP_PIPE & 2) && !LAT && std::is_same<PT, gexz>::value) {
    entry_stage stage;
    bool dneg;
    uint32_t d = next_digit<W, 4, SIGNED>(k, carry, dneg);
    stage.request(tab + (uint64_t)d * BV_ENTRY_U32);  // d == 0: a valid, unused slot
    bool y0 = false;
    if constexpr (YALT) {
      y0 = *ys;
      *ys = y0 != ((NWIN & 1) != 0);
    }
#pragma unroll 1
    for (int j = 0; j < NWIN; j++) {
      fe x, y;
      stage.take(x, y);
      const uint32_t dj = d;
      // YALT: as g_table_add, folded into the same sign as the half's
      const bool nj = YALT ? ((dneg != neg) != (y0 != ((j & 1) != 0))) != inf : dneg != neg;
      if (j + 1 < NWIN) {  // the same recoding as the entry consumed next: never an address off the table
        d = next_digit<W, 4, SIGNED>(k, carry, dneg);
        stage.request(tab + ((uint64_t)(j + 1) * ENT + d) * BV_ENTRY_U32);
      }
      if (phi) {
        fe beta;
        fe_load(beta, FE_BETA);
        fe_mul(x, x, beta);
      }
      fe_cneg_canon(y, nj);
      if (from_inf && j == 1 && !inf) {  // R = window 0's entry (affine)
        if (dj != 0) {
          gexz_add_ge_aff<LAT, !DEFER, YALT>(R, inf, x, y, chk);
        } else {
          BV_STEP_COUNT(skip);
          if (YALT) fe_neg(R.Y, R.Y);
        }
        continue;
      }
      pt_add_ge_step<LAT, !DEFER, YALT>(R, inf, x, y, dj != 0, last && j == NWIN - 1, chk);
    }
    return;
  }
  constexpr bool fold = !LAT;  // the latency variants keep negating the accumulator around the half
  if (!fold && neg) fe_neg(R.Y, R.Y);
  for (int j = 0; j < NWIN; j++) {
    bool dneg;
    const uint32_t d = next_digit<W, 4, SIGNED>(k, carry, dneg);
    const uint32_t *e = tab + ((uint64_t)j * ENT + d) * BV_ENTRY_U32;  // d == 0: a valid, unused slot
    fe x, y;
    fe_load4(x, e);
    fe_load4(y, e + 8);
    if (phi) {
      fe beta;
      fe_load(beta, FE_BETA);
      fe_mul(x, x, beta);
    }
    fe_cneg_canon(y, dneg != (fold && neg));
    if constexpr (std::is_same<PT, gexz>::value) {
      if (from_inf && j == 1 && !inf) {  // R = window 0's entry (affine)
        if (d != 0) gexz_add_ge_aff<LAT>(R, inf, x, y);
        continue;
      }
    }
    pt_add_ge_step<LAT>(R, inf, x, y, d != 0, last && j == NWIN - 1);
  }
  if (!fold && neg) fe_neg(R.Y, R.Y);
}

// A key's table of W-bit windows: SIGNED digits for every geometry but K8;
// KC (the cached geometries): one stored half, phi(T) formed per lookup;
// `half`: the words of one stored half.
template <int W, int NWIN>
struct key_geom {
  static constexpr bool SIGNED = W != BV_KW;
  static constexpr bool KC = BV_W_IS_CACHED(W);
  static constexpr uint64_t half =
      SIGNED ? ((uint64_t)NWIN * (1ull << (W - 1)) + 1) * BV_ENTRY_U32 : (uint64_t)NWIN * (1ull << W) * BV_ENTRY_U32;
  static_assert(W != BV_K12W || half == BV_K12HALF_U32, "K12 geometry");
  static_assert(W != BV_KCW || half == BV_KCHALF_U32, "KC geometry");
  static_assert(W != BV_KC18W || half == BV_KC18HALF_U32, "KC18 geometry");
};
// The table of item i's key.  key_tabs != null (key cache): per-batch-key
// table base addresses, null for a key without a table; else the tables are
// contiguous in key_table (per-batch K8 / K12 build).
template <int W, int NWIN>
DEV const uint32_t *key_table_of(const uint32_t *item_key, uint64_t i, const uint32_t *key_table,
                                 const uint64_t *key_tabs) {
  using G = key_geom<W, NWIN>;
  return key_tabs ? (const uint32_t *)key_tabs[item_key[i]]
                  : key_table + (uint64_t)item_key[i] * (G::KC ? 1 : 2) * G::half;
}

// R += k1 T + k2 phi(T) over the key's table (the second stored half, or
// phi of the first when KC).  One loop body for both GLV halves (one inlined
// copy of the point addition: smaller code, fewer live registers than two
// calls).  from_inf_first: R enters the first half as the identity;
// last_second: only X and ZZ are read after the second half (key_table_add).
template <int W, int NWIN, bool LAT, bool DEFER>
DEV void key_halves_add(gexz &R, bool &inf, const uint32_t *tab, const uint32_t k1[4], const uint32_t k2[4],
                        uint32_t signs, bool from_inf_first, bool last_second, bool chk, bool *yn) {
  using G = key_geom<W, NWIN>;
  constexpr bool PARK = (BV_LOOKUP_PIPE & 2) && !LAT;
  lane_park park;
  if (PARK) park.put(k2);
#pragma unroll 1
  for (int h = 0; h < 2; h++) {
    uint32_t kk[4];
    glv_half<PARK>(kk, h, k1, k2, park);
    key_table_add<W, NWIN, G::SIGNED, LAT, gexz, DEFER, y_alt(LAT, 2)>(
        R, inf, tab + (h && !G::KC ? G::half : 0), kk, (signs >> h) & 1u, G::KC && h, from_inf_first && h == 0,
        last_second && h == 1, chk, yn);
  }
}

// Phase 2: R = R_G + k1 Q + k2 phi(Q) with the key's two half-tables;
// final check -> status.
template <int W, int NWIN, bool LAT = false>
DEV uint8_t verify_item_q(uint64_t i, uint64_t n, const uint32_t *item_key, const uint32_t *r_be,
                          const uint32_t *s_be, const uint8_t *pre, const uint8_t *kstatus, const uint32_t *u12,
                          const uint32_t *key_table, const uint64_t *key_tabs, const uint32_t *rg) {
  constexpr bool DEFER = BV_DEFER_EXC != 0 && (BV_LOOKUP_PIPE & 2) != 0 && !LAT;
  fe r;
  const uint8_t st = classify_item(i, item_key, r_be, s_be, pre, kstatus, r);
  if (st != 0xFF) return st;
  const uint32_t *tab = key_table_of<W, NWIN>(item_key, i, key_table, key_tabs);
  if (!tab) return BV_DEFERRED;  // key cache, partial batch: no table for this key
  for (bool chk = false;; chk = true) {  // a second pass only for a flagged item (BV_DEFER_EXC)
    chk = defer_uniform(chk);
    uint32_t k1[4], k2[4], signs;
    load_k(k1, k2, signs, u12, i);
    gexz R;
    bool inf;
    rg_load(rg, n, i, R, inf);
    bool yn = false;  // BV_Y_ALT: R_G comes with its true Y; final_check reads no Y
    key_halves_add<W, NWIN, LAT, DEFER>(R, inf, tab, k1, k2, signs, false, true, chk, &yn);
    // ZZ == 0 <=> some step of either half had P == 0 (the lemma at
    // BV_DEFER_EXC; R_G entered with ZZ != 0: k_verify_g tested it).  The
    // flagged item starts again from R_G and u12 in memory, every step
    // checked.
    if (defer_redo<DEFER>(R, inf, chk)) continue;
    fe_load_be_words(r, r_be + 8 * i);  // reloaded: not kept live through the loop
    return final_check(R, inf, r) ? BV_ACCEPT : BV_REJECT;
  }
}

// Key part first, for host entries whose messages are still crossing PCIe:
// u2 = r s^-1 needs no digest, so R_Q = k1 Q + k2 phi(Q) is summed as soon
// as r, s, the keys and their tables are in HBM (k_verify_qf), and only
// u1 G and the decision wait for each chunk's digests (k_verify_gf).  The
// same additions as verify_item_g + verify_item_q in the other order; R_Q
// goes through the R_G buffer (rg_store), and no u12 round trip.
template <int W, int NWIN, bool LAT = false>
DEV void verify_item_qfirst(uint64_t i, uint64_t n, const uint32_t *item_key, const uint32_t *r_be,
                            const uint32_t *s_be, const uint8_t *pre, const uint8_t *kstatus, const uint32_t *w_in,
                            const uint32_t *key_table, const uint64_t *key_tabs, uint32_t *rq) {
  constexpr bool DEFER = BV_DEFER_EXC != 0 && (BV_LOOKUP_PIPE & 2) != 0 && !LAT;
  fe r;
  if (classify_item(i, item_key, r_be, s_be, pre, kstatus, r) != 0xFF) return;
  const uint32_t *tab = key_table_of<W, NWIN>(item_key, i, key_table, key_tabs);
  if (!tab) {  // key cache, partial batch: k_verify_gf leaves the item BV_DEFERRED
    rq[(uint64_t)32 * n + i] = 2u;
    return;
  }
  for (bool chk = false;; chk = true) {  // a second pass only for a flagged item (BV_DEFER_EXC)
    chk = defer_uniform(chk);
    uint32_t k1[4], k2[4], signs;
    {
      sc w;
      sc_load_w(w, w_in, i);
      u2_split_of(i, r_be, w, k1, k2, signs);
    }
    gexz R;
    bool inf;
    pt_set_identity(R, inf);
    bool yn = false;  // BV_Y_ALT: R holds the opposite of the sum
    key_halves_add<W, NWIN, LAT, DEFER>(R, inf, tab, k1, k2, signs, true, false, chk, &yn);
    y_true(R, yn);  // R_Q is stored with its true Y
    // ZZ == 0 <=> some step had P == 0 (the lemma at BV_DEFER_EXC; the
    // chain starts from the identity).  The flagged item starts again from
    // w_in, every step checked, so the stored R_Q has ZZ != 0 when
    // k_verify_gf continues from it.
    if (defer_redo<DEFER>(R, inf, chk)) continue;
    rg_store(rq, n, i, R, inf);
    return;
  }
}

template <bool LAT = false>
DEV uint8_t verify_item_gfinish(uint64_t i, uint64_t n, const uint32_t *item_key, const uint32_t *r_be,
                                const uint32_t *s_be, const uint8_t *pre, const uint8_t *kstatus,
                                const uint32_t *item_msg, const uint32_t *digest_words, const uint32_t *w_in,
                                const uint32_t *g_table, const uint32_t *rq) {
  fe r;
  const uint8_t st = classify_item(i, item_key, r_be, s_be, pre, kstatus, r);
  if (st != 0xFF) return st;
  if (rq[(uint64_t)32 * n + i] == 2u) return BV_DEFERRED;  // no key table (k_verify_qf)
  constexpr bool DEFER = BV_DEFER_EXC != 0 && (BV_LOOKUP_PIPE & 1) != 0 && !LAT;
  for (bool chk = false;; chk = true) {  // a second pass only for a flagged item (BV_DEFER_EXC)
    chk = defer_uniform(chk);
    uint32_t u[8];
    {
      sc w;
      sc_load_w(w, w_in, i);
      u1_of(i, item_msg, digest_words, w, u);
    }
    gexz R;
    bool inf;
    rg_load(rq, n, i, R, inf);
    // BV_Y_ALT is not applied here: the alternating form raised k_verify_gf's
    // scratch (44 -> 48 B), and this kernel waits for PCIe, not for its VALU
    g_table_add<BV_GW, BV_GNWIN, LAT, gexz, false, true, DEFER>(R, inf, g_table, u, chk);
    // ZZ == 0 <=> some G step had P == 0 (the lemma at BV_DEFER_EXC; R_Q
    // entered with ZZ != 0: k_verify_qf tested it).  G entries added to
    // R_Q can meet R_Q itself or its opposite, so here the test does fire:
    // the flagged item starts again from R_Q in memory, every step checked.
    if (defer_redo<DEFER>(R, inf, chk)) continue;
    fe_load_be_words(r, r_be + 8 * i);
    return final_check(R, inf, r) ? BV_ACCEPT : BV_REJECT;
  }
}

// Key-cache path in ONE pass (k_verify_gq): R = u1 G + k1 T + k2 phi(T) with
// the G table and the key's cached table, R_G kept in registers (no HBM
// round trip of R_G / u12 between two kernels, no kernel boundary).  Same
// decisions as verify_item_g followed by verify_item_q.  <W, NWIN>: the
// context's cached geometry (KC or KC18).
template <int W, int NWIN, bool LAT = false>
DEV uint8_t verify_item_gq_kc(uint64_t i, const uint32_t *item_key, const uint32_t *r_be, const uint32_t *s_be,
                              const uint8_t *pre, const uint8_t *kstatus, const uint32_t *item_msg,
                              const uint32_t *digest_words, const uint32_t *w_in, const uint32_t *g_table,
                              const uint64_t *key_tabs) {
  static_assert(BV_W_IS_CACHED(W), "a cached geometry");
  fe r;
  const uint8_t st = classify_item(i, item_key, r_be, s_be, pre, kstatus, r);
  if (st != 0xFF) return st;
  const uint32_t *tab = (const uint32_t *)key_tabs[item_key[i]];
  if (!tab) return BV_DEFERRED;  // partial batch: no table for this key
  // deferred only when both loops are the pipelined ones: one test for the item
  constexpr bool DEFER = BV_DEFER_EXC != 0 && BV_LOOKUP_PIPE == 3 && !LAT;
  for (bool chk = false;; chk = true) {  // a second pass only for a flagged item (BV_DEFER_EXC)
    chk = defer_uniform(chk);
    uint32_t u[8], k1[4], k2[4], signs;
    item_scalars(i, r_be, item_msg, digest_words, w_in, u, k1, k2, signs);
    gexz R;
    bool inf;
    pt_set_identity(R, inf);
    bool yn = false;  // BV_Y_ALT: R holds the opposite of the sum; final_check reads no Y
    g_table_add<BV_GW, BV_GNWIN, LAT, gexz, true, false, DEFER, y_alt(LAT, 1)>(R, inf, g_table, u, chk, &yn);
    if (!y_alt(LAT, 2)) y_true(R, yn);
    key_halves_add<W, NWIN, LAT, DEFER>(R, inf, tab, k1, k2, signs, false, true, chk, &yn);
    // ZZ == 0 <=> some step of the G chain or of either half had P == 0
    // (the lemma at BV_DEFER_EXC; the item's one chain starts from the
    // identity).  The flagged item starts again, every step checked.
    if (defer_redo<DEFER>(R, inf, chk)) continue;
    fe_load_be_words(r, r_be + 8 * i);
    return final_check(R, inf, r) ? BV_ACCEPT : BV_REJECT;
  }
}

// One signature item without a key table: k1 Q + k2 phi(Q) by a joint
// (Strauss-Shamir) per-lane double-and-add over the 128-bit GLV halves.
template <bool LAT = false>
DEV uint8_t verify_item_generic(uint64_t i, const uint32_t *item_key, const uint32_t *r_be, const uint32_t *s_be,
                                const uint8_t *pre, const uint8_t *kstatus, const uint32_t *kxy,
                                const uint32_t *item_msg, const uint32_t *digest_words, const uint32_t *w_in,
                                const uint32_t *g_table) {
  fe r;
  const uint8_t st = classify_item(i, item_key, r_be, s_be, pre, kstatus, r);
  if (st != 0xFF) return st;
  const uint32_t k = item_key[i];
  uint32_t u1[8], k1[4], k2[4], signs;
  item_scalars(i, r_be, item_msg, digest_words, w_in, u1, k1, k2, signs);
  fe q1x, q1y, q2x, q2y, beta;
  fe_load(q1x, kxy + 16 * k);
  fe_load(q1y, kxy + 16 * k + 8);
  fe_load(beta, FE_BETA);
  fe_mul(q2x, q1x, beta);  // phi(Q) = (beta x, y)
  q2y = q1y;
  if (signs & 1u) fe_neg(q1y, q1y);
  if (signs & 2u) fe_neg(q2y, q2y);
  gej R;
  bool inf;
  pt_set_identity(R, inf);
  for (int bit = 127; bit >= 0; bit--) {
    if (!inf) gej_double_sel<LAT>(R, R);
    if ((k1[bit >> 5] >> (bit & 31)) & 1u) gej_add_ge_sel<LAT>(R, inf, q1x, q1y);
    if ((k2[bit >> 5] >> (bit & 31)) & 1u) gej_add_ge_sel<LAT>(R, inf, q2x, q2y);
  }
  g_table_add<BV_GW, BV_GNWIN, LAT>(R, inf, g_table, u1);
  return final_check(R, inf, r) ? BV_ACCEPT : BV_REJECT;
}

// ---------------------------------------------------------------------------
// Small batches (k_small: one workgroup per item, every step of one item's
// verification in one launch).  The pieces below are the
// per-lane work of its roles.
// ---------------------------------------------------------------------------
// w = s^-1 R (Montgomery form, as k_sinv makes it) for one item: the plain
// inverse R^2 / s of s (taken as (s/R) R), times 1.
DEV void sinv_one(sc &w, const sc &s) {
  sc t, one;
#pragma unroll
  for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u;
  sc_inverse_var(t, s);
  sc_mont(w, t, one);
}

// u1 = e w and the GLV split of u2 = r w (item_scalars over values)
DEV void scalars_from(const sc &w, const sc &e, const sc &r, uint32_t u1[8], uint32_t k1[4], uint32_t k2[4],
                      uint32_t &signs) {
  u1_from(e, w, u1);
  u2_split_from(r, w, k1, k2, signs);
}

// g_table_add over windows [j0, j1) only: the signed recoding runs over
// every window (a digit depends on the carry out of the window below), the
// table additions only in the range — so lanes can sum disjoint ranges.
template <int W, int NWIN, bool LAT = false, class PT = gexz>
DEV void g_table_add_range(PT &R, bool &inf, const uint32_t *tab, uint32_t u[8], int j0, int j1) {
  constexpr uint32_t ENT = 1u << (W - 1);
  uint32_t carry = 0;
  for (int j = 0; j < NWIN; j++) {
    bool dneg;
    const uint32_t d = next_digit<W, 8, true>(u, carry, dneg);
    if (j < j0 || j >= j1) continue;
    const uint32_t *e = tab + ((uint64_t)j * ENT + d) * BV_ENTRY_U32;
    fe x, y;
    fe_load4(x, e);
    fe_load4(y, e + 8);
    fe_cneg_canon(y, dneg);
    pt_add_ge_step<LAT>(R, inf, x, y, d != 0);
  }
}

// R = k P for an affine P and a 128-bit k (4 limbs), MSB-first over the
// non-adjacent form of k (digits in {-1, 0, 1}, ~k/3 additions): a key
// without a table (the small-batch kernel's cold path).  pos / neg digit
// masks: c = 3k ^ k, pos = (c & 3k) >> 1, neg = (c & k) >> 1.
template <bool LAT = false>
DEV void naf_mul(gej &R, bool &inf, const fe &px, const fe &py, const uint32_t k[4]) {
  uint32_t h[5], kk[5], pos[5], neg[5];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) kk[i] = k[i];
  kk[4] = 0;
  // h = 3k = k + 2k
  uint32_t prev = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint32_t k2 = (kk[i] << 1) | (prev >> 31);
    prev = kk[i];
    h[i] = addc32(kk[i], k2, c);
  }
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint32_t x = h[i] ^ kk[i];
    pos[i] = x & h[i];
    neg[i] = x & kk[i];
  }
#pragma unroll
  for (int i = 0; i < 5; i++) {  // >> 1
    pos[i] = (pos[i] >> 1) | (i < 4 ? pos[i + 1] << 31 : 0u);
    neg[i] = (neg[i] >> 1) | (i < 4 ? neg[i + 1] << 31 : 0u);
  }
  fe ny;
  fe_neg(ny, py);
  pt_set_identity(R, inf);
  for (int bit = 129; bit >= 0; bit--) {
    if (!inf) gej_double_sel<LAT>(R, R);
    const uint32_t p = (pos[bit >> 5] >> (bit & 31)) & 1u, n = (neg[bit >> 5] >> (bit & 31)) & 1u;
    if (p | n) gej_add_ge_sel<LAT>(R, inf, px, n ? ny : py);
  }
}

// One leaf of k_small's sum tree: the entry window j of u (NW limbs of 32
// bits, consumed; W-bit SIGNED digits by carry recoding, as g_table_add /
// key_table_add) contributes: (x, y) with y negated for a negative digit,
// XOR `neg` (the GLV half's sign); `phi`: (beta x, y) of the stored entry;
// *zero: the digit is 0 (the leaf is the identity).  The recoding runs over
// windows 0..j (a digit depends on the carry out of the window below).
// Returns the slot it read, j ENT + |d| (the CPU replay of the warm leaves,
// tests/kcsmall, holds it to the stored slots; the kernels drop it).
template <int W, int NW>
DEV uint64_t table_leaf(fe &x, fe &y, bool &zero, const uint32_t *tab, uint32_t u[NW], int j, bool neg, bool phi) {
  constexpr uint32_t ENT = 1u << (W - 1);
  uint32_t carry = 0, d = 0;
  bool dneg = false;
  for (int w = 0; w <= j; w++) d = next_digit<W, NW, true>(u, carry, dneg);  // the last digit is window j's
  zero = d == 0;
  const uint64_t slot = (uint64_t)j * ENT + d;
  const uint32_t *e = tab + slot * BV_ENTRY_U32;  // d == 0: a valid, unused slot
  fe_load4(x, e);
  fe_load4(y, e + 8);
  if (phi) {
    fe beta;
    fe_load(beta, FE_BETA);
    fe_mul(x, x, beta);
  }
  fe_cneg_canon(y, dneg != neg);
  return slot;
}

// Leaves of k_small's warm tree (a key with a key-cache table of the cached
// geometry <KW, KNWIN>: KC <22, 6> or KC18 <18, 8>): BV_GNWIN G leaves, then
// 2 KNWIN table leaves.
template <int KNWIN>
struct small_warm {
  static constexpr int kLeaves = BV_GNWIN + 2 * KNWIN;  // 22 (KC), 26 (KC18)
  static constexpr int kNodes = (kLeaves + 1) / 2;      // XYZZ nodes after the leaf pairs: 11, 13
};
// Table leaf q of 2 KNWIN (lane BV_GNWIN + q of wave 0): q < KNWIN is window q
// of k1 on T, the others window q - KNWIN of k2 on phi(T) = (beta x, y) of
// the same stored entries.  k12 = k1[4] | k2[4] (magnitudes), signs bit h =
// half h is negative.  The layout is verify_item_q's for a cached W: ONE
// stored half of KNWIN 2^(KW-1) + 1 entries (BV_KCHALF_U32 / BV_KC18HALF_U32),
// slot j ENT + |d| with |d| <= ENT, so every read is inside the allocation:
// a zero digit reads slot j ENT (the digit ENT of window j - 1 for j >= 1,
// the never-written slot 0 for j = 0; the leaf is flagged zero either way),
// and a half below 2^128 leaves the top window of KC18 (bits 126, 127 and
// the carry) digits 0..4, all in the first stored block of its window.
template <int KW, int KNWIN>
DEV uint64_t small_table_leaf(fe &x, fe &y, bool &zero, const uint32_t *tab, const uint32_t k12[8], uint32_t signs,
                              uint32_t q) {
  static_assert(BV_W_IS_CACHED(KW) && KW * KNWIN >= 129 && KW * (KNWIN - 1) < 128, "a cached geometry over a GLV half");
  static_assert(key_geom<KW, KNWIN>::half == (KW == BV_KCW ? BV_KCHALF_U32 : BV_KC18HALF_U32),
                "the stored half of the cached geometry");
  const uint32_t h = q / KNWIN;
  uint32_t kk[4];
#pragma unroll
  for (int k = 0; k < 4; k++) kk[k] = k12[4 * h + k];
  return table_leaf<KW, 4>(x, y, zero, tab, kk, (int)(q % KNWIN), (signs >> h) & 1u, h != 0);
}

// One XYZZ partial sum (+ identity flag) in 33 words (LDS hand-off)
DEV void part_store(uint32_t *p, const gexz &R, bool inf) {
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = R.X.v[k], p[8 + k] = R.Y.v[k], p[16 + k] = R.ZZ.v[k], p[24 + k] = R.ZZZ.v[k];
  p[32] = inf ? 1u : 0u;
}
DEV void part_load(const uint32_t *p, gexz &R, bool &inf) {
#pragma unroll
  for (int k = 0; k < 8; k++) R.X.v[k] = p[k], R.Y.v[k] = p[8 + k], R.ZZ.v[k] = p[16 + k], R.ZZZ.v[k] = p[24 + k];
  inf = p[32] != 0;
}
