// audit.h — TEST INFRASTRUCTURE: the relations that tie every entry of a
// fixed-base table (babble_amd/csrc/geometry.h) to its neighbours, written
// with field.h primitives only and compilable for the host and the device.
// None of the table-build code is used: the relations are the cross-multiplied
// affine addition and doubling formulas, so no inversion is needed.
//
// Window j of a table for the point Q holds T[j][d] = d 2^(W j) Q.
//   R0 anchor  T[0][1] is the key's input point, word for word.
//   R1 step    T[j][d] = T[j][d-1] + T[j][1] for every required d >= 2
//              (d = 2: the doubling form).
//   R2 link    signed tables: T[j][1] = 2 T[j-1][2^(W-1)];
//              K8 (unsigned): T[j][1] = T[j-1][255] + T[j-1][1].
//   R3 form    both coordinates of a required entry are below p and the entry
//              is not (0, 0); K8 slot 0 of every window is (0, 0) in both halves.
//   R4 phi     phi[j][d] = (beta x mod p, y) of T[j][d], canonical.
// With R0 as the anchor, R1 walks every window and R2 steps from one window to
// the next, so all relations holding means every required entry is the
// multiple of the key it must be.
//
// Required digits.  The verify kernels recode a scalar u < 2^BITS window by
// window (verify_core.h next_digit, as g_table_add and key_table_add call it):
// window j sees v_j = floor(u / 2^(W j)) mod 2^W plus the carry of window j-1.
//   Signed: raw = v_j + carry is in [0, 2^W]; raw > 2^(W-1) becomes the digit
//   2^W - raw with a carry, so |digit| <= 2^(W-1) in every window.  Above the
//   scalar, where BITS - W j < W, floor(u / 2^(W j)) < 2^(BITS - W j), hence
//   raw <= 2^(BITS - W j); once BITS - W j <= W - 1 that is at most 2^(W-1),
//   nothing is negated, no carry leaves the window, and the digits read are
//   1 .. 2^(BITS - W j).  So window j needs 1 .. min(2^(W-1), 2^(BITS - W j)).
//   Unsigned (K8, 16 windows over 128 bits): every window reads 1 .. 2^W - 1.
// BITS is 256 for the generator table (u1 < N < 2^256) and 128 for the key
// tables: glv_split returns magnitudes below 2^128 (tests/test_glv_int.py).
// Digit 0 is never added (slot 0 of a signed window holds the digit 2^(W-1) of
// the window below; slot 0 of window 0, the pad entry after the top window and
// the top window's slots past its last required digit are not audited).
#pragma once
#include "../../babble_amd/csrc/field.h"

#define TC_ENTRY_U32 16  // affine x, y: 8 + 8 little-endian words

enum { TC_R0 = 0, TC_R1 = 1, TC_R2 = 2, TC_R3 = 3, TC_R4 = 4 };

struct tc_geom {
  uint32_t w;          // window bits
  uint32_t nwin;       // windows
  uint32_t bits;       // width of the scalar the table serves
  uint32_t is_signed;  // signed digits (G, K12, KC, KC18) or unsigned (K8)
  uint32_t phi;        // a stored phi half follows the plain half (K8, K12)
};

// entry slots per window
DEV uint64_t tc_ent(const tc_geom &g) { return g.is_signed ? 1ull << (g.w - 1) : 1ull << g.w; }

// the largest digit window j must hold (see the derivation above)
DEV uint64_t tc_required(const tc_geom &g, uint32_t j) {
  if (!g.is_signed) return (1ull << g.w) - 1;
  const int64_t live = (int64_t)g.bits - (int64_t)g.w * (int64_t)j;
  if (live < 0) return 0;
  if (live >= (int64_t)g.w - 1) return 1ull << (g.w - 1);
  return 1ull << live;
}

// the slot of digit d of window j: a signed window's top digit 2^(W-1) lives
// in slot 0 of window j + 1
DEV uint64_t tc_slot(const tc_geom &g, uint32_t j, uint64_t d) {
  const uint64_t ent = tc_ent(g);
  if (g.is_signed && d == ent) return ((uint64_t)j + 1) * ent;
  return (uint64_t)j * ent + d;
}

// words of one half (signed: one pad entry after the top window)
DEV uint64_t tc_half_u32(const tc_geom &g) {
  return ((uint64_t)g.nwin * tc_ent(g) + (g.is_signed ? 1 : 0)) * TC_ENTRY_U32;
}

DEV uint64_t tc_table_u32(const tc_geom &g) { return tc_half_u32(g) * (g.phi ? 2 : 1); }

// required entries of one half
DEV uint64_t tc_required_total(const tc_geom &g) {
  uint64_t n = 0;
  for (uint32_t j = 0; j < g.nwin; j++) n += tc_required(g, j);
  return n;
}

struct tc_pt {
  fe x, y;
};

DEV void tc_load(tc_pt &p, const uint32_t *e) {
  for (int i = 0; i < 8; i++) {
    p.x.v[i] = e[i];
    p.y.v[i] = e[8 + i];
  }
}

DEV bool tc_words_equal(const uint32_t *a, const uint32_t *b, int n) {
  uint32_t d = 0;
  for (int i = 0; i < n; i++) d |= a[i] ^ b[i];
  return d == 0;
}

DEV bool tc_is_zero_entry(const uint32_t *e) {
  uint32_t d = 0;
  for (int i = 0; i < TC_ENTRY_U32; i++) d |= e[i];
  return d == 0;
}

// a == b as field elements (both made canonical first)
DEV bool tc_eq(fe a, fe b) {
  fe_canon(a);
  fe_canon(b);
  return tc_words_equal(a.v, b.v, 8);
}

DEV bool tc_zero(fe a) {
  fe_canon(a);
  uint32_t d = 0;
  for (int i = 0; i < 8; i++) d |= a.v[i];
  return d == 0;
}

// R3: stored words are canonical (fe_canon changes nothing) and not (0, 0)
DEV bool tc_form_ok(const uint32_t *e) {
  tc_pt p, c;
  tc_load(p, e);
  c = p;
  fe_canon(c.x);
  fe_canon(c.y);
  return tc_words_equal(c.x.v, p.x.v, 8) && tc_words_equal(c.y.v, p.y.v, 8) && !tc_is_zero_entry(e);
}

// C = A + B by the chord through A and B, cross-multiplied:
//   H = xB - xA != 0, r = yB - yA,
//   (xC + xA + xB) H^2 = r^2,  (yC + yA) H = r (xA - xC)
DEV bool tc_chord_ok(const tc_pt &A, const tc_pt &B, const tc_pt &C) {
  fe H, r, H2, r2, t, l, m;
  fe_sub(H, B.x, A.x);
  if (tc_zero(H)) return false;
  fe_sub(r, B.y, A.y);
  fe_sqr(H2, H);
  fe_sqr(r2, r);
  fe_add(t, C.x, A.x);
  fe_add(t, t, B.x);
  fe_mul(l, t, H2);
  if (!tc_eq(l, r2)) return false;
  fe_add(t, C.y, A.y);
  fe_mul(l, t, H);
  fe_sub(t, A.x, C.x);
  fe_mul(m, r, t);
  return tc_eq(l, m);
}

// C = 2 A by the tangent at A, cross-multiplied (a = 0):
//   m = 3 xA^2, s = 2 yA != 0,
//   (xC + 2 xA) s^2 = m^2,  (yC + yA) s = m (xA - xC)
DEV bool tc_double_ok(const tc_pt &A, const tc_pt &C) {
  fe m, s, t, s2, m2, l, q;
  fe_sqr(t, A.x);
  fe_add(m, t, t);
  fe_add(m, m, t);
  fe_add(s, A.y, A.y);
  if (tc_zero(s)) return false;
  fe_sqr(s2, s);
  fe_sqr(m2, m);
  fe_add(t, C.x, A.x);
  fe_add(t, t, A.x);
  fe_mul(l, t, s2);
  if (!tc_eq(l, m2)) return false;
  fe_add(t, C.y, A.y);
  fe_mul(l, t, s);
  fe_sub(t, A.x, C.x);
  fe_mul(q, m, t);
  return tc_eq(l, q);
}

// R4: the phi entry is (beta x mod p, y) of the plain entry, word for word
DEV bool tc_phi_ok(const uint32_t *e, const uint32_t *phi) {
  tc_pt p;
  tc_load(p, e);
  fe beta, bx;
  for (int i = 0; i < 8; i++) beta.v[i] = FE_BETA[i];
  fe_mul(bx, p.x, beta);
  fe_canon(bx);
  fe_canon(p.y);
  return tc_words_equal(bx.v, phi, 8) && tc_words_equal(p.y.v, phi + 8, 8);
}

// Every relation of the required digit d (1 .. tc_required(g, j)) of window j
// of a signed table.  `tab`: the key's table, `kxy`: the key's 16 input words.
// Returns the failed relations as a bit mask (1 << TC_Rn).
DEV uint32_t tc_audit_signed(const tc_geom &g, const uint32_t *tab, const uint32_t *kxy, uint32_t j, uint64_t d) {
  const uint64_t ent = tc_ent(g);
  const uint32_t *c = tab + tc_slot(g, j, d) * TC_ENTRY_U32;
  uint32_t bad = 0;
  if (!tc_form_ok(c)) bad |= 1u << TC_R3;
  tc_pt A, B, C;
  tc_load(C, c);
  if (d == 1) {
    if (j == 0) {
      if (!tc_words_equal(c, kxy, TC_ENTRY_U32)) bad |= 1u << TC_R0;
    } else {
      tc_load(A, tab + tc_slot(g, j - 1, ent) * TC_ENTRY_U32);
      if (!tc_double_ok(A, C)) bad |= 1u << TC_R2;
    }
  } else {
    tc_load(A, tab + tc_slot(g, j, d - 1) * TC_ENTRY_U32);
    bool ok;
    if (d == 2) {
      ok = tc_double_ok(A, C);
    } else {
      tc_load(B, tab + tc_slot(g, j, 1) * TC_ENTRY_U32);
      ok = tc_chord_ok(A, B, C);
    }
    if (!ok) bad |= 1u << TC_R1;
  }
  if (g.phi && !tc_phi_ok(c, c + tc_half_u32(g))) bad |= 1u << TC_R4;
  return bad;
}

// The same for slot d (0 .. 2^W - 1) of window j of an unsigned table with a
// phi half (K8); d = 0 is the (0, 0) identity in both halves.
DEV uint32_t tc_audit_unsigned(const tc_geom &g, const uint32_t *tab, const uint32_t *kxy, uint32_t j, uint64_t d) {
  const uint64_t half = tc_half_u32(g);
  const uint32_t *c = tab + tc_slot(g, j, d) * TC_ENTRY_U32;
  if (d == 0) return tc_is_zero_entry(c) && (!g.phi || tc_is_zero_entry(c + half)) ? 0u : 1u << TC_R3;
  uint32_t bad = 0;
  if (!tc_form_ok(c)) bad |= 1u << TC_R3;
  tc_pt A, B, C;
  tc_load(C, c);
  if (d == 1) {
    if (j == 0) {
      if (!tc_words_equal(c, kxy, TC_ENTRY_U32)) bad |= 1u << TC_R0;
    } else {
      tc_load(A, tab + tc_slot(g, j - 1, tc_ent(g) - 1) * TC_ENTRY_U32);
      tc_load(B, tab + tc_slot(g, j - 1, 1) * TC_ENTRY_U32);
      if (!tc_chord_ok(A, B, C)) bad |= 1u << TC_R2;
    }
  } else {
    tc_load(A, tab + tc_slot(g, j, d - 1) * TC_ENTRY_U32);
    bool ok;
    if (d == 2) {
      ok = tc_double_ok(A, C);
    } else {
      tc_load(B, tab + tc_slot(g, j, 1) * TC_ENTRY_U32);
      ok = tc_chord_ok(A, B, C);
    }
    if (!ok) bad |= 1u << TC_R1;
  }
  if (g.phi && !tc_phi_ok(c, c + half)) bad |= 1u << TC_R4;
  return bad;
}
