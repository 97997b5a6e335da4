// P-384 (a = -3) Jacobian point arithmetic on fp384.h elements.
//
// Bounds (multiples of p, fp384.h's value contract). A Jacobian coordinate
// entering any formula is < 20p; every formula returns coordinates
// within that: doubling (18, 18, 6), mixed addition (9, 4, 3), full addition
// (8, 4, 2). An affine table coordinate is < 2p. Each line below carries the
// bound of its result in brackets; a product line also shows alpha beta, which
// stays far below fp384.h's limit of 2^15 (the largest is 23 * 69 = 1587 in
// the doubling; R / p = 2^8 makes a product's result alpha beta / 256 + 1).
//
// The three point operations are NOT inlined (BH_HDNI) and take pointers: a
// kernel keeps its points in private memory and each operation's temporaries
// in registers. One body per operation keeps the code small, and the memory
// traffic (42 words in, 42 out) is nothing beside 8 to 16 products of 392
// multiply-adds each.
//
// Exceptional cases are handled explicitly, with Go's nistec answers: either
// operand at infinity, equal operands (doubling), opposite operands
// (infinity). Verification data is public, so the branches are free to
// depend on it.
#pragma once
#include "fp384.h"

namespace bh {

using P384 = Fp_p384;

struct J384 {
  uint32_t x[14], y[14], z[14];
  uint32_t inf;  // 1: the point at infinity (x, y, z then unspecified)
};

BH_HD void j384_set_affine(J384* A, const uint32_t x[14], const uint32_t y[14]) {
  f384_copy(A->x, x);
  f384_copy(A->y, y);
  f384_const(A->z, P384::r1);
  A->inf = 0;
}

// y^2 = x^3 - 3x + b, x and y canonical Montgomery values
BH_HD bool j384_on_curve(const uint32_t x[14], const uint32_t y[14]) {
  uint32_t l[14], r[14], t[14], b[14];
  f384_sqr<P384>(l, y);          // [2p]
  f384_sqr<P384>(t, x);          // [2p]
  f384_mul<P384>(r, t, x);       // [2p]
  f384_muls<3>(t, x);            // [3p]
  f384_sub<P384, 3>(r, r, t);    // x^3 + 3p - 3x [5p]
  f384_const(b, Cv_p384::b_m);
  f384_add(r, r, b);             // [6p]
  f384_sub<P384, 6>(l, l, r);    // y^2 + 6p - rhs [8p]
  return f384_is_zero<P384>(l);
}

// A = 2A (dbl-2001-b). In: X, Y, Z < 20p. Out: X, Y < 18p, Z < 6p.
// j384_dbl_inl is the body; j384_dbl the shared out-of-line copy (see j384_madd).
BH_HD void j384_dbl_inl(J384* A) {
  if (A->inf) return;
  uint32_t delta[14], gamma[14], beta[14], alpha[14], t0[14], t1[14];
  f384_sqr<P384>(delta, A->z);           // 20*20 = 400 [3p]
  f384_sqr<P384>(gamma, A->y);           // 400 [3p]
  f384_mul<P384>(beta, A->x, gamma);     // 20*3 = 60 [2p]
  f384_sub<P384, 3>(t0, A->x, delta);    // X + 3p - delta [23p]
  f384_add(t1, A->x, delta);             // [23p]
  f384_muls<3>(t0, t0);                  // [69p]
  f384_mul<P384>(alpha, t1, t0);         // 23*69 = 1587 [8p]
  f384_mul<P384>(t0, A->y, A->z);        // 400 [3p]
  f384_muls<2>(A->z, t0);                // Z3 = 2 Y Z [6p]
  f384_sqr<P384>(t0, alpha);             // 64 [2p]
  f384_muls<8>(t1, beta);                // [16p]
  f384_sub<P384, 16>(A->x, t0, t1);      // X3 = alpha^2 + 16p - 8 beta [18p]
  f384_muls<4>(t1, beta);                // [8p]
  f384_sub<P384, 18>(t1, t1, A->x);      // 4 beta + 18p - X3 [26p]
  f384_mul<P384>(t0, alpha, t1);         // 8*26 = 208 [2p]
  f384_sqr<P384>(t1, gamma);             // 9 [2p]
  f384_muls<8>(t1, t1);                  // [16p]
  f384_sub<P384, 16>(A->y, t0, t1);      // Y3 = alpha (4 beta - X3) + 16p - 8 gamma^2 [18p]
}
inline BH_HDNI void j384_dbl(J384* A) { j384_dbl_inl(A); }

// A = A + (x2, y2), the affine point negated when neg. x2, y2 < 2p.
// In: A < 20p. Out: X < 9p, Y < 4p, Z < 3p.
// j384_madd_body is the body, inlined into its caller. j384_madd is the shared
// out-of-line copy (its rare doubling a call as well); j384_madd_inl has no
// call in it: k384_keywin (keys384.h) does nothing but mixed additions and
// keeps its one point in registers, at its own register count.
template <bool INL>
BH_HD void j384_madd_body(J384* A, const uint32_t x2[14], const uint32_t y2in[14], uint32_t neg) {
  uint32_t y2[14];
  if (neg) f384_sub<P384, 2>(y2, P384::km[0], y2in);  // 2p - y [2p]
  else f384_copy(y2, y2in);
  if (A->inf) {
    j384_set_affine(A, x2, y2);
    return;
  }
  uint32_t zz[14], u2[14], s2[14], h[14], r[14], z3[14], hh[14], hhh[14], v[14], t[14];
  f384_sqr<P384>(zz, A->z);              // 400 [3p]
  f384_mul<P384>(u2, x2, zz);            // 2*3 [2p]
  f384_mul<P384>(t, A->z, zz);           // 60 [2p]
  f384_mul<P384>(s2, y2, t);             // 4 [2p]
  f384_sub<P384, 20>(h, u2, A->x);       // U2 + 20p - X1 [22p]
  f384_sub<P384, 20>(r, s2, A->y);       // S2 + 20p - Y1 [22p]
  f384_mul<P384>(z3, A->z, h);           // 20*22 = 440 [3p]
  if (f384_is_zero_small<P384, 3>(z3)) { // H = 0 mod p (Z1 is not): same x
    if (f384_is_zero<P384>(r)) {
      j384_set_affine(A, x2, y2);        // A == T: 2T
      if (INL) j384_dbl_inl(A);
      else j384_dbl(A);
    } else {
      A->inf = 1;                        // A == -T
    }
    return;
  }
  f384_sqr<P384>(hh, h);                 // 484 [3p]
  f384_mul<P384>(hhh, h, hh);            // 66 [2p]
  f384_mul<P384>(v, A->x, hh);           // 60 [2p]
  f384_sqr<P384>(t, r);                  // 484 [3p]
  f384_muls<2>(u2, v);                   // [4p]
  f384_add(u2, u2, hhh);                 // HHH + 2V [6p]
  f384_sub<P384, 6>(A->x, t, u2);        // X3 = R^2 + 6p - HHH - 2V [9p]
  f384_sub<P384, 9>(t, v, A->x);         // V + 9p - X3 [11p]
  f384_mul<P384>(t, r, t);               // 22*11 = 242 [2p]
  f384_mul<P384>(v, A->y, hhh);          // 40 [2p]
  f384_sub<P384, 2>(A->y, t, v);         // Y3 [4p]
  f384_copy(A->z, z3);                   // Z3 = Z1 H [3p]
}
inline BH_HDNI void j384_madd(J384* A, const uint32_t x2[14], const uint32_t y2in[14], uint32_t neg) {
  j384_madd_body<false>(A, x2, y2in, neg);
}
BH_HD void j384_madd_inl(J384* A, const uint32_t x2[14], const uint32_t y2in[14], uint32_t neg) {
  j384_madd_body<true>(A, x2, y2in, neg);
}

// A = A + T, T negated when neg. In: both < 20p. Out: X < 8p, Y < 4p, Z < 2p.
// In the ladder of verify384.h the accumulator before the last window is
// 16c Q and the entry is d Q with u2 = 16c + d, so A == T needs 16c = d mod n:
// as n = 3 mod 16 that is u2 = n - 6 (16c = n - 3, d = -3), a public input
// (fixture record u2_eq_nm6); A == -T would need u2 = 0 mod n. Both branches
// are also exercised directly through the host harness (hs384_point_sum).
// The mixed addition's A == T branch is reached by Q = G, u1 = u2: the
// accumulator then equals the G-table entry being added.
inline BH_HDNI void j384_add(J384* A, const J384* T, uint32_t neg) {
  if (T->inf) return;
  uint32_t ty[14];
  if (neg) f384_sub<P384, 20>(ty, P384::km[0], T->y);  // 20p - Y2 [20p]
  else f384_copy(ty, T->y);
  if (A->inf) {
    f384_copy(A->x, T->x);
    f384_copy(A->y, ty);
    f384_copy(A->z, T->z);
    A->inf = 0;
    return;
  }
  uint32_t z1z1[14], z2z2[14], u1[14], u2[14], s1[14], s2[14], h[14], r[14], t[14], z3[14];
  f384_sqr<P384>(z1z1, A->z);            // 400 [3p]
  f384_sqr<P384>(z2z2, T->z);            // 400 [3p]
  f384_mul<P384>(u1, A->x, z2z2);        // 60 [2p]
  f384_mul<P384>(u2, T->x, z1z1);        // 60 [2p]
  f384_mul<P384>(t, T->z, z2z2);         // 60 [2p]
  f384_mul<P384>(s1, A->y, t);           // 40 [2p]
  f384_mul<P384>(t, A->z, z1z1);         // 60 [2p]
  f384_mul<P384>(s2, ty, t);             // 40 [2p]
  f384_sub<P384, 2>(h, u2, u1);          // U2 + 2p - U1 [4p]
  f384_sub<P384, 2>(r, s2, s1);          // S2 + 2p - S1 [4p]
  f384_mul<P384>(t, A->z, T->z);         // 400 [3p]
  f384_mul<P384>(z3, t, h);              // 12 [2p]
  if (f384_is_zero_small<P384, 2>(z3)) { // H = 0 mod p: same x
    if (f384_is_zero<P384>(r)) {
      f384_copy(A->x, T->x);             // A == T: 2T
      f384_copy(A->y, ty);
      f384_copy(A->z, T->z);
      j384_dbl(A);
    } else {
      A->inf = 1;                        // A == -T
    }
    return;
  }
  uint32_t* hh = z1z1;
  uint32_t* hhh = z2z2;
  uint32_t* v = u2;
  f384_sqr<P384>(hh, h);                 // 16 [2p]
  f384_mul<P384>(hhh, h, hh);            // 8 [2p]
  f384_mul<P384>(v, u1, hh);             // 4 [2p]
  f384_sqr<P384>(t, r);                  // 16 [2p]
  f384_muls<2>(u1, v);                   // [4p]
  f384_add(u1, u1, hhh);                 // HHH + 2V [6p]
  f384_sub<P384, 6>(A->x, t, u1);        // X3 [8p]
  f384_sub<P384, 8>(t, v, A->x);         // V + 8p - X3 [10p]
  f384_mul<P384>(t, r, t);               // 40 [2p]
  f384_mul<P384>(v, s1, hhh);            // 4 [2p]
  f384_sub<P384, 2>(A->y, t, v);         // Y3 [4p]
  f384_copy(A->z, z3);                   // Z3 = Z1 Z2 H [2p]
}

// Affine Montgomery coordinates (canonical) of a finite point.
BH_HD void j384_to_affine(uint32_t x[14], uint32_t y[14], const J384* A) {
  uint32_t z[14], zi[14], zi2[14], t[14];
  f384_canon<P384>(z, A->z);             // [p]
  f384_inv<P384>(zi, z);                 // [2p]
  f384_sqr<P384>(zi2, zi);               // [2p]
  f384_mul<P384>(t, A->x, zi2);          // 40 [2p]
  f384_canon<P384>(x, t);
  f384_mul<P384>(t, zi, zi2);            // [2p]
  f384_mul<P384>(t, A->y, t);            // 40 [2p]
  f384_canon<P384>(y, t);
}

// x(A) = v as field elements, v in Montgomery form (< 2p): X = v Z^2.
BH_HD bool j384_x_equals(const J384* A, const uint32_t v[14]) {
  uint32_t zz[14], t[14];
  f384_sqr<P384>(zz, A->z);              // 400 [3p]
  f384_mul<P384>(t, v, zz);              // 6 [2p]
  f384_sub<P384, 2>(t, A->x, t);         // X + 2p - v Z^2 [22p]
  return f384_is_zero<P384>(t);
}

}  // namespace bh
