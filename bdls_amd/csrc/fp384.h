// 384-bit Montgomery arithmetic in radix 2^28 for P-384: the base field
// (M = Fp_p384, p = 2^384 - 2^128 - 2^96 + 2^32 - 1) and the scalar field
// (M = Fn_p384, the group order n). fp30.h (256-bit fields) is untouched.
//
// VALUE CONTRACT
//   * An element is 14 limbs, every limb < 2^28 ("normalised"), value
//     < R = 2^392. R / m is only ~2^8, so an element is at most ~256 m.
//     Bounds are written as multiples of the modulus: "a < 20m".
//   * f384_mul(a, b): Montgomery product a b R^-1 mod m. Needs a < alpha m,
//     b < beta m with alpha beta <= 2^15 (kMulMaxAB); returns a normalised
//     value < (alpha beta / 256 + 1) m. Proof: the result is (a b + q m) / R
//     with q < R, so it is < a b / R + m, and a b / R < alpha beta m^2 / R
//     < alpha beta m / 256 because m < 2^384. With alpha beta <= 2^15 that
//     is < 129 m < R, so the 14 limbs hold it.
//   * Columns: the product is accumulated per column in 64 bits, one
//     multiply-add per term and no carry flag. A column receives at most 14
//     terms a_i b_j and 14 terms q_i m_j, each < 2^56, plus one carry
//     < 2^36: < 2^61. (13 limbs of 30 bits would not fit: 26 terms of 2^60.)
//   * p = -1 mod 2^28, so the base field's Montgomery factor n0 is 1 and the
//     quotient digit is the low limb itself; n needs the generic n0.
//   * f384_add: a + b, no reduction; needs a + b < R.
//   * f384_sub<M, K>(a, b): a + K m - b; needs b <= K m and a + K m < R
//     (K <= 32, the table M::km). Bounds add: a < alpha m gives < (alpha + K) m.
//   * f384_muls<k>(a): k a for a small constant k; needs k a < R.
//   * f384_canon: the value mod m in [0, m) for any element (one product by
//     R mod m, then one conditional subtraction).
//   * f384_is_zero_small<M, K>(a): a = 0 mod m for a < K m, by comparing with
//     0, m, .., (K-1) m. f384_is_zero: any element (one product).
// Every function is BH_HD: the kernels (verify384_kernels.hip) and the
// test-only host harness (tests/native/hostsim384.cpp) run the same code.
#pragma once
#include "bh_common.h"
#include "curve_consts384.h"

namespace bh {

constexpr uint32_t kMask28 = (1u << 28) - 1u;
constexpr uint32_t kMulMaxAB = 1u << 15;  // largest alpha * beta f384_mul accepts

BH_HD void f384_copy(uint32_t r[14], const uint32_t a[14]) {
#pragma unroll
  for (int i = 0; i < 14; i++) r[i] = a[i];
}

template <class C>
BH_HD void f384_const(uint32_t r[14], const C& c) {
#pragma unroll
  for (int i = 0; i < 14; i++) r[i] = c[i];
}

BH_HD bool f384_eq(const uint32_t a[14], const uint32_t b[14]) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) x |= a[i] ^ b[i];
  return x == 0;
}

// a b R^-1 mod m (see the contract above).
template <class M>
BH_HD void f384_mul(uint32_t r[14], const uint32_t a[14], const uint32_t b[14]) {
  uint64_t t[14];
#pragma unroll
  for (int j = 0; j < 14; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
#pragma unroll
    for (int j = 0; j < 14; j++) t[j] += (uint64_t)a[i] * b[j];
    const uint32_t q = ((uint32_t)t[0] * M::n0) & kMask28;
#pragma unroll
    for (int j = 0; j < 14; j++) t[j] += (uint64_t)q * M::m[j];
    // the low 28 bits of column 0 are zero now: shift the window one limb down
    const uint64_t c = t[0] >> 28;
#pragma unroll
    for (int j = 0; j < 13; j++) t[j] = t[j + 1];
    t[0] += c;
    t[13] = 0;
  }
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 14; j++) {
    c += t[j];
    r[j] = (uint32_t)c & kMask28;
    c >>= 28;
  }
}

template <class M>
BH_HD void f384_sqr(uint32_t r[14], const uint32_t a[14]) {
  f384_mul<M>(r, a, a);
}

// a + b (no reduction); a + b < R.
BH_HD void f384_add(uint32_t r[14], const uint32_t a[14], const uint32_t b[14]) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    c += a[i] + b[i];
    r[i] = c & kMask28;
    c >>= 28;
  }
}

// a + K m - b; b <= K m, a + K m < R.
template <class M, int K>
BH_HD void f384_sub(uint32_t r[14], const uint32_t a[14], const uint32_t b[14]) {
  static_assert(K >= 1 && K <= 32, "K");
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    c += (int32_t)(a[i] + M::km[K][i]) - (int32_t)b[i];
    r[i] = (uint32_t)c & kMask28;
    c >>= 28;  // arithmetic: the borrow travels as -1
  }
}

// k a for a small constant k; k a < R.
template <int K>
BH_HD void f384_muls(uint32_t r[14], const uint32_t a[14]) {
  static_assert(K >= 2 && K <= 8, "K");
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    c += a[i] * (uint32_t)K;
    r[i] = c & kMask28;
    c >>= 28;
  }
}

// a >= b as integers (both normalised).
BH_HD bool f384_geq(const uint32_t a[14], const uint32_t b[14]) {
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    c += (int32_t)a[i] - (int32_t)b[i];
    c >>= 28;
  }
  return c >= 0;
}

// a < 2m -> a mod m.
template <class M>
BH_HD void f384_cond_sub(uint32_t r[14], const uint32_t a[14]) {
  uint32_t d[14];
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    c += (int32_t)a[i] - (int32_t)M::m[i];
    d[i] = (uint32_t)c & kMask28;
    c >>= 28;
  }
#pragma unroll
  for (int i = 0; i < 14; i++) r[i] = c < 0 ? a[i] : d[i];
}

// The value mod m, in [0, m), for any element.
template <class M>
BH_HD void f384_canon(uint32_t r[14], const uint32_t a[14]) {
  uint32_t one_m[14], t[14];
  f384_const(one_m, M::r1);
  f384_mul<M>(t, a, one_m);  // a R R^-1; a < R and r1 < m: t < 2m
  f384_cond_sub<M>(r, t);
}

// Plain value -> Montgomery form (a < 2^384 + ..., any element): a R mod m, < 2m.
template <class M>
BH_HD void f384_to_mont(uint32_t r[14], const uint32_t a[14]) {
  uint32_t r2[14];
  f384_const(r2, M::r2);
  f384_mul<M>(r, a, r2);  // callers pass a < 2m: < 2m
}

// Montgomery form -> the plain value in [0, m), for any element.
template <class M>
BH_HD void f384_from_mont(uint32_t r[14], const uint32_t a[14]) {
  uint32_t one[14], t[14];
#pragma unroll
  for (int i = 0; i < 14; i++) one[i] = 0;
  one[0] = 1;
  f384_mul<M>(t, a, one);  // a / R + m: <= m
  f384_cond_sub<M>(r, t);
}

// a = 0 mod m, for a < K m.
template <class M, int K>
BH_HD bool f384_is_zero_small(const uint32_t a[14]) {
  static_assert(K >= 1 && K <= 32, "K");
  bool z = false;
#pragma unroll
  for (int k = 0; k < K; k++) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) x |= a[i] ^ M::km[k][i];
    z |= (x == 0);
  }
  return z;
}

// a = 0 mod m, any element.
template <class M>
BH_HD bool f384_is_zero(const uint32_t a[14]) {
  uint32_t t[14];
  f384_from_mont<M>(t, a);  // zero-ness survives the factor R^-1
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) x |= t[i];
  return x == 0;
}

// a^e (Montgomery form in and out, a < 2m -> < 2m), e a public 384-bit
// exponent as 12 words with its top bit set (m - 2).
template <class M, class E>
BH_HD void f384_pow(uint32_t r[14], const uint32_t a[14], const E& e) {
  uint32_t acc[14];
  f384_copy(acc, a);  // bit 383 of the exponent is 1
#pragma unroll 1
  for (int bit = 382; bit >= 0; bit--) {
    f384_sqr<M>(acc, acc);
    uint32_t t[14];
    f384_mul<M>(t, acc, a);
    const bool set = (e[bit >> 5] >> (bit & 31)) & 1u;
#pragma unroll
    for (int i = 0; i < 14; i++) acc[i] = set ? t[i] : acc[i];
  }
  f384_copy(r, acc);
}

// a^-1 by Fermat (Montgomery form; a != 0 mod m).
template <class M>
BH_HD void f384_inv(uint32_t r[14], const uint32_t a[14]) {
  f384_pow<M>(r, a, M::mm2);
}

// ---- 12 x 32-bit words (plain integers < 2^384) ----
BH_HD void w12_from_be48(uint32_t r[12], const uint8_t* b) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint8_t* q = b + 44 - 4 * i;
    r[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}

BH_HD bool w12_geq(const uint32_t a[12], const uint32_t b[12]) {
  uint32_t bo = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - bo;
    bo = (uint32_t)(d >> 63);
  }
  return bo == 0;
}

// r = a - b, returns the borrow
BH_HD uint32_t w12_sub(uint32_t r[12], const uint32_t a[12], const uint32_t b[12]) {
  uint32_t bo = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - bo;
    r[i] = (uint32_t)d;
    bo = (uint32_t)(d >> 63);
  }
  return bo;
}

// r = a + b, returns the carry
BH_HD uint32_t w12_add(uint32_t r[12], const uint32_t a[12], const uint32_t b[12]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    c += (uint64_t)a[i] + b[i];
    r[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}

template <class C>
BH_HD void w12_const(uint32_t r[12], const C& c) {
#pragma unroll
  for (int i = 0; i < 12; i++) r[i] = c[i];
}

// 384-bit integer -> 14 limbs of 28 bits (the top two limbs hold 20 bits)
BH_HD void f384_from_w12(uint32_t r[14], const uint32_t w[12]) {
#pragma unroll
  for (int i = 0; i < 14; i++) {
    const int bit = 28 * i, k = bit >> 5, sh = bit & 31;
    uint64_t v = w[k];
    if (k + 1 < 12) v |= (uint64_t)w[k + 1] << 32;
    r[i] = (uint32_t)(v >> sh) & kMask28;
  }
}

// 14 normalised limbs with value < 2^384 -> 12 words
BH_HD void f384_to_w12(uint32_t w[12], const uint32_t a[14]) {
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const int bit = 32 * k, i = bit / 28, sh = bit % 28;
    uint64_t v = a[i];
    if (i + 1 < 14) v |= (uint64_t)a[i + 1] << 28;
    if (i + 2 < 14) v |= (uint64_t)a[i + 2] << 56;
    w[k] = (uint32_t)(v >> sh);
  }
}

}  // namespace bh
