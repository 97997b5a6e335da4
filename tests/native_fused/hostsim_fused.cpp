// Test-only host build of the fused field / point formulas (fp30.h f_mul2,
// ec30.h j_madd / j_add / j_zaddc, verify.h ll_dbladd / j_dbladd) for
// tests/test_fused_cpu.py. Never linked into the product.
// curve 0 = P-256 (the fused forms), 1 = secp256k1 (two products; f_mul2 is
// P-256 only).
#include <cstddef>
#include <cstdint>

#include "../../bdls_amd/csrc/verify.h"

using namespace bh;

namespace {
void ld(J30& p, const uint32_t* xyz) {
  f_copy(p.X, xyz);
  f_copy(p.Y, xyz + 9);
  f_copy(p.Z, xyz + 18);
}
void st(uint32_t* xyz, const J30& p) {
  f_copy(xyz, p.X);
  f_copy(xyz + 9, p.Y);
  f_copy(xyz + 18, p.Z);
}
}  // namespace

extern "C" void hf_f_mul2(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                          const uint32_t* d, uint32_t* r) {
  f_mul2<F30_p256>(r, a, b, c, d);
}

extern "C" void hf_f_negk96(int curve, const uint32_t* a, uint32_t* r) {
  if (curve == 0) f_negk<F30_p256, 96>(r, a);
  else f_negk<F30_k1, 96>(r, a);
}

extern "C" void hf_f_dblsub(int curve, int K, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (curve == 0) {
    if (K == 32) f_dblsub<F30_p256, 32>(r, a, b);
    else f_dblsub<F30_p256, 64>(r, a, b);
  } else {
    if (K == 32) f_dblsub<F30_k1, 32>(r, a, b);
    else f_dblsub<F30_k1, 64>(r, a, b);
  }
}

// r = p + (x2, +-y2, 1); returns degenerate | same_y << 1. in_place: r aliases p.
extern "C" int hf_j_madd(int curve, const uint32_t* pxyz, const uint32_t* x2, const uint32_t* y2,
                         int neg, int in_place, uint32_t* rxyz) {
  J30 p, r;
  ld(p, pxyz);
  bool same = false, deg;
  J30& out = in_place ? p : r;
  if (curve == 0) deg = j_madd<F30_p256>(out, p, x2, y2, &same, neg != 0);
  else deg = j_madd<F30_k1>(out, p, x2, y2, &same, neg != 0);
  st(rxyz, out);
  return (int)deg | ((int)same << 1);
}

extern "C" int hf_j_add(int curve, const uint32_t* pxyz, const uint32_t* qxyz, int in_place,
                        uint32_t* rxyz) {
  J30 p, q, r;
  ld(p, pxyz);
  ld(q, qxyz);
  bool same = false, deg;
  J30& out = in_place ? p : r;
  if (curve == 0) deg = j_add<F30_p256>(out, p, q, &same);
  else deg = j_add<F30_k1>(out, p, q, &same);
  st(rxyz, out);
  return (int)deg | ((int)same << 1);
}

// the co-Z addition without the partner update, on its own inputs
extern "C" void hf_j_zaddc(int curve, const uint32_t* x1, const uint32_t* y1, const uint32_t* x2,
                           const uint32_t* dx, const uint32_t* sy, const uint32_t* z,
                           uint32_t* rxyz) {
  J30 r;
  if (curve == 0) j_zaddc<F30_p256>(r, x1, y1, x2, dx, sy, z);
  else j_zaddc<F30_k1>(r, x1, y1, x2, dx, sy, z);
  st(rxyz, r);
}

// A = 2 A + (tx, +-ty, 1) with the explicit degenerate cases (verify.h
// ll_dbladd); a_inf in and out. Returns the new a_inf.
extern "C" int hf_ll_dbladd(int curve, uint32_t* axyz, int a_inf, const uint32_t* tx,
                            const uint32_t* ty, int neg) {
  J30 A;
  ld(A, axyz);
  bool inf = a_inf != 0;
  uint32_t x[9], y[9], one[9];
  f_copy(x, tx);
  f_copy(y, ty);
  if (curve == 0) {
    f_const(one, F30_p256::r1);
    ll_dbladd<F30_p256>(A, inf, x, y, neg != 0, one);
  } else {
    f_const(one, F30_k1::r1);
    ll_dbladd<F30_k1>(A, inf, x, y, neg != 0, one);
  }
  st(axyz, A);
  return (int)inf;
}

// A = 2 A + (+-T) for a Jacobian T (verify.h j_dbladd; P-256's ladder)
extern "C" int hf_j_dbladd(uint32_t* axyz, int a_inf, const uint32_t* txyz, int neg) {
  J30 A, T;
  ld(A, axyz);
  ld(T, txyz);
  bool inf = a_inf != 0;
  j_dbladd<F30_p256>(A, inf, T, neg != 0);
  st(axyz, A);
  return (int)inf;
}
