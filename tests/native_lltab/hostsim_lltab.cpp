// Test-only host build of the per-batch comb table build (verify.h
// lltab_build: sign-paired entries) and of ec30.h j_dbl, for
// tests/test_lltab_cpu.py and lltab_selftest.cpp. Never linked into the product.
// curve 0 = P-256, 1 = secp256k1.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../bdls_amd/csrc/verify.h"

using namespace bh;

// the comb's shape as built: teeth | spacing << 8 | low-group digits a << 16
extern "C" uint32_t hl_shape() {
  return (uint32_t)kLLTeeth | ((uint32_t)kLLSpace << 8) | ((uint32_t)kLLA << 16);
}
// words a table build touches (entries + scratch); words per table slot
extern "C" uint32_t hl_scratch_words() { return kLLScr; }
extern "C" uint32_t hl_slot_words() { return kKTabWords; }

namespace {

// value a R (any beta f_mul takes) -> the canonical integer a, 9 limbs
template <class P>
void plain(uint32_t r[9], const uint32_t a[9]) {
  const uint32_t one[9] = {1u, 0, 0, 0, 0, 0, 0, 0, 0};
  f_mul<P>(r, a, one);
  f_canon<P>(r, r);
}

// One table for the key (qx, qy) (canonical Montgomery limbs) built into
// `tab` (kLLScr words are enough when scr is null; entries only when the
// scratch is separate).
template <class P>
void build(uint32_t* tab, uint32_t* scr, const uint32_t* qx, const uint32_t* qy) {
  std::vector<uint32_t> q(2 * 9 * 64, 0u);  // [9][ns = 64] x 2, record 5
  Work w{};
  w.ns = 64;
  w.qx = q.data();
  w.qy = q.data() + 9 * 64;
  st9(w.qx, 5, w.ns, qx);
  st9(w.qy, 5, w.ns, qy);
  lltab_build<P>(tab, w, 5, scr);
}

}  // namespace

// raw: the kLLEnt entries as the comb reads them (kLLAff words each: x then y,
// Montgomery domain, lazy); canon: 18 words per entry, the canonical integers
// x, y. tab has room for exactly `words` words: hl_scratch_words() with the
// scratch in the slot (sep == 0), kLLEnt * kLLAff with a separate scratch of
// exactly hl_scratch_words().
extern "C" int hl_lltab(int curve, const uint32_t* qx, const uint32_t* qy, int sep, uint32_t* tab,
                        uint32_t words, uint32_t* canon) {
  if (words != (sep ? kLLEnt * kLLAff : kLLScr)) return -1;
  std::vector<uint32_t> scr(sep ? kLLScr : 0u);
  if (curve == 0) build<F30_p256>(tab, sep ? scr.data() : nullptr, qx, qy);
  else build<F30_k1>(tab, sep ? scr.data() : nullptr, qx, qy);
  for (uint32_t m = 0; m < kLLEnt; m++) {
    uint32_t x[9], y[9];
    llaff_load(x, y, tab, m);
    if (curve == 0) {
      plain<F30_p256>(canon + 18 * m, x);
      plain<F30_p256>(canon + 18 * m + 9, y);
    } else {
      plain<F30_k1>(canon + 18 * m, x);
      plain<F30_k1>(canon + 18 * m + 9, y);
    }
  }
  return 0;
}

// r = 2 p (Jacobian, 27 words X Y Z each); in_place: r aliases p
extern "C" void hl_j_dbl(int curve, const uint32_t* pxyz, int in_place, uint32_t* rxyz) {
  J30 p, r;
  f_copy(p.X, pxyz);
  f_copy(p.Y, pxyz + 9);
  f_copy(p.Z, pxyz + 18);
  J30& out = in_place ? p : r;
  if (curve == 0) j_dbl<F30_p256>(out, p);
  else j_dbl<F30_k1>(out, p);
  f_copy(rxyz, out.X);
  f_copy(rxyz + 9, out.Y);
  f_copy(rxyz + 18, out.Z);
}
