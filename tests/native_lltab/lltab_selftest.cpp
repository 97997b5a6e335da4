// Stand-alone check of verify.h lltab_build's scratch layout on the CPU, built
// with -fsanitize=address,undefined: comb tables for a few keys on both curves,
// built (a) into a heap buffer of exactly kLLScr words (the scratch in the
// slot, as the per-batch build runs) and (b) into exactly kLLEnt * kLLAff
// words of entries with a separate scratch of exactly kLLScr words (k_reg_win's
// LDS scratch), so a read or write outside either is an AddressSanitizer
// error. Of each table the all-minus entry E[0] (the H - L' half of a pair)
// and the all-plus entry E[2^(t-1) - 1] (the H + L' half) are compared with a
// plain double-and-add of their scalars.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hostsim_lltab.cpp"

namespace {

template <class P>
void smul(uint32_t x[9], uint32_t y[9], const uint32_t k[8], const uint32_t qx[9],
          const uint32_t qy[9]) {  // canonical integers x, y of k (qx, qy); k != 0
  J30 A;
  bool inf = true, same = false;
  for (int b = 255; b >= 0; b--) {
    if (!inf) j_dbl<P>(A, A);
    if (!((k[b >> 5] >> (b & 31)) & 1u)) continue;
    if (inf) {
      f_copy(A.X, qx);
      f_copy(A.Y, qy);
      f_const(A.Z, P::r1);
      inf = false;
    } else if (j_madd<P>(A, A, qx, qy, &same)) {
      abort();  // never for these scalars
    }
  }
  uint32_t zi[9], ax[9], ay[9];
  f_inv<P>(zi, A.Z);
  ll_to_affine<P>(ax, ay, A, zi);
  plain<P>(x, ax);
  plain<P>(y, ay);
}

void set_bit(uint32_t k[8], int b) { k[b >> 5] |= 1u << (b & 31); }

// a - b over 8 words (a > b)
void sub8(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t bw = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a[i] - b[i] - bw;
    r[i] = (uint32_t)t;
    bw = (t >> 32) & 1u;
  }
}

template <class P>
int run(int curve, const char* name) {
  int bad = 0;
  uint32_t gx[9], gy[9];
  f_const(gx, P::gx_m);
  f_const(gy, P::gy_m);
  // the entry scalars: all digits +1, and +1 at the top tooth with -1 below
  uint32_t plus[8] = {0}, top[8] = {0}, low[8] = {0}, minus[8];
  for (int i = 0; i < kLLTeeth; i++) set_bit(plus, kLLSpace * i);
  set_bit(top, kLLSpace * (kLLTeeth - 1));
  for (int i = 0; i + 1 < kLLTeeth; i++) set_bit(low, kLLSpace * i);
  sub8(minus, top, low);
  const uint32_t mult[4][8] = {{1u}, {2u}, {0xdeadbeefu, 0x12345678u, 0x9abcdef0u, 7u},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x0fffffffu}};
  for (int kk = 0; kk < 4; kk++) {
    uint32_t px[9], py[9], qx[9], qy[9];
    smul<P>(px, py, mult[kk], gx, gy);  // plain integers -> canonical Montgomery limbs
    f_to_mont<P>(qx, px);
    f_canon<P>(qx, qx);
    f_to_mont<P>(qy, py);
    f_canon<P>(qy, qy);
    uint32_t want[2][18];
    smul<P>(want[0], want[0] + 9, minus, qx, qy);
    smul<P>(want[1], want[1] + 9, plus, qx, qy);
    for (int sep = 0; sep < 2; sep++) {
      const uint32_t words = sep ? kLLEnt * kLLAff : kLLScr;
      uint32_t* tab = (uint32_t*)malloc((size_t)words * 4);
      uint32_t* canon = (uint32_t*)malloc((size_t)kLLEnt * 18 * 4);
      if (!tab || !canon) abort();
      memset(tab, 0xa5, (size_t)words * 4);
      if (hl_lltab(curve, qx, qy, sep, tab, words, canon) != 0) abort();
      if (memcmp(canon, want[0], sizeof want[0]) ||
          memcmp(canon + 18 * (kLLEnt - 1u), want[1], sizeof want[1])) {
        fprintf(stderr, "%s key %d sep %d: entry mismatch\n", name, kk, sep);
        bad = 1;
      }
      free(tab);
      free(canon);
    }
  }
  return bad;
}

}  // namespace

int main() {
  const int bad = run<F30_p256>(0, "p256") | run<F30_k1>(1, "secp256k1");
  printf("lltab_selftest: %u scratch words, %s\n", kLLScr, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
