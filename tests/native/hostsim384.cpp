// TEST-ONLY host build of the P-384 device arithmetic: the BH_HD functions of
// bdls_amd/csrc/{fp384,ec384,verify384}.h compiled as plain C++, so the CPU
// suite checks the code the gfx950 kernels run. Never linked into the product.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../bdls_amd/csrc/verify384.h"

using namespace bh;

namespace {

std::vector<uint32_t> g_gtab;
std::once_flag g_gtab_once;

void par_for(uint32_t n, const std::function<void(uint32_t)>& fn) {
  const uint32_t nt = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      for (uint32_t i = t; i < n; i += nt) fn(i);
    });
  for (auto& x : th) x.join();
}

const uint32_t* gtab() {
  std::call_once(g_gtab_once, [] {
    g_gtab.assign(kGTab384Words, 0);
    par_for(kG384Win * kG384Ent, [](uint32_t t) { gtab384_entry(t, g_gtab.data()); });
  });
  return g_gtab.data();
}

struct WorkMem {
  std::vector<uint32_t> words;
  std::vector<uint8_t> st;
  Work384 w;
  explicit WorkMem(uint32_t n) {
    const uint32_t ns = (n + 63) & ~63u;
    words.assign((size_t)kWork384Words * std::max(ns, 64u), 0);
    st.assign(std::max(ns, 64u), 0);
    uint32_t* p = words.data();
    auto take = [&](size_t per) {
      uint32_t* q = p;
      p += per * std::max(ns, 64u);
      return q;
    };
    w.ns = std::max(ns, 64u);
    w.e = take(12);
    w.r = take(12);
    w.sm = take(14);
    w.pre = take(14);
    w.qx = take(14);
    w.qy = take(14);
    w.rm = take(14);
    w.r2m = take(14);
    w.qtab = take(8 * 3 * 14);
    w.st = st.data();
  }
};

template <class M>
int field_op(int op, int k, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  switch (op) {
    case 0: f384_mul<M>(out, a, b); return 0;
    case 1: f384_sqr<M>(out, a); return 0;
    case 2: f384_add(out, a, b); return 0;
    case 3:
      switch (k) {
        case 2: f384_sub<M, 2>(out, a, b); return 0;
        case 3: f384_sub<M, 3>(out, a, b); return 0;
        case 6: f384_sub<M, 6>(out, a, b); return 0;
        case 8: f384_sub<M, 8>(out, a, b); return 0;
        case 9: f384_sub<M, 9>(out, a, b); return 0;
        case 16: f384_sub<M, 16>(out, a, b); return 0;
        case 18: f384_sub<M, 18>(out, a, b); return 0;
        case 20: f384_sub<M, 20>(out, a, b); return 0;
        case 32: f384_sub<M, 32>(out, a, b); return 0;
      }
      return -1;
    case 4:
      switch (k) {
        case 2: f384_muls<2>(out, a); return 0;
        case 3: f384_muls<3>(out, a); return 0;
        case 4: f384_muls<4>(out, a); return 0;
        case 8: f384_muls<8>(out, a); return 0;
      }
      return -1;
    case 5: f384_canon<M>(out, a); return 0;
    case 6: f384_from_mont<M>(out, a); return 0;
    case 7: f384_to_mont<M>(out, a); return 0;
    case 8: out[0] = f384_is_zero<M>(a) ? 1 : 0; return 0;
    case 9: out[0] = f384_is_zero_small<M, 3>(a) ? 1 : 0; return 0;
    case 10: f384_cond_sub<M>(out, a); return 0;
    case 11: f384_inv<M>(out, a); return 0;
  }
  return -1;
}

}  // namespace

extern "C" {

// field 0: mod p, 1: mod n. a, b, out: 14 limbs of 28 bits. See field_op.
int hs384_field(int field, int op, int k, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  return field == 0 ? field_op<Fp_p384>(op, k, a, b, out) : field_op<Fn_p384>(op, k, a, b, out);
}

// 12-word integers <-> 14 limbs
void hs384_from_w12(const uint32_t* w, uint32_t* out) { f384_from_w12(out, w); }
void hs384_to_w12(const uint32_t* a, uint32_t* out) { f384_to_w12(out, a); }

// stage384_inv alone: record i has e, r, s (12 words each, < n); valid[i] = 0
// makes it contribute 1 as a rejected record does. chunk = records per lane.
void hs384_inv(const uint32_t* e, const uint32_t* r, const uint32_t* s, const uint8_t* valid,
               uint32_t n, uint32_t chunk, uint32_t* u1, uint32_t* u2) {
  WorkMem m(n);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t sm[14];
    if (valid[i]) {
      f384_from_w12(sm, s + 12 * i);
      f384_to_mont<N384>(sm, sm);
    } else {
      f384_const(sm, N384::r1);
    }
    stw<12>(m.w.e, i, m.w.ns, e + 12 * i);
    stw<12>(m.w.r, i, m.w.ns, r + 12 * i);
    stw<14>(m.w.sm, i, m.w.ns, sm);
  }
  const uint32_t stride = (n + chunk - 1) / chunk;
  for (uint32_t c = 0; c < stride; c++) stage384_inv(m.w, c, stride, n);
  for (uint32_t i = 0; i < n; i++) {
    ldw<12>(u1 + 12 * i, m.w.e, i, m.w.ns);
    ldw<12>(u2 + 12 * i, m.w.r, i, m.w.ns);
  }
}

// d 16^win G from the fixed-base table: affine x || y, plain big-endian-free
// 12-word integers (x then y).
void hs384_gtab_entry(uint32_t win, uint32_t d, uint32_t* xy) {
  const uint32_t* g = gtab() + ((size_t)win * kG384Ent + d - 1) * kG384Words;
  uint32_t t[14];
  f384_from_mont<P384>(t, g);
  f384_to_w12(xy, t);
  f384_from_mont<P384>(t, g + 14);
  f384_to_w12(xy + 12, t);
}

// The whole pass on the host: the stages in kernel order. flags: BH_F_*.
void hs384_verify(const uint8_t* pub, const uint8_t* sig, const uint64_t* so, const uint32_t* sl,
                  const uint8_t* msg, const uint64_t* mo, const uint32_t* ml, uint32_t n,
                  uint32_t flags, uint32_t chunk, uint8_t* reason) {
  if (!n) return;
  WorkMem m(n);
  const In384 in{pub, sig, so, sl, msg, mo, ml, flags};
  const uint32_t* gt = gtab();
  par_for(n, [&](uint32_t i) { stage384_prep(in, m.w, i); });
  const uint32_t stride = (n + chunk - 1) / chunk;
  par_for(stride, [&](uint32_t c) { stage384_inv(m.w, c, stride, n); });
  par_for(n, [&](uint32_t i) {
    const uint8_t st = m.w.st[i] & 0x7fu;
    reason[i] = st != R_OK ? st : (stage384_ladder(m.w, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH);
  });
}

// The point operations alone: A = a G and T = t G (12-word scalars, 0 = the
// point at infinity), each built by its own double-and-add chain so that equal
// points come with different Z; then A + T (mode 0), A - T (1), A + affine(T)
// (2), A - affine(T) (3; modes 2 and 3 need t != 0) or 2A (4). Returns 1 and
// leaves xy alone when the result is the point at infinity, else 0 with the
// affine x || y as plain 12-word integers.
static void scalar_g(J384* out, const uint32_t k[12]) {
  uint32_t gx[14], gy[14];
  f384_const(gx, Cv_p384::gx_m);
  f384_const(gy, Cv_p384::gy_m);
  J384 B;
  j384_set_affine(&B, gx, gy);
  j384_dbl(&B);
  j384_madd(&B, gx, gy, 1);  // G again, now with Z != 1
  out->inf = 1;
  for (int bit = 383; bit >= 0; bit--) {
    j384_dbl(out);
    if ((k[bit >> 5] >> (bit & 31)) & 1u) j384_add(out, &B, 0);
  }
}

int hs384_point_sum(const uint32_t* a, const uint32_t* t, int mode, uint32_t* xy) {
  J384 A, T;
  scalar_g(&A, a);
  scalar_g(&T, t);
  if (mode == 0 || mode == 1) {
    j384_add(&A, &T, (uint32_t)mode);
  } else if (mode == 2 || mode == 3) {
    uint32_t tx[14], ty[14];
    j384_to_affine(tx, ty, &T);
    j384_madd(&A, tx, ty, (uint32_t)(mode - 2));
  } else {
    j384_dbl(&A);
  }
  if (A.inf) return 1;
  uint32_t x[14], y[14], v[14];
  j384_to_affine(x, y, &A);
  f384_from_mont<P384>(v, x);
  f384_to_w12(xy, v);
  f384_from_mont<P384>(v, y);
  f384_to_w12(xy + 12, v);
  return 0;
}

// der.h's 12-word instantiation: returns the reason; r, s as 12 words.
int hs384_parse_der(const uint8_t* der, uint32_t len, uint32_t* r, uint32_t* s, uint32_t* big) {
  DerSigT<12> ds;
  std::memset(&ds, 0, sizeof(ds));
  const uint8_t rc = der_parse_sig(der, len, &ds);
  std::memcpy(r, ds.r, 48);
  std::memcpy(s, ds.s, 48);
  big[0] = ds.r_big;
  big[1] = ds.s_big;
  return rc;
}

}  // extern "C"
