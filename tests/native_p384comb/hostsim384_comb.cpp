// TEST-ONLY: the P-384 host harness (tests/native/hostsim384.cpp, included
// whole: its gtab, par_for and WorkMem are this file's too) plus the entries
// for the per-pass key combs of bdls_amd/csrc/comb384.h (BH_F_BATCH_KEYS): the
// grouping and routing of a pass, the comb build, and a whole flagged pass
// whose records take the registry, comb or ladder route. The grouping runs
// record after record (the kernels' compare-and-swap is a plain store here).
// libhostsim384c.so is built from this translation unit;
// comb384_selftest.cpp includes it for the sanitizer run.
#include "../native/hostsim384.cpp"

#include "../../bdls_amd/csrc/comb384.h"

namespace {

struct PlainCas {
  uint32_t operator()(uint32_t* p, uint32_t v) const {
    if (*p == 0) *p = v;
    return *p;
  }
};

// Comb384 in host memory for a pass of n records.
struct CombMem {
  std::vector<uint32_t> mem;
  Comb384 cb{};
  CombMem(uint32_t n, uint32_t min) {
    const uint32_t ns = std::max(64u, (n + 63) & ~63u);
    uint32_t hc = 128;
    while (hc < 2 * ns) hc <<= 1;
    const uint32_t cap = std::max(1u, ns / min);
    mem.assign(2 + (size_t)3 * hc + (size_t)2 * ns + cap +
                   (size_t)cap * (kComb384BaseWords + 2 * kComb384Words), 0);
    uint32_t* p = mem.data();
    auto take = [&](size_t words) {
      uint32_t* q = p;
      p += words;
      return q;
    };
    cb.hc = hc;
    cb.cap = cap;
    cb.min = min;
    cb.ctr = take(2);
    cb.rep = take(hc);
    cb.cnt = take(hc);
    cb.gslot = take(hc);
    cb.bkt = take(ns);
    cb.list = take(ns);
    cb.slot_rep = take(cap);
    cb.bases = take((size_t)cap * kComb384BaseWords);
    cb.side = take((size_t)cap * kComb384Words);
    cb.tables = take((size_t)cap * kComb384Words);
  }
};

// A registry of the given keys (tables built only if `tables`).
struct RegMem {
  std::vector<uint32_t> bucket, keys, tabs, count;
  KeyReg384 g{};
  RegMem(const uint8_t* pub, uint32_t n, bool tables) {
    if (!n) return;
    uint32_t hc = 1;
    while (hc < 2 * n) hc <<= 1;
    bucket.assign(hc, 0);
    keys.assign((size_t)n * 24, 0);
    tabs.assign(tables ? (size_t)n * kKTab384Words : 1, 0);
    count.assign(1, 0);
    g = KeyReg384{n, hc, bucket.data(), keys.data(), tabs.data(), count.data()};
    std::vector<uint8_t> status(n, 0);
    std::vector<uint32_t> fresh(n + 1);
    for (uint32_t i = 0; i < n; i++) {
      uint32_t qx[14], qy[14];
      status[i] = key_import384(pub + (size_t)i * 96, qx, qy) ? 0 : (uint8_t)R_BAD_KEY;
    }
    keys384_insert(g, pub, n, status.data(), fresh.data(), &fresh[n]);
    const uint32_t nfresh = fresh[n];
    if (!count[0]) g.cap = 0;  // nothing registered: no lookup
    if (!tables) return;
    for (uint32_t k = 0; k < nfresh; k++) {
      std::vector<uint32_t> bases((size_t)kG384Win * kBase384Words);
      keytab384_bases(g, fresh[k], bases.data());
      par_for(kG384Win, [&](uint32_t w) {
        keytab384_window(bases.data() + (size_t)w * kBase384Words,
                         g.tables + (size_t)fresh[k] * kKTab384Words +
                             (size_t)w * kG384Ent * kG384Words);
      });
    }
  }
};

// k384_comb_group, k384_comb_assign and k384_comb_plan, record after record.
// ok[i]: prep let record i through. route[i]: 0 ladder, 1 comb, 2 registry;
// slot[i]: the table's slot on the two table routes.
void plan_pass(const uint8_t* pub, const uint8_t* ok, uint32_t n, const KeyReg384& g, Comb384& cb,
               uint8_t* route, uint32_t* slot) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t b = kNoSlot384;
    if (ok[i]) {
      b = comb384_claim(pub, cb, i, PlainCas{});
      if (b != kNoSlot384) cb.cnt[b]++;
    }
    cb.bkt[i] = b;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t b = cb.bkt[i];
    if (b == kNoSlot384 || cb.rep[b] != i + 1) continue;
    uint32_t r = comb384_group_route(pub, g, cb, i, b);
    if (r == 0) {
      r = cb.ctr[0]++;
      if (r < cb.cap) cb.slot_rep[r] = i;
      else r = kNoSlot384;
    }
    cb.gslot[b] = r;
  }
  for (uint32_t i = 0; i < n; i++) {
    uint32_t s = kNoSlot384;
    route[i] = (uint8_t)comb384_record_route(cb, i, &s);
    slot[i] = s;
    if (route[i] == 1) cb.list[cb.ctr[1]++] = i;
  }
}

std::vector<uint32_t> g_gcomb;
std::once_flag g_gcomb_once;

const uint32_t* gcomb() {
  std::call_once(g_gcomb_once, [] {
    g_gcomb.assign(kComb384Words, 0);
    std::vector<uint32_t> bases(kComb384BaseWords), side(kComb384Words);
    uint32_t gx[14], gy[14];
    f384_const(gx, Cv_p384::gx_m);
    f384_const(gy, Cv_p384::gy_m);
    comb384_bases(gx, gy, bases.data());
    comb384_rows(bases.data(), side.data(), g_gcomb.data());
  });
  return g_gcomb.data();
}

}  // namespace

extern "C" {

uint32_t hs384c_hash(const uint8_t* pub) {
  uint32_t k[24];
  key384_words(pub, k);
  return key384_hash(k);
}

// Buckets of a pass of n records.
uint32_t hs384c_buckets(uint32_t n, uint32_t min) { return CombMem(n, min).cb.hc; }

// Group and route a pass of n records (ok[i]: prep let it through) against a
// registry of the nreg keys at reg_pub. Returns the number of comb slots handed
// out; route / slot per record as plan_pass gives them; rep[i] (optional) the
// record's group's representative, 0xffffffff without a group.
uint32_t hs384c_plan(const uint8_t* pub, const uint8_t* ok, uint32_t n, uint32_t min,
                     const uint8_t* reg_pub, uint32_t nreg, uint8_t* route, uint32_t* slot,
                     uint32_t* rep) {
  CombMem m(n, min);
  RegMem reg(reg_pub, nreg, false);
  plan_pass(pub, ok, n, reg.g, m.cb, route, slot);
  if (rep)
    for (uint32_t i = 0; i < n; i++)
      rep[i] = m.cb.bkt[i] == kNoSlot384 ? kNoSlot384 : m.cb.rep[m.cb.bkt[i]] - 1;
  return m.cb.ctr[0];
}

// The comb of the key at pub as stored: 63 rows of x || y, 14 limbs each,
// canonical Montgomery. Returns 0, or -1 if the key is not a point of the curve.
int hs384c_table_raw(const uint8_t* pub, uint32_t* out) {
  uint32_t qx[14], qy[14];
  if (!key_import384(pub, qx, qy)) return -1;
  std::vector<uint32_t> bases(kComb384BaseWords), side(kComb384Words);
  comb384_bases(qx, qy, bases.data());
  comb384_rows(bases.data(), side.data(), out);
  return 0;
}
void hs384c_gcomb_raw(uint32_t* out) { std::memcpy(out, gcomb(), kComb384Words * 4); }

// A whole flagged pass: per chunk of pass_chunk records (0: all at once) prep,
// inverse (inv_chunk records per lane), grouping and routing, the comb build,
// then the three routes. reason / route per record; returns the combs built,
// summed over the chunks.
uint32_t hs384c_verify(const uint8_t* pub, const uint8_t* sig, const uint64_t* so,
                       const uint32_t* sl, const uint8_t* msg, const uint64_t* mo,
                       const uint32_t* ml, uint32_t n, uint32_t flags, uint32_t pass_chunk,
                       uint32_t inv_chunk, uint32_t min, const uint8_t* reg_pub, uint32_t nreg,
                       uint8_t* reason, uint8_t* route) {
  if (!n) return 0;
  RegMem reg(reg_pub, nreg, true);
  const uint32_t* gt = gtab();
  const uint32_t* gc = gcomb();
  uint32_t tables = 0;
  if (!pass_chunk) pass_chunk = n;
  for (uint32_t base = 0; base < n; base += pass_chunk) {
    const uint32_t c = std::min(pass_chunk, n - base);
    WorkMem m(c);
    CombMem cm(c, min);
    const In384 in{pub + (size_t)base * 96, sig, so + base, sl + base, msg, mo + base, ml + base,
                   flags};
    par_for(c, [&](uint32_t i) { stage384_prep(in, m.w, i); });
    const uint32_t stride = (c + inv_chunk - 1) / inv_chunk;
    par_for(stride, [&](uint32_t l) { stage384_inv(m.w, l, stride, c); });
    std::vector<uint8_t> ok(c);
    std::vector<uint32_t> slot(c);
    for (uint32_t i = 0; i < c; i++) ok[i] = (m.w.st[i] & 0x7fu) == R_OK;
    plan_pass(in.pub, ok.data(), c, reg.g, cm.cb, route + base, slot.data());
    const uint32_t nt = std::min(cm.cb.ctr[0], cm.cb.cap);
    tables += nt;
    par_for(nt, [&](uint32_t t) {
      const uint32_t i = cm.cb.slot_rep[t];
      uint32_t qx[14], qy[14];
      ldw<14>(qx, m.w.qx, i, m.w.ns);
      ldw<14>(qy, m.w.qy, i, m.w.ns);
      comb384_bases(qx, qy, cm.cb.bases + (size_t)t * kComb384BaseWords);
      comb384_rows(cm.cb.bases + (size_t)t * kComb384BaseWords,
                   cm.cb.side + (size_t)t * kComb384Words, cm.cb.tables + (size_t)t * kComb384Words);
    });
    par_for(c, [&](uint32_t i) {
      uint8_t* out = reason + base + i;
      if (route[base + i] == 1) {
        const uint32_t* qtab = cm.cb.tables + (size_t)slot[i] * kComb384Words;
        *out = stage384_comb(m.w, qtab, gc, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
      } else if (route[base + i] == 2) {
        const uint32_t* qtab = reg.g.tables + (size_t)slot[i] * kKTab384Words;
        *out = stage384_keywin(m.w, qtab, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
      } else {
        const uint8_t st = m.w.st[i] & 0x7fu;
        *out = st != R_OK ? st : (stage384_ladder(m.w, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH);
      }
    });
  }
  return tables;
}

}  // extern "C"
