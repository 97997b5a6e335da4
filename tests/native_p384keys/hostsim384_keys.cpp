// TEST-ONLY: the P-384 host harness (tests/native/hostsim384.cpp, included
// whole: its gtab, par_for and WorkMem are this file's too) plus the entries
// for the key registry of bdls_amd/csrc/keys384.h: the table build, the hash
// table, and a pass whose records take the table route where their key is
// registered. libhostsim384k.so is built from this translation unit.
#include "../native/hostsim384.cpp"

#include "../../bdls_amd/csrc/keys384.h"

namespace {

struct HostReg {
  std::vector<uint32_t> bucket, keys, tables, count;
  KeyReg384 g{};
  void alloc(uint32_t cap) {
    uint32_t hc = 1;
    while (hc < 2 * cap) hc <<= 1;
    bucket.assign(hc, 0);
    keys.assign((size_t)cap * 24, 0);
    tables.assign((size_t)cap * kKTab384Words, 0);
    count.assign(1, 0);
    g = KeyReg384{cap, hc, bucket.data(), keys.data(), tables.data(), count.data()};
  }
};
HostReg g_reg;

// keytab384_bases + keytab384_window for the key in slot `slot`, as the two build kernels do.
void build_table(const KeyReg384& g, uint32_t slot) {
  std::vector<uint32_t> bases((size_t)kG384Win * kBase384Words);
  keytab384_bases(g, slot, bases.data());
  par_for(kG384Win, [&](uint32_t w) {
    keytab384_window(bases.data() + (size_t)w * kBase384Words,
                     g.tables + (size_t)slot * kKTab384Words + (size_t)w * kG384Ent * kG384Words);
  });
}

}  // namespace

extern "C" {

// (Re)allocate the harness registry, empty.
void hs384k_reserve(uint32_t cap) { g_reg.alloc(cap); }
uint32_t hs384k_count() { return g_reg.count.empty() ? 0 : g_reg.count[0]; }
uint32_t hs384k_buckets() { return g_reg.g.hc; }
void hs384k_clear() {
  std::fill(g_reg.bucket.begin(), g_reg.bucket.end(), 0u);
  if (!g_reg.count.empty()) g_reg.count[0] = 0;
}

// bh_keys384_register's kernel sequence: verdicts, serial insert, tables of the fresh slots.
void hs384k_register(const uint8_t* pub, uint32_t n, uint8_t* status) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t qx[14], qy[14];
    status[i] = key_import384(pub + (size_t)i * 96, qx, qy) ? 0 : (uint8_t)R_BAD_KEY;
  }
  std::vector<uint32_t> fresh(n + 1);
  keys384_insert(g_reg.g, pub, n, status, fresh.data(), &fresh[n]);
  for (uint32_t k = 0; k < fresh[n]; k++) build_table(g_reg.g, fresh[k]);
}

// The slot of a key, or -1.
int hs384k_find(const uint8_t* pub) {
  uint32_t k[24];
  key384_words(pub, k);
  const uint32_t s = keys384_find(g_reg.g, k);
  return s == kNoSlot384 ? -1 : (int)s;
}

uint32_t hs384k_hash(const uint8_t* pub) {
  uint32_t k[24];
  key384_words(pub, k);
  return key384_hash(k);
}

// The table of slot `slot` as stored (Montgomery rows), and the table of G.
void hs384k_table_raw(uint32_t slot, uint32_t* out) {
  std::memcpy(out, g_reg.g.tables + (size_t)slot * kKTab384Words, kKTab384Words * 4);
}
void hs384k_gtab_raw(uint32_t* out) { std::memcpy(out, gtab(), kGTab384Words * 4); }

// Entry d (1..15) of window win of slot's table: affine x || y as plain 12-word integers.
void hs384k_entry(uint32_t slot, uint32_t win, uint32_t d, uint32_t* xy) {
  const uint32_t* row = g_reg.g.tables + (size_t)slot * kKTab384Words +
                        ((size_t)win * kG384Ent + d - 1) * kG384Words;
  uint32_t t[14];
  f384_from_mont<P384>(t, row);
  f384_to_w12(xy, t);
  f384_from_mont<P384>(t, row + 14);
  f384_to_w12(xy + 12, t);
}

// The pass with the harness registry: prep, inverse, plan, then stage384_keywin
// for the records whose key is registered and stage384_ladder for the rest.
// route[i] (optional) = 1 where record i took the table route.
void hs384k_verify(const uint8_t* pub, const uint8_t* sig, const uint64_t* so, const uint32_t* sl,
                   const uint8_t* msg, const uint64_t* mo, const uint32_t* ml, uint32_t n,
                   uint32_t flags, uint32_t chunk, uint8_t* reason, uint8_t* route) {
  if (!n) return;
  WorkMem m(n);
  const In384 in{pub, sig, so, sl, msg, mo, ml, flags};
  const uint32_t* gt = gtab();
  par_for(n, [&](uint32_t i) { stage384_prep(in, m.w, i); });
  const uint32_t stride = (n + chunk - 1) / chunk;
  par_for(stride, [&](uint32_t c) { stage384_inv(m.w, c, stride, n); });
  par_for(n, [&](uint32_t i) {
    const uint32_t slot = stage384_plan(in, m.w, g_reg.g, i);
    if (route) route[i] = slot != kNoSlot384;
    if (slot != kNoSlot384) {
      const uint32_t* qtab = g_reg.g.tables + (size_t)slot * kKTab384Words;
      reason[i] = stage384_keywin(m.w, qtab, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
      return;
    }
    const uint8_t st = m.w.st[i] & 0x7fu;
    reason[i] = st != R_OK ? st : (stage384_ladder(m.w, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH);
  });
}

}  // extern "C"
