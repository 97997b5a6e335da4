// TEST-ONLY: the P-384 host harness (tests/native/hostsim384.cpp, included
// whole) plus the pass over two-span records: record i's message is
// msg[mo, +ml) || msg[mo2, +ml2), hashed by stage384_prep in the fused modes.
// libhostsim384s.so is built from this translation unit.
#include "../native/hostsim384.cpp"

extern "C" {

// hs384_verify with the second-span arrays (both null: one span).
void hs384s_verify(const uint8_t* pub, const uint8_t* sig, const uint64_t* so, const uint32_t* sl,
                   const uint8_t* msg, const uint64_t* mo, const uint32_t* ml,
                   const uint64_t* mo2, const uint32_t* ml2, uint32_t n, uint32_t flags,
                   uint32_t chunk, uint8_t* reason) {
  if (!n) return;
  WorkMem m(n);
  const In384 in{pub, sig, so, sl, msg, mo, ml, flags, mo2, ml2};
  const uint32_t* gt = gtab();
  par_for(n, [&](uint32_t i) { stage384_prep(in, m.w, i); });
  const uint32_t stride = (n + chunk - 1) / chunk;
  par_for(stride, [&](uint32_t c) { stage384_inv(m.w, c, stride, n); });
  par_for(n, [&](uint32_t i) {
    const uint8_t st = m.w.st[i] & 0x7fu;
    reason[i] = st != R_OK ? st : (stage384_ladder(m.w, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH);
  });
}

}  // extern "C"
