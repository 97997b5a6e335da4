// TEST-ONLY: the host harness (tests/native/hostsim.cpp, included whole: its
// run_seq is this file's too) plus the entries for BDLS records whose
// SignedProto.Hash() the caller supplies (bh_verify_bdls_prehashed_dev).
// libhostsim.so is built from this translation unit.
#include "../native/hostsim.cpp"

// As hs_verify_bdls, with msg taken as SignedProto.Hash() itself: run_seq's
// digest stage (verify.h stage_bdls_hash) then runs stage_bdls_given, the
// function k_bdls_given runs on the device, so the digest -- hence e, u1, u2 --
// is the caller's; ver is not read. hs_set_wide / hs_set_ll / hs_set_reg apply.
extern "C" int hs_verify_bdls_prehashed(int curve, const uint8_t* xy, const uint8_t* r,
                                        const uint64_t* roff, const uint32_t* rlen,
                                        const uint8_t* s, const uint64_t* soff,
                                        const uint32_t* slen, const uint32_t* ver,
                                        const uint8_t* msg, const uint64_t* moff,
                                        const uint32_t* mlen, uint32_t n, uint32_t min_uses,
                                        uint8_t* reason) {
  BdlsIn in{xy, r, roff, rlen, s, soff, slen, ver, msg, moff, mlen, BHF_BDLS_PREHASHED};
  if (curve == 0) return run_seq<F30_p256, Fn_p256, Cv_p256>(in, n, 4, min_uses, reason, nullptr);
  return run_seq<F30_k1, Fn_k1, Cv_k1>(in, n, 4, min_uses, reason, nullptr);
}

// stage_bdls_given alone: e (8 little-endian u32 limbs) of the digest bytes
// dg[0, len) (tests place dg at every byte alignment)
extern "C" void hs_bdls_given_e(int curve, const uint8_t* dg, uint32_t len, uint32_t* e) {
  alignas(16) uint32_t buf[8 * 64] = {0};
  Work w{};
  w.ns = 64;
  w.e = buf;
  const uint64_t off = 0;
  BdlsIn in{};
  in.msg = dg;
  in.msg_off = &off;
  in.msg_len = &len;
  in.flags = BHF_BDLS_PREHASHED;
  if (curve == 0) stage_bdls_given<Cv_p256>(in, w, 0);
  else stage_bdls_given<Cv_k1>(in, w, 0);
  ld8(e, w.e, 0, w.ns);
}
