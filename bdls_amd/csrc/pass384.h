// One P-384 verify pass as the host launches it: the interface between
// bdls_hip.cpp (run_pass384) and verify384_kernels.hip (launch_pass384).
// Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include "comb384.h"

namespace bh {

// Everything a pass of n records reads and writes. Its route follows from it:
//   cb.tables != nullptr   a BH_F_BATCH_KEYS pass: records grouped by key, three routes
//   else reg.cap != 0      keys in the registry: table route and ladder
//   else                   the ladder over all n records
struct Pass384 {
  In384 in;
  Work384 w;
  Plan384 pl;
  KeyReg384 reg;      // cap == 0: no lookup, no registry route
  Comb384 cb;         // tables == nullptr: no comb
  size_t zero_bytes;  // comb: the bytes from cb.ctr on (ctr, rep, cnt) that the pass clears
  const uint32_t* gtab;
  const uint32_t* gcomb;  // comb only
  uint32_t n;
  uint64_t* bitmap;
  uint8_t* reason;
};

// The optional timing events of a pass, on s unless noted. A route records
// the ones it has: the ladder alone kStart, kPrep, kInv, kEnd; the registry
// route all but kBuild; the comb route all eight.
enum Ev384 {
  kEv384Start,   // before prep
  kEv384Prep,    // end of prep
  kEv384Inv,     // end of the inverse
  kEv384Plan,    // end of the grouping / plan: the routes start here
  kEv384Routes,  // end of the table routes (on aux)
  kEv384Ladder,  // end of the ladder list
  kEv384End,     // end of the bitmap: the pass is done
  kEv384Build,   // end of the comb build (on aux, before the table routes)
  kEv384Count
};

// s: the pass's stream; aux / fork / join: the table routes beside the ladder
// (unused by the ladder-alone route); ev: kEv384Count events or nullptr.
hipError_t launch_pass384(const Pass384& p, hipStream_t s, hipStream_t aux, hipEvent_t fork,
                          hipEvent_t join, hipEvent_t* ev);

}  // namespace bh
