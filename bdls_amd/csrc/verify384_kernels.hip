// HIP kernels (gfx950) of the P-384 verify pass (BH_CURVE_P384). The stage
// logic lives in verify384.h (shared with the test-only host harness); this
// file only maps lanes to records. A translation unit of its own:
// verify_kernels.hip and the code generated from it do not change.
//
//   k384_gtab    1 lane/entry    fixed-base table of G, once per device
//   k384_prep    1 lane/record   parse + checks + digest + Montgomery inputs
//   k384_inv     1 lane/chunk    s^-1 by Montgomery's trick, u1, u2
//   k384_ladder  1 lane/record   u2 Q (signed window) + u1 G (table), x check
//   k384_bitmap  1 lane/record   validity bitmap from the reason bytes
//
// With keys in the registry (bh_keys384_*, keys384.h) a pass routes its records:
//   k384_plan         1 lane/record   registry lookup, the two index lists
//   k384_keywin       1 lane/record   table route: u2 Q and u1 G from tables
//   k384_ladder_list  1 lane/record   k384_ladder over the other list
// and bh_keys384_register runs
//   k384_keys_import  1 lane/key      key_import384's verdict
//   k384_keys_insert  1 lane          the registry's one writer
//   k384_keytab_bases 1 lane/key      the doubling chain, 96 window bases
//   k384_keytab_rows  1 lane/window   15 affine entries, one inversion
//
// A pass with BH_F_BATCH_KEYS (comb384.h) groups its records by key instead:
//   k384_comb_group   1 lane/record   claim or find the key's bucket, count
//   k384_comb_assign  1 lane/record   representatives: registry, comb slot or ladder
//   k384_comb_plan    1 lane/record   the three index lists
//   k384_comb_bases   1 lane/comb     the doubling chain, 6 bases
//   k384_comb_rows    1 lane/comb     63 affine entries, one inversion
//   k384_comb         1 lane/record   comb route: 64 doublings, u2 Q + u1 G folded
//   k384_comb_g       1 lane          the comb of G, once per device
//
// An index-keyed shard (In384::key_idx: bh_verify384_compact,
// bh_batch_verify384_ptrs) imports its distinct keys once, ahead of its chunks:
//   k384_keys_prep        1 lane/key      key_import384, registry lookup -> Keys384
// k384_prep then gathers verdict and coordinates, k384_plan reads the key's
// slot, and a flagged pass groups by key index:
//   k384_comb_group_idx   1 lane/record   one atomic addition on cnt[key_idx[i]]
//   k384_comb_assign_idx  1 lane/key      registry, comb slot or ladder
//   k384_comb_bases_idx   1 lane/comb     the chain from the key workspace
//
// The host's entry points (namespace bh, at the end of the file):
//   launch_gtab384_build     k384_gtab
//   launch_comb384_g         k384_comb_g
//   launch_pass384           one pass by any of the three routes above (pass384.h)
//   launch_keys384_prep      k384_keys_prep
//   launch_keys384_register  the four registration kernels
#include "pass384.h"

using namespace bh;

constexpr uint32_t kInvChunk384 = 16;  // records per inversion

__global__ __launch_bounds__(64) void k384_gtab(uint32_t* __restrict__ gtab) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)(kG384Win * kG384Ent)) return;
  gtab384_entry(t, gtab);
}

__global__ __launch_bounds__(64) void k384_prep(In384 in, Work384 w, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  stage384_prep(in, w, i);
}

__global__ __launch_bounds__(64) void k384_inv(Work384 w, uint32_t stride, uint32_t n) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= stride) return;
  stage384_inv(w, c, stride, n);
}

__global__ __launch_bounds__(64) void k384_ladder(Work384 w, const uint32_t* __restrict__ gtab,
                                                  uint32_t n, uint8_t* __restrict__ reason) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = w.st[i] & 0x7fu;
  if (st != R_OK) {
    reason[i] = st;
    return;
  }
  reason[i] = stage384_ladder(w, gtab, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
}

__global__ __launch_bounds__(64) void k384_plan(In384 in, Work384 w, KeyReg384 g, uint32_t n,
                                                Plan384 pl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slot = i < n ? stage384_plan(in, w, g, i) : kNoSlot384;
  const bool hit = slot != kNoSlot384, miss = i < n && !hit;
  // one route per wave downstream: each wave appends its records to the two lists
  const uint64_t mh = __ballot(hit), mm = __ballot(miss);
  uint32_t bh_ = 0, bm_ = 0;
  if (lane == 0) {
    if (mh) bh_ = atomicAdd(&pl.cnt[0], (uint32_t)__popcll(mh));
    if (mm) bm_ = atomicAdd(&pl.cnt[1], (uint32_t)__popcll(mm));
  }
  bh_ = __shfl(bh_, 0);
  bm_ = __shfl(bm_, 0);
  const uint64_t below = (1ull << lane) - 1;
  if (hit) {
    pl.slot[i] = slot;
    pl.tab_list[bh_ + (uint32_t)__popcll(mh & below)] = i;
  } else if (miss) {
    pl.lad_list[bm_ + (uint32_t)__popcll(mm & below)] = i;
  }
}

__global__ __launch_bounds__(64) void k384_keywin(Work384 w, KeyReg384 g, Plan384 pl,
                                                  const uint32_t* __restrict__ gtab,
                                                  uint8_t* __restrict__ reason) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pl.cnt[0]) return;
  const uint32_t i = pl.tab_list[t];
  const uint32_t* qtab = g.tables + (size_t)pl.slot[i] * kKTab384Words;
  reason[i] = stage384_keywin(w, qtab, gtab, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
}

__global__ __launch_bounds__(64) void k384_ladder_list(Work384 w, Plan384 pl,
                                                       const uint32_t* __restrict__ gtab,
                                                       uint8_t* __restrict__ reason) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pl.cnt[1]) return;
  const uint32_t i = pl.lad_list[t];
  const uint8_t st = w.st[i] & 0x7fu;
  if (st != R_OK) {
    reason[i] = st;
    return;
  }
  reason[i] = stage384_ladder(w, gtab, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
}

__global__ __launch_bounds__(64) void k384_keys_import(const uint8_t* __restrict__ pub, uint32_t n,
                                                       uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t qx[14], qy[14];
  status[i] = key_import384(pub + (size_t)i * 96, qx, qy) ? (uint8_t)0 : (uint8_t)R_BAD_KEY;
}

__global__ __launch_bounds__(64) void k384_keys_insert(KeyReg384 g, const uint8_t* pub, uint32_t n,
                                                       uint8_t* status, uint32_t* fresh,
                                                       uint32_t* nfresh) {
  if (blockIdx.x == 0 && threadIdx.x == 0) keys384_insert(g, pub, n, status, fresh, nfresh);
}

__global__ __launch_bounds__(64) void k384_keytab_bases(KeyReg384 g, const uint32_t* __restrict__ fresh,
                                                        const uint32_t* __restrict__ nfresh,
                                                        uint32_t* __restrict__ bases) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= *nfresh) return;
  keytab384_bases(g, fresh[t], bases + (size_t)t * kG384Win * kBase384Words);
}

__global__ __launch_bounds__(64) void k384_keytab_rows(KeyReg384 g, const uint32_t* __restrict__ fresh,
                                                       const uint32_t* __restrict__ nfresh,
                                                       const uint32_t* __restrict__ bases) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t key = t / kG384Win, win = t % kG384Win;
  if (key >= *nfresh) return;
  keytab384_window(bases + (size_t)t * kBase384Words,
                   g.tables + (size_t)fresh[key] * kKTab384Words +
                       (size_t)win * kG384Ent * kG384Words);
}

// The claim of an empty bucket: the winner's value, ours or an earlier lane's.
struct Cas384 {
  __device__ uint32_t operator()(uint32_t* p, uint32_t v) const {
    const uint32_t old = atomicCAS(p, 0u, v);
    return old ? old : v;
  }
};

__global__ __launch_bounds__(64) void k384_comb_group(In384 in, Work384 w, Comb384 cb, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t b = kNoSlot384;
  if ((w.st[i] & 0x7fu) == R_OK) {
    b = comb384_claim(in, cb, i, Cas384{});
    if (b != kNoSlot384) atomicAdd(&cb.cnt[b], 1u);
  }
  cb.bkt[i] = b;
}

__global__ __launch_bounds__(64) void k384_comb_assign(In384 in, KeyReg384 g, Comb384 cb, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = cb.bkt[i];
  if (b == kNoSlot384 || cb.rep[b] != i + 1) return;
  uint32_t r = comb384_group_route(in, g, cb, i, b);
  if (r == 0) {
    r = atomicAdd(&cb.ctr[0], 1u);
    if (r < cb.cap) cb.slot_rep[r] = i;
    else r = kNoSlot384;  // (cap >= ns / min: not reached)
  }
  cb.gslot[b] = r;
}

__global__ __launch_bounds__(64) void k384_keys_prep(const uint8_t* __restrict__ pub, Keys384 kt,
                                                     KeyReg384 g) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= kt.nk) return;
  keys384_prep(pub, kt, g, j);
}

// The 64 records of a wave mostly share a few keys: the additions of one
// address are combined by the hardware's atomic unit in L2, one instruction
// per lane, no loop over the wave.
__global__ __launch_bounds__(64) void k384_comb_group_idx(In384 in, Work384 w, Comb384 cb,
                                                          uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t b = kNoSlot384;
  if ((w.st[i] & 0x7fu) == R_OK) {
    b = in.key_idx[i];
    atomicAdd(&cb.cnt[b], 1u);
  }
  cb.bkt[i] = b;
}

__global__ __launch_bounds__(64) void k384_comb_assign_idx(In384 in, Comb384 cb) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= in.kt.nk) return;
  uint32_t r = comb384_index_route(in.kt, cb, j);
  if (r == 0) {
    r = atomicAdd(&cb.ctr[0], 1u);
    if (r < cb.cap) cb.slot_rep[r] = j;
    else r = kNoSlot384;  // (cap >= ns / min: not reached)
  }
  cb.gslot[j] = r;
}

__global__ __launch_bounds__(64) void k384_comb_bases_idx(In384 in, Comb384 cb) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ns = cb.ctr[0] < cb.cap ? cb.ctr[0] : cb.cap;
  if (t >= ns) return;
  const uint32_t j = cb.slot_rep[t];
  uint32_t qx[14], qy[14];
  ldw<14>(qx, in.kt.qx, j, in.kt.nks);
  ldw<14>(qy, in.kt.qy, j, in.kt.nks);
  comb384_bases(qx, qy, cb.bases + (size_t)t * kComb384BaseWords);
}

__global__ __launch_bounds__(64) void k384_comb_plan(Comb384 cb, uint32_t n, Plan384 pl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t slot = 0;
  const int route = i < n ? comb384_record_route(cb, i, &slot) : -1;
  // one route per wave downstream: each wave appends its records to the three lists
  const uint64_t m0 = __ballot(route == 0), m1 = __ballot(route == 1), m2 = __ballot(route == 2);
  uint32_t b0 = 0, b1 = 0, b2 = 0;
  if (lane == 0) {
    if (m0) b0 = atomicAdd(&pl.cnt[1], (uint32_t)__popcll(m0));
    if (m1) b1 = atomicAdd(&cb.ctr[1], (uint32_t)__popcll(m1));
    if (m2) b2 = atomicAdd(&pl.cnt[0], (uint32_t)__popcll(m2));
  }
  b0 = __shfl(b0, 0);
  b1 = __shfl(b1, 0);
  b2 = __shfl(b2, 0);
  const uint64_t below = (1ull << lane) - 1;
  if (route == 0) {
    pl.lad_list[b0 + (uint32_t)__popcll(m0 & below)] = i;
  } else if (route == 1) {
    pl.slot[i] = slot;
    cb.list[b1 + (uint32_t)__popcll(m1 & below)] = i;
  } else if (route == 2) {
    pl.slot[i] = slot;
    pl.tab_list[b2 + (uint32_t)__popcll(m2 & below)] = i;
  }
}

__global__ __launch_bounds__(64) void k384_comb_bases(Work384 w, Comb384 cb) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ns = cb.ctr[0] < cb.cap ? cb.ctr[0] : cb.cap;
  if (t >= ns) return;
  const uint32_t i = cb.slot_rep[t];
  uint32_t qx[14], qy[14];
  ldw<14>(qx, w.qx, i, w.ns);
  ldw<14>(qy, w.qy, i, w.ns);
  comb384_bases(qx, qy, cb.bases + (size_t)t * kComb384BaseWords);
}

__global__ __launch_bounds__(64) void k384_comb_rows(Comb384 cb) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ns = cb.ctr[0] < cb.cap ? cb.ctr[0] : cb.cap;
  if (t >= ns) return;
  comb384_rows(cb.bases + (size_t)t * kComb384BaseWords, cb.side + (size_t)t * kComb384Words,
               cb.tables + (size_t)t * kComb384Words);
}

__global__ __launch_bounds__(64) void k384_comb(Work384 w, Comb384 cb, Plan384 pl,
                                                const uint32_t* __restrict__ gcomb,
                                                uint8_t* __restrict__ reason) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cb.ctr[1]) return;
  const uint32_t i = cb.list[t];
  const uint32_t* qtab = cb.tables + (size_t)pl.slot[i] * kComb384Words;
  reason[i] = stage384_comb(w, qtab, gcomb, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
}

// bases: kComb384BaseWords, side: kComb384Words (scratch of the build), gcomb: the table
__global__ __launch_bounds__(64) void k384_comb_g(uint32_t* bases, uint32_t* side, uint32_t* gcomb) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t gx[14], gy[14];
  f384_const(gx, Cv_p384::gx_m);
  f384_const(gy, Cv_p384::gy_m);
  comb384_bases(gx, gy, bases);
  comb384_rows(bases, side, gcomb);
}

__global__ __launch_bounds__(256) void k384_bitmap(const uint8_t* __restrict__ reason, uint32_t n,
                                                   uint64_t* __restrict__ bitmap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i & ~63u) >= n) return;
  const bool ok = i < n && reason[i] == R_OK;
  const uint64_t m = __ballot(ok);
  if ((threadIdx.x & 63u) == 0) bitmap[i >> 6] = m;
}

namespace bh {

hipError_t launch_gtab384_build(uint32_t* gtab, hipStream_t s) {
  const uint32_t t = (uint32_t)(kG384Win * kG384Ent);
  hipLaunchKernelGGL(k384_gtab, dim3((t + 63) / 64), dim3(64), 0, s, gtab);
  return hipGetLastError();
}

// The comb of G into gcomb (kComb384Words), with a comb slot's bases and side as scratch.
hipError_t launch_comb384_g(uint32_t* bases, uint32_t* side, uint32_t* gcomb, hipStream_t s) {
  hipLaunchKernelGGL(k384_comb_g, dim3(1), dim3(64), 0, s, bases, side, gcomb);
  return hipGetLastError();
}

// One pass of p.n records on s; its route follows from p (pass384.h).
//
// The ladder alone (no comb, p.reg.cap == 0): prep, inverse, k384_ladder over
// all n records, bitmap.
//
// With keys in the registry, or with BH_F_BATCH_KEYS: p.pl.cnt is cleared here
// (a comb pass: cb's per-pass counters and buckets, contiguous from cb.ctr,
// too). After the inverse the records are planned -- a comb pass groups them by
// key first -- into index lists; then, side by side, the ladder list on s,
// whose one wave per SIMD leaves registers for the table routes' waves, and on
// aux (fork / join order it after the plan and before the bitmap) the comb
// build and the comb route of a comb pass and, with p.reg.cap != 0, the
// registry's table route. The list kernels are launched for n lanes, the build
// kernels for cb.cap, and read their counts on the device.
//
// ev (optional): the events of Ev384 that the route has.
hipError_t launch_pass384(const Pass384& p, hipStream_t s, hipStream_t aux, hipEvent_t fork,
                          hipEvent_t join, hipEvent_t* ev) {
  const uint32_t n = p.n;
  if (n == 0) return hipSuccess;
  const In384& in = p.in;
  const Work384& w = p.w;
  const Plan384& pl = p.pl;
  const Comb384& cb = p.cb;
  const bool comb = cb.tables != nullptr, routed = comb || p.reg.cap != 0;
  hipError_t e;
  auto mark = [&](Ev384 k, hipStream_t on) { return ev ? hipEventRecord(ev[k], on) : hipSuccess; };
  const dim3 blk(64), grd((n + 63) / 64), grdk((cb.cap + 63) / 64);
  if (routed && (e = hipMemsetAsync(pl.cnt, 0, 8, s)) != hipSuccess) return e;
  if (comb && (e = hipMemsetAsync(cb.ctr, 0, p.zero_bytes, s)) != hipSuccess) return e;
  if ((e = mark(kEv384Start, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k384_prep, grd, blk, 0, s, in, w, n);
  if ((e = mark(kEv384Prep, s)) != hipSuccess) return e;
  const uint32_t stride = (n + kInvChunk384 - 1) / kInvChunk384;
  hipLaunchKernelGGL(k384_inv, dim3((stride + 63) / 64), blk, 0, s, w, stride, n);
  if ((e = mark(kEv384Inv, s)) != hipSuccess) return e;
  if (!routed) {
    hipLaunchKernelGGL(k384_ladder, grd, blk, 0, s, w, p.gtab, n, p.reason);
  } else {
    if (!comb) {
      hipLaunchKernelGGL(k384_plan, grd, blk, 0, s, in, w, p.reg, n, pl);
    } else {
      if (in.key_idx) {  // grouped by key index (cb.hc >= in.kt.nk)
        hipLaunchKernelGGL(k384_comb_group_idx, grd, blk, 0, s, in, w, cb, n);
        hipLaunchKernelGGL(k384_comb_assign_idx, dim3((in.kt.nk + 63) / 64), blk, 0, s, in, cb);
      } else {
        hipLaunchKernelGGL(k384_comb_group, grd, blk, 0, s, in, w, cb, n);
        hipLaunchKernelGGL(k384_comb_assign, grd, blk, 0, s, in, p.reg, cb, n);
      }
      hipLaunchKernelGGL(k384_comb_plan, grd, blk, 0, s, cb, n, pl);
    }
    if ((e = mark(kEv384Plan, s)) != hipSuccess) return e;
    if ((e = hipEventRecord(fork, s)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(aux, fork, 0)) != hipSuccess) return e;
    if (comb) {
      if (in.key_idx) hipLaunchKernelGGL(k384_comb_bases_idx, grdk, blk, 0, aux, in, cb);
      else hipLaunchKernelGGL(k384_comb_bases, grdk, blk, 0, aux, w, cb);
      hipLaunchKernelGGL(k384_comb_rows, grdk, blk, 0, aux, cb);
      if ((e = mark(kEv384Build, aux)) != hipSuccess) return e;
      hipLaunchKernelGGL(k384_comb, grd, blk, 0, aux, w, cb, pl, p.gcomb, p.reason);
    }
    if (p.reg.cap)
      hipLaunchKernelGGL(k384_keywin, grd, blk, 0, aux, w, p.reg, pl, p.gtab, p.reason);
    if ((e = mark(kEv384Routes, aux)) != hipSuccess) return e;
    if ((e = hipEventRecord(join, aux)) != hipSuccess) return e;
    hipLaunchKernelGGL(k384_ladder_list, grd, blk, 0, s, w, pl, p.gtab, p.reason);
    if ((e = mark(kEv384Ladder, s)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(s, join, 0)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k384_bitmap, dim3((n + 255) / 256), dim3(256), 0, s, p.reason, n, p.bitmap);
  if ((e = mark(kEv384End, s)) != hipSuccess) return e;
  return hipGetLastError();
}

// The distinct keys of an index-keyed shard (kt.nk of them at pub, device) into
// the key workspace kt, once per shard; g.cap == 0: no registry lookup.
hipError_t launch_keys384_prep(const uint8_t* pub, const Keys384& kt, const KeyReg384& g,
                               hipStream_t s) {
  if (kt.nk == 0) return hipSuccess;
  hipLaunchKernelGGL(k384_keys_prep, dim3((kt.nk + 63) / 64), dim3(64), 0, s, pub, kt, g);
  return hipGetLastError();
}

// bh_keys384_register's kernels for n keys at pub (device): verdicts, the
// serial insert, then the tables of the slots it handed out. bases: n * 96 *
// kBase384Words words; fresh: n + 1 words (the last is the count).
hipError_t launch_keys384_register(const KeyReg384& g, const uint8_t* pub, uint32_t n,
                                   uint8_t* status, uint32_t* fresh, uint32_t* bases,
                                   hipStream_t s) {
  if (n == 0) return hipSuccess;
  uint32_t* nfresh = fresh + n;
  hipLaunchKernelGGL(k384_keys_import, dim3((n + 63) / 64), dim3(64), 0, s, pub, n, status);
  hipLaunchKernelGGL(k384_keys_insert, dim3(1), dim3(64), 0, s, g, pub, n, status, fresh, nfresh);
  hipLaunchKernelGGL(k384_keytab_bases, dim3((n + 63) / 64), dim3(64), 0, s, g, fresh, nfresh, bases);
  const uint32_t t = n * (uint32_t)kG384Win;
  hipLaunchKernelGGL(k384_keytab_rows, dim3((t + 63) / 64), dim3(64), 0, s, g, fresh, nfresh, bases);
  return hipGetLastError();
}

}  // namespace bh
