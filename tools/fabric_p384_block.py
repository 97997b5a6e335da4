#!/usr/bin/env python3
"""Pre-verification latency of a Fabric block whose identities all hold P-384
keys, one JSON. Recorded, not gated.

  python tools/fabric_p384_block.py [--out profiles/p384/fabric_block.json] [--ntx 500]

The config-3 block of bdls_amd/workload/fabric.py with p384_orgs = norgs (ntx
transactions, a creator signature and three endorsements each, 1/100
corrupted), through bh_fabric_block_preverify, which sends it to the device as
one bh_verify_mixed batch. Three legs in one process on one device, each with
warm-up calls and then timed calls of the C entry point itself on the host
clock, output buffers allocated beforehand (p50, min, max):

  empty   the P-384 key registry empty: every record on the ladder
  warm    BH_FAB_F_KEEP_KEYS after two calls have registered the block's keys:
          the records of registered keys on the table route
  p256    the same block with p384_orgs = 0, for scale (config 3 itself)

Parity with the construction is checked on every call. Beside them: libcrypto
verifying the block's P-384 signatures (SHA-256 digests, as the MSP hashes) on
16 threads. Exit status 1 if parity fails. No torch; bench.py is not involved.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CPU_THREADS = 16


def stats(ms):
    ms = sorted(ms)
    return {"p50_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "calls": len(ms)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384", "fabric_block.json"))
    ap.add_argument("--ntx", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()

    import p384_rate as PR
    from bdls_amd import _lib, fabric
    from bdls_amd.provenance import kernel_src_sha
    from bdls_amd.workload import fabric as F
    from tests import p384_util as U

    fb384 = F.generate_fabric_block(ntx=a.ntx, p384_orgs=4, norgs=4)
    fb256 = F.generate_fabric_block(ntx=a.ntx)
    _lib.ensure_init(1)  # device 0
    L = _lib.lib()

    def count():
        c = ctypes.c_size_t()
        _lib.check(L.bh_keys384_count(0, ctypes.byref(c)))
        return c.value

    parity = [True]

    def leg(fb, keep, prime=0):
        want = [(fb.tx_status[i], fb.tx_creator[i], fb.tx_endorse[i], fb.tx_valid_identities[i])
                for i in range(fb.ntx)]
        buf = np.frombuffer(bytes(fb.block) + b"\0", np.uint8)
        ntx, nend = ctypes.c_size_t(), ctypes.c_size_t()
        txs = (_lib.BhFabTx * fb.ntx)()
        end = np.zeros(sum(len(e) for e in fb.tx_endorse) + 1, np.uint8)
        flags = _lib.BH_FAB_F_KEEP_KEYS if keep else 0
        ms = []
        for it in range(prime + a.warmup + a.steps):
            t0 = time.perf_counter()
            rc = L.bh_fabric_block_preverify(buf.ctypes.data, len(fb.block), flags, txs, fb.ntx,
                                             ctypes.byref(ntx), end.ctypes.data, len(end),
                                             ctypes.byref(nend))
            dt = (time.perf_counter() - t0) * 1e3
            _lib.check(rc)
            got = [(t.status, t.creator,
                    [int(x) for x in end[t.endorse_first:t.endorse_first + t.endorse_count]],
                    t.valid_endorsers) for t in txs[:ntx.value]]
            parity[0] &= got == want
            if it >= prime + a.warmup:
                ms.append(dt)
        return stats(ms)

    _lib.check(L.bh_keys384_reserve(0, 256))
    empty = leg(fb384, False)
    empty["keys_registered"] = count()
    warm = leg(fb384, True, prime=2)
    warm["keys_registered"] = count()
    _lib.check(L.bh_keys384_reserve(0, 256))
    p256 = leg(fb256, False)

    # libcrypto on the same signatures, CPU_THREADS threads (ctypes drops the GIL)
    _, creators, ends = fabric.block_preverify_refs(fb384.block, decode_only=True)
    by_ser = {i.serialized: i.pub for i in fb384.identities}
    refs = [r for r in creators + ends if r is not None and r.identity in by_ser]
    lc = U.LibCrypto()
    keys = {}
    for pub in set(by_ser.values()):
        keys[pub] = lc.key(None, int.from_bytes(pub[:48], "big"), int.from_bytes(pub[48:], "big"))
    work = [(keys[by_ser[r.identity]], hashlib.sha256(r.data).digest(), r.signature) for r in refs]

    def one(w):
        return lc.verify(*w)

    with ThreadPoolExecutor(CPU_THREADS) as ex:
        list(ex.map(one, work[:64]))
        t0 = time.perf_counter()
        ok = list(ex.map(one, work, chunksize=32))
        cpu_s = time.perf_counter() - t0
    for k in keys.values():
        lc.free_key(k)

    out = {
        "what": f"bh_fabric_block_preverify, {a.ntx}-tx block, every identity on P-384 "
                "(creator + 3 endorsements per tx, SHA-256): host clock per call of the C ABI",
        "ntx": a.ntx, "signatures": fb384.n_signatures, "block_bytes": len(fb384.block),
        "warmup": a.warmup, "steps": a.steps,
        "empty_registry": empty, "warm_registry": warm, "p256_block": p256,
        "warm_p50_ms": warm["p50_ms"],
        "cpu": {"what": f"libcrypto ECDSA_verify (secp384r1), {CPU_THREADS} threads",
                "signatures": len(work), "accepted": int(sum(ok)), "seconds": cpu_s,
                "rate_per_s": len(work) / cpu_s, "block_ms": cpu_s * 1e3,
                "openssl": PR.openssl_version(lc)},
        "parity": parity[0], "cpus_visible": len(os.sched_getaffinity(0)),
        "commit": PR.commit(), "kernel_src_sha": kernel_src_sha(), "version": L.bh_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if parity[0] else 1


if __name__ == "__main__":
    sys.exit(main())
