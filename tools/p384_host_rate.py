#!/usr/bin/env python3
"""Host-path P-384 verify rate: bh_verify against the P-384 BatchVerify, one JSON.

  python tools/p384_host_rate.py [--out profiles/p384/host_rate.json] [--sizes 65536,262144]

For each size: libcrypto-signed records (tools/p384_rate.py's generator: 64
keys, 256-byte messages, one in eight corrupted by construction) in
caller-owned pageable numpy buffers, fused SHA-256, BH_F_BATCH_KEYS on; first
with the P-384 registry empty, then with the 64 keys registered. Three ways
to verify the same batch, five alternating runs of each, wall-clock around the
calls, the median and the range recorded:

  bh_verify         bh_verify(BH_CURVE_P384) on the expanded batch: the yardstick,
                    the parent's behaviour on the same box in the same run
  ptrs              bh_batch_verify384_ptrs from per-record pointers
  ptrs_submit_x4    four bh_batch_verify384_ptrs_submit jobs of the batch kept in
                    flight (the rate counts all four batches)

Every run's reasons are checked against the construction. The new path is
expected not to be slower than the yardstick beyond the run-to-run range this
file records; the verdict is written, never tuned. On a box with one device
the multi-device rate is recorded as unmeasured. No torch; bench.py is not involved.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pointer_batch(arrs):
    """bh_pbatch over the SoA arrays: per-record addresses into the caller's buffers."""
    from bdls_amd import _lib
    pub, sig, so, sl, msg, mo, ml = arrs
    n = len(sl)
    cols = (pub.ctypes.data + 96 * np.arange(n, dtype=np.uint64),
            sig.ctypes.data + so, msg.ctypes.data + mo)
    cols = [np.ascontiguousarray(c, np.uint64) for c in cols]
    pb = _lib.BhPBatch(cols[0].ctypes.data, cols[1].ctypes.data, sl.ctypes.data,
                       cols[2].ctypes.data, ml.ctypes.data)
    return pb, cols


def stats(rates):
    return {"median": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates)),
            "runs": [float(r) for r in rates]}


def measure(L, arrs, want, runs, inflight):
    from bdls_amd import _lib
    n = len(want)
    flags = _lib.BH_F_HASH_SHA256 | _lib.BH_F_BATCH_KEYS
    b = _lib.BhBatch(*[a.ctypes.data for a in arrs])
    pb, keep = pointer_batch(arrs)
    outs = [(np.zeros((n + 7) // 8, np.uint8), np.zeros(n, np.uint8)) for _ in range(inflight)]

    def expanded():
        bm, rs = outs[0]
        _lib.check(L.bh_verify(_lib.BH_CURVE_P384, ctypes.byref(b), n, flags, bm.ctypes.data,
                               rs.ctypes.data))
        return 1

    def ptrs():
        bm, rs = outs[0]
        _lib.check(L.bh_batch_verify384_ptrs(ctypes.byref(pb), n, flags, bm.ctypes.data,
                                             rs.ctypes.data))
        return 1

    def submit():
        jobs = []
        for bm, rs in outs:
            j = ctypes.c_void_p()
            _lib.check(L.bh_batch_verify384_ptrs_submit(ctypes.byref(pb), n, flags, bm.ctypes.data,
                                                        rs.ctypes.data, ctypes.byref(j)))
            jobs.append(j)
        for j in jobs:
            _lib.check(L.bh_verify_wait(j))
        return len(jobs)

    ways = (("bh_verify", expanded), ("ptrs", ptrs), (f"ptrs_submit_x{inflight}", submit))
    for _, fn in ways:  # warm-up: workspaces, staging, the packer's pool
        fn()
    rates = {name: [] for name, _ in ways}
    for _ in range(runs):  # alternating
        for name, fn in ways:
            for _, rs in outs:
                rs[:] = 255
            t0 = time.perf_counter()
            k = fn()
            dt = time.perf_counter() - t0
            for _, rs in outs[:k]:
                assert (rs == want).all(), name
            rates[name].append(k * n / dt)
    del keep
    return {name: stats(r) for name, r in rates.items()}


def verdict(res):
    """The new path against the yardstick's own run-to-run range."""
    base = res["bh_verify"]
    out = {}
    for name, r in res.items():
        if name == "bh_verify":
            continue
        out[name] = {"ratio_of_medians": r["median"] / base["median"],
                     "slower_beyond_range": bool(r["median"] < base["min"])}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384", "host_rate.json"))
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    a = ap.parse_args()

    import p384_rate as R
    from bdls_amd import _lib
    sizes = [int(x) for x in a.sizes.split(",")]
    t0 = time.perf_counter()
    lc, keys, rows, arrs_all, want_all = R.generate(max(sizes))
    gen_s = time.perf_counter() - t0
    _lib.ensure_init()
    L = _lib.lib()
    ndev = L.bh_device_count()
    key_bytes = b"".join(qx.to_bytes(48, "big") + qy.to_bytes(48, "big") for qx, qy, _ in keys)
    out = {"tool": "tools/p384_host_rate.py", "commit": R.commit(), "devices": ndev,
           "keys": len(keys), "msg_len": 256, "hash": "fused SHA-256", "flags": "BH_F_BATCH_KEYS",
           "inputs": "caller-owned pageable numpy buffers", "runs": a.runs,
           "unit": "records per second, wall clock around the calls", "generate_s": gen_s,
           "shapes": []}
    pub, sig, so, sl, msg, mo, ml = arrs_all
    for n in sizes:
        arrs = (pub[:96 * n], sig, so[:n], sl[:n], msg, mo[:n], ml[:n])
        want = want_all[:n]
        for registry in ("empty", "64 keys"):
            _lib.check(L.bh_keys384_clear(-1))
            if registry != "empty":
                st = np.zeros(len(keys), np.uint8)
                _lib.check(L.bh_keys384_register(-1, key_bytes, len(keys), st.ctypes.data))
                assert (st == 0).all()
            res = measure(L, arrs, want, a.runs, a.inflight)
            out["shapes"].append({"records": n, "registry": registry, "rates": res,
                                  "against_bh_verify": verdict(res)})
            print(json.dumps(out["shapes"][-1]), flush=True)
    _lib.check(L.bh_keys384_clear(-1))
    out["multi_device"] = ("measured over %d devices" % ndev if ndev > 1 else
                           "unmeasured: one device on this box (bh_verify uses the first device "
                           "alone; the new entry points shard over all of them)")
    out["slower_anywhere"] = any(v["slower_beyond_range"] for s in out["shapes"]
                                 for v in s["against_bh_verify"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({"out": a.out, "slower_anywhere": out["slower_anywhere"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
