#!/usr/bin/env python3
"""Resident P-384 verify rate with and without the key registry, one JSON.

  python tools/p384_keys_rate.py [--out profiles/p384/keys_rate.json] [--n 65536]

The batch of tools/p384_rate.py (n libcrypto-signed records over 64 keys,
256-byte messages, fused SHA-256, one in eight corrupted by construction),
resident, run three ways in one process on one device, each with 3 warm-up and
10 timed bh_verify_dev(BH_CURVE_P384) passes with stage events (pass_ms: the
stages, the two routes counted as the longer of them since they overlap) and
as many synchronous passes without events timed by the host clock (wall_ms):

  empty     no key registered: every record on the ladder (the yardstick;
            compare profiles/p384/rate.json)
  all       every key registered: every record that passes prep on the table route
  half      every other key registered: both routes in every wave of the plan

Parity with the construction is checked on every leg. Then bh_keys384_register
is timed for 1, 64 and 1,024 fresh keys (registry reserved and emptied before
each), and the break-even uses per key follow from the per-key build time and
the per-record saving. Exit status 1 if parity fails or `all` is not faster
than `empty`. No torch; bench.py is not involved.
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
STAGES = ("prep_ms", "inv_ms", "plan_ms", "keycomb_ms", "build_ladder_ms")


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384", "keys_rate.json"))
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()

    import p384_rate as R
    from bdls_amd import _lib
    from bdls_amd.provenance import kernel_src_sha
    from oracle import ecdsa_ref as O
    from tests import p384_util as U

    lc, keys, rows, arrs, want = R.generate(a.n)
    n = a.n
    _lib.ensure_init(1)  # device 0
    L = _lib.lib()
    dev = [_lib.DeviceArray.from_numpy(0, x) for x in arrs]
    bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
    rs = _lib.DeviceArray(0, n)
    b = _lib.BhBatch(*[d.ptr for d in dev])
    raw = [qx.to_bytes(48, "big") + qy.to_bytes(48, "big") for qx, qy, _ in keys]

    def register(ks):
        st = np.zeros(len(ks), np.uint8)
        t0 = time.perf_counter()
        _lib.check(L.bh_keys384_register(0, b"".join(ks), len(ks), st.ctypes.data))
        return (time.perf_counter() - t0) * 1e3, st

    def leg(name, ks):
        _lib.check(L.bh_keys384_reserve(0, 256))
        if ks:
            assert (register(ks)[1] == 0).all()
        reg = set(ks)
        on_table = int(sum(1 for row, w in zip(rows, want) if w in (0, 9) and row[0] in reg))
        runs = []
        for it in range(a.warmup + a.steps):
            t = _lib.BhTiming()
            _lib.check(L.bh_verify_dev(0, _lib.BH_CURVE_P384, ctypes.byref(b), n,
                                       _lib.BH_F_HASH_SHA256, bm.ptr, rs.ptr, None, 1,
                                       ctypes.byref(t)))
            assert t.n_keycomb == on_table and t.n_keycomb + t.n_ladder == n, (name, t.n_keycomb)
            if it >= a.warmup:
                runs.append({k: float(getattr(t, k)) for k in STAGES})
        # and the pass as a caller sees it: synchronous calls without stage events, host clock
        wall = []
        for it in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            _lib.check(L.bh_verify_dev(0, _lib.BH_CURVE_P384, ctypes.byref(b), n,
                                       _lib.BH_F_HASH_SHA256, bm.ptr, rs.ptr, None, 1, None))
            if it >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        reason = rs.to_numpy(np.uint8, n)
        words = bm.to_numpy(np.uint64, (n + 63) // 64)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        parity = bool((reason == want).all() and (bits == (want == 0)).all())
        # the two routes run side by side after the plan: a pass is as long as the longer one
        total = sorted(r["prep_ms"] + r["inv_ms"] + r["plan_ms"] +
                       max(r["keycomb_ms"], r["build_ladder_ms"]) for r in runs)
        m = total[len(total) // 2]
        return {"keys_registered": len(ks), "n_keycomb": on_table, "n_ladder": n - on_table,
                "rate_per_s": n / (m * 1e-3), "pass_ms_median": m, "pass_ms_min": total[0],
                "pass_ms_max": total[-1],
                "wall_ms_median": med(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
                "wall_rate_per_s": n / (med(wall) * 1e-3),
                "stage_ms_median": {k: med(r[k] for r in runs) for k in STAGES},
                "stage_ms_min_max": {k: [min(r[k] for r in runs), max(r[k] for r in runs)]
                                     for k in STAGES},
                "parity": parity}

    legs = {"empty": leg("empty", []), "all": leg("all", raw), "half": leg("half", raw[::2])}

    # registration time for fresh keys (distinct points d G, d small: any valid point will do)
    import random
    rng = random.Random(1024)
    fresh = []
    pt = O.pubkey(U.P384, rng.randrange(1, U.N))
    for _ in range(1024):  # a chain of additions of G: 1,024 distinct points, cheaply
        pt = O.point_add(U.P384, pt, (U.P384.gx, U.P384.gy))
        fresh.append(pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big"))
    reg_ms = {}
    for k in (1, 64, 1024):
        ts = []
        for _ in range(3):
            _lib.check(L.bh_keys384_reserve(0, 1024))
            ms, st = register(fresh[:k])
            assert (st == 0).all()
            ts.append(ms)
        reg_ms[str(k)] = {"ms_median": med(ts), "ms_min": min(ts), "ms_max": max(ts),
                          "ms_per_key": med(ts) / k}
    _lib.check(L.bh_keys384_reserve(0, 256))

    e, al = legs["empty"], legs["all"]
    # per record, in a full pass: what the table route saves over the ladder
    lad_us = e["stage_ms_median"]["build_ladder_ms"] / n * 1e3
    tab_us = (al["stage_ms_median"]["keycomb_ms"] + al["stage_ms_median"]["plan_ms"]) / \
        max(al["n_keycomb"], 1) * 1e3
    build_us = reg_ms["1024"]["ms_per_key"] * 1e3
    out = {
        "what": "bh_verify_dev(BH_CURVE_P384), resident, fused SHA-256, 256-byte messages, "
                "64 keys: registry empty / all keys registered / every other key registered",
        "n": n, "warmup": a.warmup, "steps": a.steps, "legs": legs,
        "speedup_all_over_empty": al["rate_per_s"] / e["rate_per_s"],
        "speedup_half_over_empty": legs["half"]["rate_per_s"] / e["rate_per_s"],
        "wall_speedup_all_over_empty": e["wall_ms_median"] / al["wall_ms_median"],
        "wall_speedup_half_over_empty": e["wall_ms_median"] / legs["half"]["wall_ms_median"],
        "curve_stage_us_per_record": {"ladder": lad_us, "table_route_with_plan": tab_us,
                                      "ratio": lad_us / tab_us},
        "product_count_ratio_predicted": 2.8,
        "register_ms": reg_ms,
        "break_even_uses_per_key": {
            "rule": "register ms per key (1,024 keys at once) / (ladder - table route) us per record "
                    "in a full pass",
            "uses": build_us / max(lad_us - tab_us, 1e-9)},
        "rejected_by_construction": int((want != 0).sum()),
        "kernels": json.load(open(R.KRES)) if os.path.exists(R.KRES) else None,
        "commit": R.commit(), "kernel_src_sha": kernel_src_sha(), "version": L.bh_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    for d in dev + [bm, rs]:
        d.free()
    ok = all(l["parity"] for l in legs.values()) and al["rate_per_s"] > e["rate_per_s"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
