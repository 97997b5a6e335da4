#!/usr/bin/env python3
"""Resident P-384 verify rate with and without BH_F_BATCH_KEYS, one JSON.

  python tools/p384_comb_rate.py [--out profiles/p384/comb_rate.json] [--n 65536]

n libcrypto-signed records (256-byte messages, fused SHA-256, one in eight
corrupted by construction as in tools/p384_rate.py), resident, registry empty,
over 64, 4,096, 16,384 and n distinct keys: 1,024, 16, 4 and 1 uses per key,
the last shape with every record on the ladder, which shows what the flag
costs where it cannot help. Per shape, in one process on one device, after 2
warm-up pairs, unflagged and flagged bh_verify_dev(BH_CURVE_P384) passes
alternate: 10 timed passes each with stage events, then 10 each without events
timed by the host clock (wall_ms, what a caller sees). Parity with the
construction and the routing counts are checked on every pass. Exit status 1
if parity fails or the flagged pass at 64 keys is not faster than the
unflagged one of the same run. No torch; bench.py is not involved.
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
STAGES = ("prep_ms", "inv_ms", "plan_ms", "keycomb_ms", "build_ladder_ms")
KRES = os.path.join(ROOT, "profiles", "p384", "kres_comb.json")


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_keys(lc, nkeys, seed=384):
    """nkeys distinct keys d, d + 1, ...: a chain of additions of G."""
    import random
    from oracle import ecdsa_ref as O
    from tests import p384_util as U
    d = random.Random(seed).randrange(1, U.N - nkeys)
    pt = O.pubkey(U.P384, d)
    keys = []
    for k in range(nkeys):
        keys.append((pt[0], pt[1], lc.key(d + k, pt[0], pt[1])))
        pt = O.point_add(U.P384, pt, (U.P384.gx, U.P384.gy))
    return keys


def generate(lc, keys, n, msg_len=256, seed=384, threads=16):
    from oracle import ecdsa_ref as O
    from tests import p384_util as U
    nkeys = len(keys)
    msgs = np.random.default_rng(seed).integers(0, 256, (n, msg_len), dtype=np.uint8)
    kinds = ("msg_bit", "r_plus1", "high_s", "wrong_key", "offcurve_key")

    def one(i):
        qx, qy, k = keys[i % nkeys]
        r, s = lc.sign(k, hashlib.sha256(msgs[i].tobytes()).digest())
        s = min(s, U.N - s)
        reason = O.R_OK
        if i % 8 == 5:
            kind = kinds[(i // 8) % len(kinds)]
            if kind == "msg_bit":
                msgs[i, i % msg_len] ^= 1 << (i % 8)
                reason = O.R_MATH
            elif kind == "r_plus1":
                r, reason = (r + 1) % U.N or 1, O.R_MATH
            elif kind == "high_s":
                s, reason = U.N - s, O.R_HIGH_S
            elif kind == "wrong_key":
                qx, qy, _ = keys[(i + 1) % nkeys]
                reason = O.R_MATH
            else:
                qy, reason = (qy + 1) % U.P, O.R_BAD_KEY
        return qx.to_bytes(48, "big") + qy.to_bytes(48, "big"), O.marshal_ecdsa_signature(r, s), reason

    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(one, range(n), chunksize=256))
    pub = np.frombuffer(b"".join(r[0] for r in rows), np.uint8)
    sig, so, sl = U.pack_bytes([r[1] for r in rows])
    msg = np.concatenate([msgs.reshape(-1), np.zeros(8, np.uint8)])
    mo = np.arange(n, dtype=np.uint64) * msg_len
    ml = np.full(n, msg_len, np.uint32)
    want = np.array([r[2] for r in rows], np.uint8)
    return rows, (pub, sig, so, sl, msg, mo, ml), want


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384", "comb_rate.json"))
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kres-only", action="store_true")
    a = ap.parse_args()
    import p384_rate as R
    if a.kres_only:
        rows = {k: v for k, v in R.kernel_resources().items() if k.startswith("k384_comb")}
        with open(KRES, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)
        print(open(KRES).read())
        return 0

    from bdls_amd import _lib
    from bdls_amd.provenance import kernel_src_sha
    from tests import p384_util as U
    n = a.n
    lc = U.LibCrypto()
    all_keys = make_keys(lc, n)
    _lib.ensure_init(1)  # device 0
    L = _lib.lib()
    cnt = ctypes.c_size_t(1)
    _lib.check(L.bh_keys384_count(0, ctypes.byref(cnt)))
    assert cnt.value == 0
    F = _lib.BH_F_HASH_SHA256
    shapes, ok = {}, True
    for nkeys in (64, 4096, 16384, n):
        if nkeys > n:
            continue
        rows, arrs, want = generate(lc, all_keys[:nkeys], n)
        uses = {}
        for row, w in zip(rows, want):
            if w in (0, 9):
                uses[row[0]] = uses.get(row[0], 0) + 1
        on_comb = int(sum(1 for row, w in zip(rows, want) if w in (0, 9) and uses[row[0]] >= 4))
        tables = int(sum(1 for v in uses.values() if v >= 4))
        dev = [_lib.DeviceArray.from_numpy(0, x) for x in arrs]
        bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
        rs = _lib.DeviceArray(0, n)
        b = _lib.BhBatch(*[d.ptr for d in dev])

        def one(flag, timing):
            t = _lib.BhTiming() if timing else None
            t0 = time.perf_counter()
            _lib.check(L.bh_verify_dev(0, _lib.BH_CURVE_P384, ctypes.byref(b), n, F | flag, bm.ptr,
                                       rs.ptr, None, 1, ctypes.byref(t) if timing else None))
            wall = (time.perf_counter() - t0) * 1e3
            reason = rs.to_numpy(np.uint8, n)
            words = bm.to_numpy(np.uint64, (n + 63) // 64)
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
            par = bool((reason == want).all() and (bits == (want == 0)).all())
            if timing:
                exp = (on_comb, tables) if flag else (0, 0)
                par = par and (t.n_keycomb, t.n_keytables) == exp and t.n_keycomb + t.n_ladder == n
                return par, {k: float(getattr(t, k)) for k in STAGES}
            return par, wall

        legs = {"unflagged": {"runs": [], "wall": [], "parity": True},
                "flagged": {"runs": [], "wall": [], "parity": True}}
        for timing, key in ((True, "runs"), (False, "wall")):
            for it in range(a.warmup + a.steps):
                for name, flag in (("unflagged", 0), ("flagged", _lib.BH_F_BATCH_KEYS)):
                    par, v = one(flag, timing)
                    legs[name]["parity"] &= par
                    if it >= a.warmup:
                        legs[name][key].append(v)
        res = {"keys": nkeys, "uses_per_key": n // nkeys, "n_keycomb": on_comb, "n_keytables": tables,
               "rejected_by_construction": int((want != 0).sum())}
        for name, lg in legs.items():
            res[name] = {"wall_ms_median": med(lg["wall"]), "wall_ms_min": min(lg["wall"]),
                         "wall_ms_max": max(lg["wall"]),
                         "stage_ms_median": {k: med(r[k] for r in lg["runs"]) for k in STAGES},
                         "parity": lg["parity"]}
            ok &= lg["parity"]
        res["wall_speedup_flagged"] = res["unflagged"]["wall_ms_median"] / res["flagged"]["wall_ms_median"]
        shapes[str(nkeys)] = res
        print(json.dumps(res), flush=True)
        for d in dev + [bm, rs]:
            d.free()
    out = {"what": "bh_verify_dev(BH_CURVE_P384), resident, fused SHA-256, 256-byte messages, registry "
                   "empty: unflagged and BH_F_BATCH_KEYS passes alternating, by number of keys",
           "n": n, "warmup": a.warmup, "steps": a.steps, "shapes": shapes,
           "kernels": json.load(open(KRES)) if os.path.exists(KRES) else None,
           "commit": R.commit(), "kernel_src_sha": kernel_src_sha(), "version": L.bh_version().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    faster = "64" in shapes and shapes["64"]["wall_speedup_flagged"] > 1.0
    print("parity", ok, "faster at 64 keys", faster)
    return 0 if ok and faster else 1


if __name__ == "__main__":
    sys.exit(main())
