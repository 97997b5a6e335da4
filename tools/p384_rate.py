#!/usr/bin/env python3
"""Resident P-384 verify rate against single-thread OpenSSL, one JSON.

  python tools/p384_rate.py [--out profiles/p384/rate.json] [--n 65536]
  python tools/p384_rate.py --kres-only     # needs hipcc: writes profiles/p384/kres.json

Generates n libcrypto-signed records (256-byte messages, fused SHA-256, one in
eight corrupted by construction), keeps them resident (bh_dev_alloc), runs 3
warm-up and 10 timed bh_verify_dev(BH_CURVE_P384) passes with stage events,
checks the results against the construction, times libcrypto's ECDSA_verify on
2,000 of the same records on one thread, and writes the rate, the per-stage
milliseconds, the per-kernel VGPR / scratch / occupancy (profiles/p384/kres.json,
made by --kres-only where the compiler is), the CPU rate, the CPU quota the
gate assumes and the commit.

The gate: the resident rate must exceed 16 x the single-thread libcrypto rate
(16 CPUs is what a command gets on the boxes this was measured on); below
that a P-384 MSP is better left on the sw provider. Exit status 1 if it fails.
No torch; bench.py is not involved.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KRES = os.path.join(ROOT, "profiles", "p384", "kres.json")
CPU_QUOTA = 16


def kernel_resources() -> dict:
    """VGPRs, AGPRs, scratch bytes per lane and waves per SIMD of each P-384 kernel."""
    src = os.path.join(ROOT, "bdls_amd", "csrc", "verify384_kernels.hip")
    err = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-c",
                          src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
            cur = name.strip().split("(")[0]
            rows[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            key = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize": "scratch_bytes_per_lane",
                   "Occupancy": "waves_per_simd"}[m.group(1).split(" ")[0]]
            rows[cur][key] = int(m.group(2))
    assert rows, err[-2000:]
    return rows


def generate(n: int, nkeys: int = 64, threads: int = 16, msg_len: int = 256, seed: int = 384):
    """n records signed by libcrypto on `threads` threads (ctypes drops the GIL)."""
    import random
    from oracle import ecdsa_ref as O
    from tests import p384_util as U
    lc = U.LibCrypto()
    rng = random.Random(seed)
    keys = []
    for _ in range(nkeys):
        d = rng.randrange(1, U.N)
        qx, qy = O.pubkey(U.P384, d)
        keys.append((qx, qy, lc.key(d, qx, qy)))
    msgs = np.random.default_rng(seed).integers(0, 256, (n, msg_len), dtype=np.uint8)
    kinds = ("msg_bit", "r_plus1", "high_s", "wrong_key", "offcurve_key")

    def one(i):
        qx, qy, k = keys[i % nkeys]
        msg = msgs[i].tobytes()
        r, s = lc.sign(k, hashlib.sha256(msg).digest())
        if s > U.HALF:
            s = U.N - s
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
        return (qx.to_bytes(48, "big") + qy.to_bytes(48, "big"),
                O.marshal_ecdsa_signature(r, s), reason)

    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(one, range(n), chunksize=256))
    pub = np.frombuffer(b"".join(r[0] for r in rows), np.uint8)
    sig, so, sl = U.pack_bytes([r[1] for r in rows])
    msg = np.concatenate([msgs.reshape(-1), np.zeros(8, np.uint8)])
    mo = np.arange(n, dtype=np.uint64) * msg_len
    ml = np.full(n, msg_len, np.uint32)
    want = np.array([r[2] for r in rows], np.uint8)
    return lc, keys, rows, (pub, sig, so, sl, msg, mo, ml), want


def cpu_rate(lc, arrs, want, count: int = 2000):
    """libcrypto ECDSA_verify, one thread, over the first `count` records whose
    key OpenSSL accepts (a record with an off-curve key cannot be given to it);
    its verdict is checked against the construction."""
    from tests import p384_util as U
    pub, sig, so, sl, msg, mo, ml = arrs
    items = []
    for i in range(len(sl)):
        if len(items) == count:
            break
        q = pub[96 * i:96 * i + 96].tobytes()
        k = lc.key(None, int.from_bytes(q[:48], "big"), int.from_bytes(q[48:], "big"))
        if k is None:
            continue
        m = msg[int(mo[i]):int(mo[i]) + int(ml[i])].tobytes()
        items.append((k, hashlib.sha256(m).digest(), sig[int(so[i]):int(so[i]) + int(sl[i])].tobytes(),
                      int(want[i])))
    live = items
    t0 = time.perf_counter()
    got = [lc.verify(k, dg, sg) for k, dg, sg, _ in live]
    dt = time.perf_counter() - t0
    # OpenSSL knows no low-S rule: a high-S record is a valid signature to it
    ok = all(g == (w in (0, 6)) for g, (_, _, _, w) in zip(got, live))
    for k, *_ in live:
        lc.free_key(k)
    return len(live) / dt, ok, len(live)


def openssl_version(lc) -> str | None:
    try:
        fn = lc.L.OpenSSL_version
    except AttributeError:
        return None
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_int]
    return fn(0).decode()


def commit() -> str | None:
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                         text=True).stdout.strip()
    if rev:
        return rev
    info = os.path.join(ROOT, "bdls_amd", "lib", "BUILD_INFO.json")
    return json.load(open(info)).get("git_rev") if os.path.exists(info) else None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384", "rate.json"))
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kres-only", action="store_true")
    a = ap.parse_args()
    if a.kres_only:
        os.makedirs(os.path.dirname(KRES), exist_ok=True)
        with open(KRES, "w") as f:
            json.dump(kernel_resources(), f, indent=1, sort_keys=True)
        print(open(KRES).read())
        return 0

    from bdls_amd import _lib
    from bdls_amd.provenance import kernel_src_sha
    t0 = time.perf_counter()
    lc, keys, rows, arrs, want = generate(a.n)
    gen_s = time.perf_counter() - t0
    _lib.ensure_init(1)  # device 0
    n = a.n
    dev = [_lib.DeviceArray.from_numpy(0, x) for x in arrs]
    bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
    rs = _lib.DeviceArray(0, n)
    b = _lib.BhBatch(*[d.ptr for d in dev])
    L = _lib.lib()
    stages = ("prep_ms", "inv_ms", "build_ladder_ms")
    runs = []
    for it in range(a.warmup + a.steps):
        t = _lib.BhTiming()
        _lib.check(L.bh_verify_dev(0, _lib.BH_CURVE_P384, ctypes.byref(b), n, _lib.BH_F_HASH_SHA256,
                                   bm.ptr, rs.ptr, None, 1, ctypes.byref(t)))
        if it >= a.warmup:
            runs.append({k: float(getattr(t, k)) for k in stages})
        assert t.n_ladder == n
    reason = rs.to_numpy(np.uint8, n)
    words = bm.to_numpy(np.uint64, (n + 63) // 64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    parity = bool((reason == want).all() and (bits == (want == 0)).all())
    total = sorted(sum(r.values()) for r in runs)
    med = total[len(total) // 2]
    rate = n / (med * 1e-3)
    crate, cpu_ok, cpu_n = cpu_rate(lc, arrs, want)
    gate = rate > CPU_QUOTA * crate
    out = {
        "what": "bh_verify_dev(BH_CURVE_P384), resident, fused SHA-256, 256-byte messages",
        "n": n, "warmup": a.warmup, "steps": a.steps,
        "rate_per_s": rate, "pass_ms_median": med, "pass_ms_min": total[0], "pass_ms_max": total[-1],
        "stage_ms_median": {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in stages},
        "parity": parity, "rejected_by_construction": int((want != 0).sum()),
        "kernels": json.load(open(KRES)) if os.path.exists(KRES) else None,
        "cpu": {"what": "libcrypto ECDSA_verify (secp384r1), one thread", "records": cpu_n,
                "rate_per_s": crate, "verdicts_match_construction": cpu_ok,
                "openssl": openssl_version(lc)},
        "cpu_quota": CPU_QUOTA, "cpus_visible": len(os.sched_getaffinity(0)),
        "gate": {"rule": "rate_per_s > cpu_quota * cpu.rate_per_s", "threshold_per_s": CPU_QUOTA * crate,
                 "ratio_to_one_thread": rate / crate, "met": bool(gate)},
        "generate_s": gen_s, "commit": commit(), "kernel_src_sha": kernel_src_sha(),
        "version": L.bh_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    for d in dev + [bm, rs]:
        d.free()
    return 0 if (parity and gate and cpu_ok) else 1


if __name__ == "__main__":
    sys.exit(main())
