#!/usr/bin/env python3
"""SHA-384 digest pre-pass rate and its cost inside a verify call, one JSON.

  python tools/sha512_rate.py [--out profiles/sha512/rate.json] [--n 1048576]
  python tools/sha512_rate.py --kres-only   # needs hipcc: writes profiles/sha512/kres.json

n records with 256-byte messages, resident (bh_dev_alloc): 65,536 distinct
signed records per curve (libcrypto, over the SHA-384 of the message, one in
eight corrupted by construction) repeated to n. 3 warm-up and 10 timed
bh_verify_dev passes with stage events per leg; median, min and max:

  digest_pass   k_sha512<48> alone. The C ABI has no entry that launches the
                digest pass by itself, so it is the event-timed prep_ms of the
                P-384 + BH_F_HASH_SHA384 call (digest pass + k384_prep, each
                between its own events) minus the event-timed prep_ms of the
                same records in digest mode (k384_prep alone), pass by pass.
  p384          BH_CURVE_P384 + BH_F_HASH_SHA384 against BH_CURVE_P384 in
                digest mode over the SHA-384 digests.
  p256          BH_CURVE_P256 + BH_F_HASH_SHA384 against BH_CURVE_P256 +
                BH_F_HASH_SHA256 (the fused path, which this feature does not
                touch) on the same batch; under SHA-256 the signatures do not
                verify, which costs the same arithmetic.

The gate is the work the feature replaces: libcrypto SHA-384 of 256-byte
messages on the host, one thread (`openssl speed`), times CPU_QUOTA = 16
threads, the rule profiles/p384/rate.json uses. The device digest pass must be
faster. Exit status 1 if it is not, or if a leg's results differ from the
construction. No torch; bench.py is not involved.
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
KRES = os.path.join(ROOT, "profiles", "sha512", "kres.json")
CPU_QUOTA = 16
DISTINCT = 65536
MSG_LEN = 256
NID = {"P-256": 415, "P-384": 715}  # NID_X9_62_prime256v1, NID_secp384r1


def kernel_resources() -> dict:
    """VGPRs, AGPRs, scratch bytes per lane and waves per SIMD of each digest kernel."""
    src = os.path.join(ROOT, "bdls_amd", "csrc", "sha512_kernels.hip")
    err = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-c",
                          src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
            cur = re.sub(r"^void ", "", name.strip()).split("(")[0]
            rows[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            key = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize": "scratch_bytes_per_lane",
                   "Occupancy": "waves_per_simd"}[m.group(1).split(" ")[0]]
            rows[cur][key] = int(m.group(2))
    assert rows, err[-2000:]
    return rows


def generate(curve: str, threads: int = 16, seed: int = 512):
    """DISTINCT records of one curve signed by libcrypto over SHA-384(msg)."""
    import random
    from oracle import ecdsa_ref as O
    from tests import sha2wide_util as W
    lc = W.LibCrypto()
    L = lc.L
    c = W.CURVES[curve][0]
    cb = (c.p.bit_length() + 7) // 8
    half = c.n >> 1
    rng = random.Random(seed)

    def mk_key(d, qx, qy):
        k = L.EC_KEY_new_by_curve_name(NID[curve])
        x, y, bd = lc._bn(qx), lc._bn(qy), lc._bn(d)
        assert L.EC_KEY_set_public_key_affine_coordinates(k, x, y) == 1
        L.EC_KEY_set_private_key(k, bd)
        for b in (x, y, bd):
            L.BN_free(b)
        return k

    keys = []
    for _ in range(64):
        d = rng.randrange(1, c.n)
        qx, qy = O.pubkey(c, d)
        keys.append((qx, qy, mk_key(d, qx, qy)))
    msgs = np.random.default_rng(seed).integers(0, 256, (DISTINCT, MSG_LEN), dtype=np.uint8)
    kinds = ("msg_bit", "r_plus1", "high_s", "wrong_key", "offcurve_key")

    def one(i):
        qx, qy, k = keys[i % 64]
        r, s = lc.sign(k, hashlib.sha384(msgs[i].tobytes()).digest())
        if s > half:
            s = c.n - s
        reason = O.R_OK
        if i % 8 == 5:
            kind = kinds[(i // 8) % len(kinds)]
            if kind == "msg_bit":
                msgs[i, i % MSG_LEN] ^= 1 << (i % 8)
                reason = O.R_MATH
            elif kind == "r_plus1":
                r, reason = (r + 1) % c.n or 1, O.R_MATH
            elif kind == "high_s":
                s, reason = c.n - s, O.R_HIGH_S
            elif kind == "wrong_key":
                qx, qy, _ = keys[(i + 1) % 64]
                reason = O.R_MATH
            else:
                qy, reason = (qy + 1) % c.p, O.R_BAD_KEY
        return qx.to_bytes(cb, "big") + qy.to_bytes(cb, "big"), O.marshal_ecdsa_signature(r, s), reason

    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(one, range(DISTINCT), chunksize=256))
    for *_, k in keys:
        L.EC_KEY_free(k)
    return rows, msgs


def tile(rows, msgs, n: int):
    """The DISTINCT records repeated to n: SoA arrays, SHA-384 digests, reasons."""
    from tests.p384_util import pack_bytes
    reps = (n + DISTINCT - 1) // DISTINCT
    pub = np.tile(np.frombuffer(b"".join(r[0] for r in rows), np.uint8), reps)[:n * len(rows[0][0])]
    sigs = ([r[1] for r in rows] * reps)[:n]
    sig, so, sl = pack_bytes(sigs)
    msg = np.concatenate([np.tile(msgs.reshape(-1), reps)[:n * MSG_LEN], np.zeros(8, np.uint8)])
    mo = np.arange(n, dtype=np.uint64) * MSG_LEN
    ml = np.full(n, MSG_LEN, np.uint32)
    dg1 = np.frombuffer(b"".join(hashlib.sha384(m.tobytes()).digest() for m in msgs), np.uint8)
    dig = np.concatenate([np.tile(dg1, reps)[:n * 48], np.zeros(8, np.uint8)])
    do = np.arange(n, dtype=np.uint64) * 48
    dl = np.full(n, 48, np.uint32)
    want = np.tile(np.array([r[2] for r in rows], np.uint8), reps)[:n]
    return (pub, sig, so, sl), (msg, mo, ml), (dig, do, dl), want


def host_sha384_rate():
    """libcrypto SHA-384 of 256-byte messages per second, one thread."""
    try:
        out = subprocess.run(["openssl", "speed", "-mr", "-seconds", "2", "-bytes", str(MSG_LEN),
                              "-evp", "sha384"], capture_output=True, text=True, timeout=60).stdout
        m = re.search(r"^\+F:[^:]*:[^:]*:([0-9.]+)", out, re.M)
        if m:
            return float(m.group(1)) / MSG_LEN, "openssl speed -evp sha384 -bytes 256, one thread"
    except (OSError, subprocess.SubprocessError):
        pass
    data = [os.urandom(MSG_LEN) for _ in range(200000)]
    t0 = time.perf_counter()
    for d in data:
        hashlib.sha384(d).digest()
    return len(data) / (time.perf_counter() - t0), "hashlib.sha384 loop, one thread"


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def commit():
    from tools.p384_rate import commit as c
    return c()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha512", "rate.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
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
    from tests import sha2wide_util as W
    n = a.n
    L = _lib.lib()
    _lib.ensure_init(1)  # device 0
    bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
    rs = _lib.DeviceArray(0, n)
    legs, parity, gen_s = {}, {}, {}

    def run(curve, rec, msg, flags, want):
        """Per-pass (total ms, prep ms) of warmup + steps passes; parity of the last."""
        b = _lib.BhBatch(*[d.ptr for d in rec + msg])
        out = []
        for it in range(a.warmup + a.steps):
            t = _lib.BhTiming()
            _lib.check(L.bh_verify_dev(0, W.CURVES[curve][1], ctypes.byref(b), n, flags, bm.ptr, rs.ptr,
                                       None, 1, ctypes.byref(t)))
            if it >= a.warmup:
                out.append((t.prep_ms + t.inv_ms + t.plan_ms + t.build_ladder_ms + t.publish_ms +
                            t.keycomb_ms, t.prep_ms))
        reason = rs.to_numpy(np.uint8, n)
        words = bm.to_numpy(np.uint64, (n + 63) // 64)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        return out, bool((reason == want).all() and (bits == (want == 0)).all())

    for curve in ("P-384", "P-256"):
        t0 = time.perf_counter()
        rows, msgs = generate(curve)
        rec_h, msg_h, dig_h, want = tile(rows, msgs, n)
        gen_s[curve] = time.perf_counter() - t0
        rec = [_lib.DeviceArray.from_numpy(0, x) for x in rec_h]
        msg = [_lib.DeviceArray.from_numpy(0, x) for x in msg_h]
        wide, ok_w = run(curve, rec, msg, _lib.BH_F_HASH_SHA384, want)
        if curve == "P-384":
            dig = [_lib.DeviceArray.from_numpy(0, x) for x in dig_h]
            base, ok_b = run(curve, rec, dig, 0, want)
            for d in dig:
                d.free()
            dp = [w[1] - b[1] for w, b in zip(wide, base)]
            legs["digest_pass"] = {
                "what": "k_sha512<48>: prep_ms with BH_F_HASH_SHA384 minus prep_ms in digest mode",
                "ms": stats(dp), "digests_per_s": n / (stats(dp)["median"] * 1e-3)}
            against = "BH_CURVE_P384, digest mode over the SHA-384 digests"
        else:
            # under SHA-256 no signature made over SHA-384 verifies: the arithmetic rejects
            # what the construction accepted
            want256 = np.where(want == 0, 9, want).astype(np.uint8)
            base, ok_b = run(curve, rec, msg, _lib.BH_F_HASH_SHA256, want256)
            against = ("BH_CURVE_P256 + BH_F_HASH_SHA256 (fused; code this change does not touch), "
                       "same batch")
        mw, mb = stats([w[0] for w in wide]), stats([b[0] for b in base])
        legs["p384" if curve == "P-384" else "p256"] = {
            "what": f"bh_verify_dev({curve}) + BH_F_HASH_SHA384", "against": against,
            "pass_ms": mw, "against_pass_ms": mb, "rate_per_s": n / (mw["median"] * 1e-3),
            "against_rate_per_s": n / (mb["median"] * 1e-3), "slowdown": mw["median"] / mb["median"]}
        parity[curve] = ok_w and ok_b
        for d in rec + msg:
            d.free()
    crate, chow = host_sha384_rate()
    drate = legs["digest_pass"]["digests_per_s"]
    out = {
        "what": f"SHA-384 digest pre-pass, {n} x {MSG_LEN}-byte messages, resident",
        "n": n, "msg_len": MSG_LEN, "distinct_records": DISTINCT, "warmup": a.warmup, "steps": a.steps,
        **legs,
        "parity": bool(all(parity.values())), "parity_by_curve": parity,
        "kernels": json.load(open(KRES)) if os.path.exists(KRES) else None,
        "cpu": {"what": chow, "rate_per_s": crate},
        "cpu_quota": CPU_QUOTA,
        "gate": {"rule": "digest_pass.digests_per_s > cpu_quota * cpu.rate_per_s",
                 "threshold_per_s": CPU_QUOTA * crate, "ratio_to_one_thread": drate / crate,
                 "ratio_to_quota": drate / (CPU_QUOTA * crate), "met": bool(drate > CPU_QUOTA * crate)},
        "generate_s": gen_s, "commit": commit(),
        "commit_note": "the commit the measured tree was built on; kernel_src_sha identifies its "
                       "kernel sources (every .hip unit linked into the library, csrc/*.h, Makefile)",
        "kernel_src_sha": kernel_src_sha(),
        "version": L.bh_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    bm.free()
    rs.free()
    return 0 if (out["parity"] and out["gate"]["met"]) else 1


if __name__ == "__main__":
    sys.exit(main())
