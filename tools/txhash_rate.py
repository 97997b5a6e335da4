#!/usr/bin/env python3
"""What CheckTxID and the proposal hash cost on the device, beside the host.

  python tools/txhash_rate.py [--parent-lib PATH] [--calls 200] [--out profiles/txhash/block.json]

On config 3's block (generate_fabric_block(): 500 endorser transactions), warm
(BH_FAB_F_KEEP_KEYS after warm-up calls), `--calls` alternating calls each of
  a1, a2  bh_fabric_block_preverify of the PARENT commit's library (--parent-lib:
          a libbdlship.so built from the parent commit), two child processes --
          what two series of the same code show against each other on this box
  b       bh_fabric_block_preverify of this build     } one child process
  c       bh_fabric_block_prevalidate of this build   }
every library in a child process of its own (BDLS_HIP_LIB), called in turn
a1, b, c, a2, ... so drift lands on all of them alike. Then
  d       the same 1,000 messages (nonce || creator, and channel_header ||
          action header || chaincode proposal payload, of every transaction)
          hashed and compared with hashlib on ONE thread of this host
  kernel  bh_hash_dev on 2^20 resident 256-byte one-span messages per
          algorithm, between device events on the call's stream, synchronised.
Rules (exit status 1 when the first fails): p50(b) lies within what a1 and a2
show against each other (p50(b) <= max(p50(a1), p50(a2)) + |p50(a1) - p50(a2)|);
(c) - (b) is written beside (d). No torch; bench.py is not involved.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return {"p50": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "p10": round(xs[len(xs) // 10], 4), "p90": round(xs[(9 * len(xs)) // 10], 4), "n": len(xs)}


# ---------------------------------------------------------------- child: one library, calls on demand
def child() -> int:
    from bdls_amd import _lib
    from bdls_amd.workload import fabric as F
    L = ctypes.CDLL(_lib.LIB_PATH)  # (a parent build lacks the new symbols: bind by hand)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bh_init.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.bh_fabric_block_preverify.argtypes = [vp, sz, ctypes.c_uint32, vp, sz, ctypes.POINTER(sz), vp,
                                            sz, ctypes.POINTER(sz)]
    assert L.bh_init(1, 0) == 0
    fb = F.generate_fabric_block()
    buf = np.frombuffer(fb.block + b"\0", np.uint8)
    ntx, nend, nref = sz(), sz(), sz()
    txs = (_lib.BhFabTx * fb.ntx)()
    cap = sum(len(e) for e in fb.tx_endorse) + 64 * fb.ntx
    end = np.zeros(cap, np.uint8)
    hs = (_lib.BhFabTxhash * fb.ntx)()
    flags = _lib.BH_FAB_F_KEEP_KEYS
    have_c = hasattr(L, "bh_fabric_block_prevalidate")
    if have_c:
        L.bh_fabric_block_prevalidate.argtypes = [vp, sz, ctypes.c_uint32, vp, sz, ctypes.POINTER(sz),
                                                  vp, sz, ctypes.POINTER(sz), vp, sz,
                                                  ctypes.POINTER(sz), vp]

    def old():
        return L.bh_fabric_block_preverify(buf.ctypes.data, len(fb.block), flags, txs, fb.ntx,
                                           ctypes.byref(ntx), end.ctypes.data, cap, ctypes.byref(nend))

    def new():
        return L.bh_fabric_block_prevalidate(buf.ctypes.data, len(fb.block), flags, txs, fb.ntx,
                                             ctypes.byref(ntx), end.ctypes.data, cap,
                                             ctypes.byref(nend), None, 0, ctypes.byref(nref), hs)
    for _ in range(5):
        assert old() == 0
        if have_c:
            assert new() == 0
    if have_c:  # parity of the new call before it is timed
        assert [t.status for t in txs[:fb.ntx]] == fb.tx_status_full
        assert [(h.txid, h.proposal_hash) for h in hs] == fb.tx_hash
    print("ready", flush=True)
    for line in sys.stdin:
        fn = {"old": old, "new": new}.get(line.strip())
        if fn is None:
            break
        t = time.perf_counter()
        rc = fn()
        ms = (time.perf_counter() - t) * 1e3
        print(f"{ms:.5f}" if rc == 0 else "err", flush=True)
    return 0


class Child:
    def __init__(self, lib_path: str):
        env = dict(os.environ, BDLS_HIP_LIB=lib_path)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self.p.stdout.readline().strip() == "ready", lib_path

    def call(self, which: str) -> float:
        self.p.stdin.write(which + "\n")
        self.p.stdin.flush()
        return float(self.p.stdout.readline())

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait(timeout=60)


# ---------------------------------------------------------------- d: the host's hashing
def host_hashing(reps: int = 50):
    from bdls_amd import fabric
    from bdls_amd.workload import fabric as F
    fb = F.generate_fabric_block()
    block = fb.block
    hashes = fabric.block_prevalidate(block, decode_only=True)[3]
    sp = lambda s: block[s[0]:s[0] + s[1]]  # noqa: E731
    recs = []
    for h in hashes:
        s = h.spans
        if s["nonce"][1]:
            recs.append(((sp(s["nonce"]), sp(s["creator"])), sp(s["txid"]), True))
        if s["ccpp"][1]:
            recs.append(((sp(s["chdr"]), sp(s["ashdr"]), sp(s["ccpp"])), sp(s["phash"]), False))
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        ok = 0
        for parts, want, hexed in recs:
            h = hashlib.sha256()
            for p in parts:
                h.update(p)
            ok += (h.hexdigest().encode() if hexed else h.digest()) == want
        ms.append((time.perf_counter() - t) * 1e3)
    nbytes = sum(sum(len(p) for p in parts) for parts, _, _ in recs)
    return {"what": "hashlib.sha256 over the same messages, hex / bytes compare, ONE thread of this "
                    "host", "messages": len(recs), "bytes": nbytes, "matching": ok,
            "compressions": sum((sum(len(p) for p in parts) + 9 + 63) // 64 for parts, _, _ in recs),
            "ms": stats(ms)}


# ---------------------------------------------------------------- the kernels alone
def kernel_rate(n: int = 1 << 20, msg_len: int = 256, steps: int = 10):
    from bdls_amd import _lib
    _lib.ensure_init(1)
    L = _lib.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    s, e0, e1 = vp(), vp(), vp()
    assert hip.hipSetDevice(0) == 0 and hip.hipStreamCreate(ctypes.byref(s)) == 0
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    data = np.random.default_rng(1).integers(0, 256, n * msg_len + 8, dtype=np.uint8)
    d_data = _lib.DeviceArray.from_numpy(0, data)
    d_off = _lib.DeviceArray.from_numpy(0, np.arange(n, dtype=np.uint64) * msg_len)
    d_len = _lib.DeviceArray.from_numpy(0, np.full(n, msg_len, np.uint32))
    d_dig = _lib.DeviceArray(0, n * 32)
    b = _lib.BhHBatch(d_data.ptr, n * msg_len, d_off.ptr, d_len.ptr, 1, None, None, None)
    out = {}
    for name, alg, fn in (("sha256", _lib.BH_HASH_SHA256, hashlib.sha256),
                          ("sha3_256", _lib.BH_HASH_SHA3_256, hashlib.sha3_256)):
        ms = []
        for it in range(3 + steps):
            assert hip.hipEventRecord(e0, s) == 0
            _lib.check(L.bh_hash_dev(0, alg, ctypes.byref(b), n, d_dig.ptr, None, s, 0))
            assert hip.hipEventRecord(e1, s) == 0 and hip.hipEventSynchronize(e1) == 0
            t = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
            if it >= 3:
                ms.append(t.value)
        dig = d_dig.to_numpy(np.uint8, n * 32).reshape(n, 32)
        idx = [0, 1, n // 2, n - 1]
        ok = all(dig[i].tobytes() == fn(data[i * msg_len:(i + 1) * msg_len].tobytes()).digest()
                 for i in idx)
        st = stats(ms)
        out[name] = {"ms": st, "digests_per_s": n / (st["p50"] * 1e-3),
                     "gb_per_s": n * msg_len / (st["p50"] * 1e-3) / 1e9, "sample_parity": ok}
    for d in (d_data, d_off, d_len, d_dig):
        d.free()
    return {"what": f"bh_hash_dev, {n} resident {msg_len}-byte one-span messages, digests out, "
                    "between device events on the call's stream", "n": n, "msg_len": msg_len, **out}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txhash", "block.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    from bdls_amd import _lib
    from bdls_amd.provenance import kernel_src_sha
    series = {"b": [], "c": []}
    new = Child(_lib.LIB_PATH)
    parents = []
    if a.parent_lib:
        parents = [Child(os.path.abspath(a.parent_lib)), Child(os.path.abspath(a.parent_lib))]
        series.update({"a1": [], "a2": []})
    for _ in range(max(200, a.calls)):
        if parents:
            series["a1"].append(parents[0].call("old"))
        series["b"].append(new.call("old"))
        series["c"].append(new.call("new"))
        if parents:
            series["a2"].append(parents[1].call("old"))
    for c in [new] + parents:
        c.close()
    st = {k: stats(v) for k, v in series.items()}
    d = host_hashing()
    kern = kernel_rate()
    c_minus_b = round(st["c"]["p50"] - st["b"]["p50"], 4)
    verdict = {"c_minus_b_ms": c_minus_b, "d_ms_one_thread": d["ms"]["p50"],
               "d_div16_ms": round(d["ms"]["p50"] / 16, 4),
               "d_div16_note": "an extrapolation (d / 16), not a measurement: one thread was measured",
               "device_checks_cost_more_than_d": bool(c_minus_b > d["ms"]["p50"])}
    ok = True
    if parents:
        pa, pb = st["a1"]["p50"], st["a2"]["p50"]
        verdict.update({"a_spread_ms": round(abs(pa - pb), 4),
                        "b_rule": "p50(b) <= max(p50(a1), p50(a2)) + |p50(a1) - p50(a2)|",
                        "b_within_a_spread": bool(st["b"]["p50"] <= max(pa, pb) + abs(pa - pb))})
        ok = verdict["b_within_a_spread"]
    out = {"what": "config 3's block (500 transactions), warm, alternating calls; ms per call",
           "calls_per_series": max(200, a.calls),
           "series": {"a1": "parent library, bh_fabric_block_preverify",
                      "a2": "parent library, bh_fabric_block_preverify (second process)",
                      "b": "this build, bh_fabric_block_preverify",
                      "c": "this build, bh_fabric_block_prevalidate"},
           "ms": st, "host_hashing_d": d, "verdict": verdict, "kernel": kern,
           "parent_lib": bool(parents), "kernel_src_sha": kernel_src_sha(),
           "version": _lib.lib().bh_version().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
