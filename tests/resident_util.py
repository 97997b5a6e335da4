"""Test-side plumbing for the multi-pass and deferred-timing paths of
bh_verify_dev (tests/test_resident_passes_gpu.py, tests/test_resident_passes_cpu.py).

* the batches: the fixture tests/golden/p384_vectors.jsonl (the oracle's
  expectations) and the by-construction batches of tests/p384_util.py and
  tests/sha2wide_util.py, each put to oracle/ecdsa_ref.py on every corrupted
  record and every 16th other one. Built once per process, never changed.
* Resident / Outputs / dev_call: one bh_verify_dev call on a device-resident
  batch into guarded outputs -- one bitmap word and 64 reason bytes more than
  the call may write, everything prefilled with a pattern that is neither 0 nor
  a reason code.
* run_plan / child_main: a list of such calls run in order; a child process
  (BH_P384_CHUNK is parsed once per process) runs a plan file and prints one
  JSON line. The child only runs calls: every expectation stays with the parent.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np

from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests import sha2wide_util as W

ROOT = U.ROOT
GUARD = 0xA5  # not BH_R_OK .. BH_R_UNSUPPORTED, not 252 .. 255
GUARD_WORD = 0xA5A5A5A5A5A5A5A5
CHUNK = 64  # BH_P384_CHUNK of the child processes
TIMING_FIELDS = ("prep_ms", "inv_ms", "plan_ms", "build_ladder_ms", "publish_ms", "keycomb_ms",
                 "n_keycomb", "n_ladder", "n_keytables", "wide")
P384_PREFIXES = (1, 64, 65, 128, 129)  # and the whole fixture
FAMILY_FLAG = {"SHA2": 1, "SHA3": 8}  # BH_F_HASH_SHA256, BH_F_HASH_SHA3_256
BH_F_NO_LOW_S, BH_F_KEEP_KEYS, BH_F_ANY_LANE = 2, 4, 16


# ---------------------------------------------------------------- expectations
def oracle_reason(curve: O.Curve, rec, no_low_s=False) -> int:
    """BH_R_* of one record from oracle/ecdsa_ref.py, with or without Fabric's low-S rule."""
    qx, qy = int(rec["qx"], 16), int(rec["qy"], 16)
    sig, dg = bytes.fromhex(rec["sig"]), bytes.fromhex(rec["digest"])
    if not no_low_s:
        return O.csp_verify(curve, qx, qy, sig, dg)[1]
    reason, r, s = O.unmarshal_ecdsa_signature(sig)
    return reason if reason != O.R_OK else O.go_ecdsa_verify(curve, qx, qy, dg, r, s)


def spot_check(curve: O.Curve, recs, want, digest_of, nls=None):
    """Every corrupted record (one in eight, i % 8 == 3) and every 16th other
    one against the oracle; the digest field against hashlib."""
    for i, r in enumerate(recs):
        if i % 8 != 3 and i % 16 != 0:
            continue
        assert bytes.fromhex(r["digest"]) == digest_of(bytes.fromhex(r["msg"])), i
        assert oracle_reason(curve, r) == want[i], i
        if nls is not None:
            assert oracle_reason(curve, r, True) == nls[i], i


def count_math(want) -> int:
    """Records that reach the group equation: expected reason BH_R_OK or BH_R_MATH."""
    want = np.asarray(want)
    return int((want == O.R_OK).sum() + (want == O.R_MATH).sum())


def bits_of(words, n: int):
    """Bits [0, n) of LSB-first uint64 bitmap words."""
    w = np.array([int(x) for x in words], np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


@functools.lru_cache(maxsize=None)
def golden384():
    """(records, reasons, reasons without low-S) of the P-384 fixture."""
    recs = U.load_golden384()
    assert 150 <= len(recs) <= 210  # 3 or 4 passes of 64
    want = np.array([r["reason"] for r in recs], np.uint8)
    nls = np.array([r.get("reason_no_low_s", r["reason"]) for r in recs], np.uint8)
    return recs, want, nls


@functools.lru_cache(maxsize=None)
def p384_fused(family: str):
    """The first 200 records (passes of 64, 64, 64, 8) of the libcrypto-signed
    batch tests/test_p384_gpu.py runs whole, and their reasons by construction."""
    recs, want = U.signed_batch(U.LibCrypto(), 600, 24, seed=600, family=family)
    recs, want = recs[:200], want[:200]
    spot_check(U.P384, recs, want, lambda m: U.family_hash(family, m))
    assert (want != 0).sum() == 25
    return recs, want


@functools.lru_cache(maxsize=None)
def wide_batch(curve: str, h: str, n: int):
    """sha2wide_util.signed_batch(curve, h, n=n, nkeys=12): (records, reasons,
    reasons without low-S). The 12 edge lengths cycle, so every run of 64
    records hashes every padding edge."""
    lc = W.LibCrypto() if curve == "P-384" else None
    recs, want, nls = W.signed_batch(curve, h, lc, n=n, nkeys=12)
    spot_check(W.CURVES[curve][0], recs, want, lambda m: W.HASHES[h][0](m).digest(), nls)
    assert (want != 0).sum() == len(range(3, n, 8)) and (nls != want).any()
    return recs, want, nls


def pack(recs, mode: str):
    """SoA arrays of records: mode "digest" (the digest field) or "msg"."""
    return U.pack384(recs, False) if mode == "digest" else W.pack_records(recs)


# ---------------------------------------------------------------- the plans
def dev_op(op_id, batch, mode, curve, n, flags, timing):
    return {"op": "dev", "id": op_id, "batch": batch, "mode": mode, "curve": curve, "n": n,
            "flags": flags, "timing": bool(timing)}


def plan_p384():
    """Section 1: resident P-384 in passes of 64. Returns (batches, ops, expect)
    with expect[id] = (n, reasons, timed)."""
    recs, want, nls = golden384()
    batches = {"golden": recs, "golden_rev": recs[::-1]}
    ops, expect = [], {}
    for no_low_s in (0, 1):
        for n in P384_PREFIXES + (len(recs),):
            for timed in (0, 1):
                op_id = f"digest/nls{no_low_s}/n{n}/t{timed}"
                ops.append(dev_op(op_id, "golden", "digest", U.BH_CURVE_P384, n,
                                  BH_F_NO_LOW_S if no_low_s else 0, timed))
                expect[op_id] = (n, (nls if no_low_s else want)[:n], timed)
    for fam in ("SHA2", "SHA3"):
        frecs, fwant = p384_fused(fam)
        batches[fam] = frecs
        for timed in (0, 1):
            op_id = f"fused/{fam}/t{timed}"
            ops.append(dev_op(op_id, fam, "msg", U.BH_CURVE_P384, len(frecs), FAMILY_FLAG[fam],
                              timed))
            expect[op_id] = (len(frecs), fwant, timed)
    ops.append({"op": "async_pair", "id": "async", "batches": ["golden", "golden_rev"],
                "mode": "digest", "curve": U.BH_CURVE_P384, "flags": 0})
    expect["async/0"] = (len(recs), want, 0)
    expect["async/1"] = (len(recs), want[::-1], 0)
    return batches, ops, expect


def plan_wide():
    """Section 2: P-384 with SHA-384 / SHA-512 resident, P-256 with SHA-512
    through bh_verify, all in passes of 64."""
    batches, ops, expect = {}, [], {}
    for h in ("SHA384", "SHA512"):
        recs, want, nls = wide_batch("P-384", h, 200)
        batches[h] = recs
        for extra, exp in ((0, want), (BH_F_NO_LOW_S | BH_F_KEEP_KEYS | BH_F_ANY_LANE, nls)):
            for timed in (0, 1):
                op_id = f"wide/{h}/f{extra}/t{timed}"
                ops.append(dev_op(op_id, h, "msg", W.BH_CURVE_P384, len(recs),
                                  W.HASHES[h][1] | extra, timed))
                expect[op_id] = (len(recs), exp, timed)
    recs, want, _ = wide_batch("P-256", "SHA512", 200)
    batches["P256"] = recs
    ops.append({"op": "host", "id": "host/P256/SHA512", "batch": "P256", "mode": "msg",
                "curve": W.BH_CURVE_P256, "flags": W.BH_F_HASH_SHA512})
    expect["host/P256/SHA512"] = (len(recs), want, 0)
    return batches, ops, expect


# ---------------------------------------------------------------- device side
class Resident:
    """A batch uploaded to device 0 once; prefixes of it share the pointers."""

    def __init__(self, arrs, device=0):
        from bdls_amd import _lib
        self.dev = [_lib.DeviceArray.from_numpy(device, a) for a in arrs]
        self.batch = _lib.BhBatch(*[d.ptr for d in self.dev])

    def free(self):
        for d in self.dev:
            d.free()


class Outputs:
    """ceil(n/64) + 1 bitmap words and n + 64 reason bytes, all prefilled with GUARD."""

    def __init__(self, n, device=0):
        from bdls_amd import _lib
        self.n, self.nw = n, (n + 63) // 64
        self.bm = _lib.DeviceArray.from_numpy(device, np.full(self.nw + 1, GUARD_WORD, np.uint64))
        self.rs = _lib.DeviceArray.from_numpy(device, np.full(n + 64, GUARD, np.uint8))

    def read(self):
        words = self.bm.to_numpy(np.uint64, self.nw + 1)
        reason = self.rs.to_numpy(np.uint8, self.n + 64)
        self.bm.free()
        self.rs.free()
        return {"reason": reason[:self.n].tolist(), "words": [int(x) for x in words[:self.nw]],
                "guard_word": int(words[self.nw]),
                "guard_bytes": sorted(set(reason[self.n:].tolist()))}


def timing_dict(t):
    return {f: getattr(t, f) for f in TIMING_FIELDS}


def dev_call(res: Resident, curve, n, flags, timing=False, sync=1, out=None):
    """bh_verify_dev on the first n records of res into guarded outputs: fresh
    ones, read back, or the caller's `out`, left on the device (a call that is
    not waited for). Returns them with the bh_timing and the movement of
    bh_device_stats."""
    from bdls_amd import _lib
    read = out is None
    out = out or Outputs(n)
    t = _lib.BhTiming() if timing else None
    s0 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify_dev(0, curve, ctypes.byref(res.batch), n, flags, out.bm.ptr,
                                        out.rs.ptr, None, sync, ctypes.byref(t) if t else None))
    s1 = _lib.device_stats()
    got = out.read() if read else {"outputs": out}
    got["timing"] = timing_dict(t) if t else None
    got["stats"] = [s1[0] - s0[0], s1[1] - s0[1]]
    return got


def host_call(arrs, curve, n, flags):
    """bh_verify on host arrays; the bitmap as words like the device API's."""
    from bdls_amd import _lib
    bm = np.zeros(8 * ((n + 63) // 64), np.uint8)
    rs = np.full(n, GUARD, np.uint8)
    b = _lib.BhBatch(*[a.ctypes.data for a in arrs])
    s0 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify(curve, ctypes.byref(b), n, flags, bm.ctypes.data,
                                    rs.ctypes.data))
    s1 = _lib.device_stats()
    return {"reason": rs.tolist(), "words": [int(x) for x in bm.view(np.uint64)],
            "guard_word": GUARD_WORD, "guard_bytes": [GUARD], "timing": None,
            "stats": [s1[0] - s0[0], s1[1] - s0[1]]}


def run_plan(batches, ops):
    """Runs the calls of a plan in order on device 0; stops at the first failure."""
    from bdls_amd import _lib
    _lib.ensure_init()
    resident, out = {}, {}

    def res(name, mode):
        if (name, mode) not in resident:
            resident[name, mode] = Resident(pack(batches[name], mode))
        return resident[name, mode]

    for op in ops:
        if op["op"] == "dev":
            out[op["id"]] = dev_call(res(op["batch"], op["mode"]), op["curve"], op["n"],
                                     op["flags"], op["timing"])
        elif op["op"] == "async_pair":
            # two calls queued one after the other, each with its own outputs, one wait
            # (inputs and outputs are on the device before the first call: the
            # library's copies are synchronous and would wait for it)
            ins = [res(name, op["mode"]) for name in op["batches"]]
            outs = [Outputs(len(batches[name])) for name in op["batches"]]
            pending = [dev_call(r, op["curve"], o.n, op["flags"], sync=0, out=o)
                       for r, o in zip(ins, outs)]
            _lib.check(_lib.lib().bh_sync(0))
            for k, got in enumerate(pending):
                got.update(got.pop("outputs").read())
                out[f"{op['id']}/{k}"] = got
        elif op["op"] == "host":
            recs = batches[op["batch"]]
            out[op["id"]] = host_call(pack(recs, op["mode"]), op["curve"], len(recs), op["flags"])
        else:
            raise ValueError(op["op"])
    for r in resident.values():
        r.free()
    return out


def child_main(path):
    with open(path) as f:
        plan = json.load(f)
    print(json.dumps(run_plan(plan["batches"], plan["ops"])))


def run_child(batches, ops, tmp_dir, chunk=CHUNK, timeout=120):
    """A fresh process with BH_P384_CHUNK=chunk runs the plan; its results."""
    path = os.path.join(str(tmp_dir), "plan.json")
    with open(path, "w") as f:
        json.dump({"batches": batches, "ops": ops}, f)
    code = ("import sys\n"
            "sys.path.insert(0, '.')\n"
            "from tests import resident_util\n"
            f"resident_util.child_main({path!r})\n")
    env = dict(os.environ, BH_P384_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_result(got, n, want, op_id=None):
    """Reasons, bits [0, n) and both guards of one call's results."""
    want = np.asarray(want, np.uint8)
    bad = [(i, g, int(w)) for i, (g, w) in enumerate(zip(got["reason"], want)) if g != w]
    assert len(got["reason"]) == n and not bad, (op_id, bad[:8])
    assert len(got["words"]) == (n + 63) // 64, op_id
    wrong = np.nonzero(bits_of(got["words"], n) != (want == 0))[0]
    assert wrong.size == 0, (op_id, wrong[:8].tolist())
    assert got["guard_word"] == GUARD_WORD, (op_id, hex(got["guard_word"]))
    assert got["guard_bytes"] == [GUARD], (op_id, got["guard_bytes"])
