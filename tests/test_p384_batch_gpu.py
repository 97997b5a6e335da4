"""GPU: the P-384 BatchVerify entry points (bh_verify384_compact,
bh_batch_verify384_ptrs and their _submit forms: k384_keys_prep, the indexed
k384_prep / k384_plan, the grouping by key index, shards over the devices and
the two pipeline slots per device) against bh_verify(BH_CURVE_P384) on the
expanded batch and against the reasons the records were built to get. Every
test leaves the registry empty."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from oracle import ecdsa_ref as O
from tests import p384_batch_util as B
from tests import p384_util as U
from tests.conftest import ROOT, pack

pytestmark = pytest.mark.gpu
SHA2, SHA3, NLS, BK = (_lib.BH_F_HASH_SHA256, _lib.BH_F_HASH_SHA3_256, _lib.BH_F_NO_LOW_S,
                       _lib.BH_F_BATCH_KEYS)
OFF_CURVE = bytes(95) + b"\x01"
X_GE_P = b"\xff" * 48 + bytes(48)


@pytest.fixture(scope="module")
def L():
    _lib.ensure_init()
    lib = _lib.lib()
    _lib.check(lib.bh_keys384_clear(-1))
    yield lib
    _lib.check(lib.bh_keys384_clear(-1))


@pytest.fixture(scope="module")
def signed():
    """signed_batch(600, 24) per hash family, made once and never changed."""
    lc = U.LibCrypto()
    return {f: U.signed_batch(lc, 600, 24, seed=600, family=f) for f in ("SHA2", "SHA3")}


def expect(recs, no_low_s):
    return np.array([r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]
                     for r in recs], np.uint8)


def signed_want(want, no_low_s):
    # a high-S record is the valid signature (r, n - s): without the rule it verifies
    return np.where(want == O.R_HIGH_S, O.R_OK, want).astype(np.uint8) if no_low_s else want


def parity(L, recs, fused, hash_flag, want_of):
    """Both synchronous entry points, the compact one with and without key
    indices, over the four flag combinations."""
    forms = [("compact", B.compact(recs, fused, seed=384, extra=(OFF_CURVE, X_GE_P))),
             ("compact, key_idx NULL", B.compact(recs, fused, indexed=False)),
             ("ptrs", B.ptrs(recs, fused))]
    for nls in (0, NLS):
        want = want_of(bool(nls))
        for bk in (0, BK):
            flags = hash_flag | nls | bk
            ref_r, ref_b = B.run_expanded(L, recs, fused, flags)
            assert (ref_r == want).all()
            for name, form in forms:
                run = B.run_ptrs if name == "ptrs" else B.run_compact
                rs, bits = run(L, form, flags)
                bad = [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(rs, want)) if g != w]
                assert not bad, (name, flags, bad[:8])
                assert (rs == ref_r).all() and (bits == ref_b).all(), (name, flags)
                assert (bits == (want == O.R_OK)).all(), (name, flags)


def test_parity_golden_digest(L):
    recs = U.load_golden384()
    parity(L, recs, False, 0, lambda n: expect(recs, n))


@pytest.mark.parametrize("family,flag", [("SHA2", SHA2), ("SHA3", SHA3)])
def test_parity_golden_fused(L, family, flag):
    recs = [r for r in U.load_golden384() if r.get("family") == family]
    assert len(recs) >= 11
    parity(L, recs, True, flag, lambda n: expect(recs, n))


@pytest.mark.parametrize("mode", ["digest", "SHA2", "SHA3"])
def test_parity_signed(L, signed, mode):
    recs, want = signed["SHA2" if mode == "digest" else mode]
    flag = {"digest": 0, "SHA2": SHA2, "SHA3": SHA3}[mode]
    parity(L, recs, mode != "digest", flag, lambda n: signed_want(want, n))


@pytest.mark.parametrize("stride", [48, 32])
def test_fixed_stride_digests(L, stride):
    """msg_len = NULL: every digest msg_stride bytes."""
    recs = [r for r in U.load_golden384() if len(r["digest"]) == 2 * stride]
    assert len(recs) >= 90
    for flags in (0, NLS | BK):
        want = expect(recs, bool(flags & NLS))
        ref_r, ref_b = B.run_expanded(L, recs, False, flags)
        for indexed in (True, False):
            cb = B.compact(recs, False, indexed=indexed, seed=7, stride=stride)
            assert cb.c.msg_len is None and cb.c.msg_stride == stride
            rs, bits = B.run_compact(L, cb, flags)
            assert (rs == want).all() and (rs == ref_r).all() and (bits == ref_b).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_sizes(L, signed, n):
    recs, want = signed["SHA2"]
    recs, want = recs[:n], want[:n]
    for flags in (SHA2, SHA2 | BK):
        for name, form in (("compact", B.compact(recs, True, seed=n)), ("ptrs", B.ptrs(recs, True))):
            rs, bits = (B.run_ptrs if name == "ptrs" else B.run_compact)(L, form, flags)
            assert (rs == want).all() and (bits == (want == O.R_OK)).all(), (name, n, flags)
    if n:
        ref_r, ref_b = B.run_expanded(L, recs, True, SHA2)
        assert (ref_r == want).all()


CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from bdls_amd import _lib
from oracle import ecdsa_ref as O
from tests import p384_batch_util as B, p384_util as U
_lib.ensure_init()
L = _lib.lib()
recs, want = U.signed_batch(U.LibCrypto(), 600, 24, seed=600, family="SHA2")
# a key used in every shard (key 0's) and one used only in the last (a 25th key's)
last = U.signed_batch(U.LibCrypto(), 8, 1, seed=77, family="SHA2")
recs = recs[:592] + [r for r in last[0]]
want = np.concatenate([want[:592], last[1]])
out = {}
for name, form, run in (("compact", B.compact(recs, True, seed=3), B.run_compact),
                        ("ptrs", B.ptrs(recs, True), B.run_ptrs)):
    for flags in (1, 1 | 128):
        b0 = _lib.device_stats()
        rs, bits = run(L, form, flags)
        b1 = _lib.device_stats()
        out["%%s %%d" %% (name, flags)] = [bool((rs == want).all()),
                                          bool((bits == (want == 0)).all()),
                                          b1[0] - b0[0], b1[1] - b0[1]]
ref_r, ref_b = B.run_expanded(L, recs, True, 1)
out["ref"] = bool((ref_r == want).all())
keys = [B.key_bytes(r) for r in recs]
out["last_only"] = keys[599] not in keys[:384] and keys[599] in keys[384:]
out["everywhere"] = all(keys[0] in keys[a:b] for a, b in ((0, 192), (192, 384), (384, 600)))
print(json.dumps(out))
"""


def test_shards_and_chunks_child_process():
    """BH_P384_CHUNK=64 BH_HOST_SHARDS=3 (both read once per process): 600
    records in three shards of 192, 192 and 216, three or four chunks each."""
    env = dict(os.environ, BH_P384_CHUNK="64", BH_HOST_SHARDS="3")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop("ref") and out.pop("last_only") and out.pop("everywhere")
    assert len(out) == 4
    for k, v in out.items():
        assert v == [True, True, 1, 600], (k, v)   # one batch per call for bh_device_stats


def test_jobs_reverse_order(L, signed, golden):
    """Four P-384 jobs through the two _submit forms and one P-256 job between
    them, waited in reverse order."""
    recs, want = signed["SHA2"]
    gold = U.load_golden384()
    parts = [(B.compact(recs[:300], True, seed=1), SHA2 | BK, want[:300]),
             (B.ptrs(recs[300:], True), SHA2, want[300:]),
             (B.compact(gold, False, indexed=False), 0, expect(gold, False)),
             (B.ptrs(gold, False), NLS | BK, expect(gold, True))]
    jobs = []
    for k, (form, flags, _) in enumerate(parts):
        bm, rs = B.outputs(form.n)
        job = ctypes.c_void_p()
        if isinstance(form, B.Ptrs):
            rc = L.bh_batch_verify384_ptrs_submit(ctypes.byref(form.p), form.n, flags,
                                                  bm.ctypes.data, rs.ctypes.data, ctypes.byref(job))
        else:
            rc = L.bh_verify384_compact_submit(ctypes.byref(form.c), form.n, flags, bm.ctypes.data,
                                               rs.ctypes.data, ctypes.byref(job))
        _lib.check(rc)
        assert job.value
        jobs.append((job, bm, rs, form.n))
        if k == 1:   # a P-256 job in flight among them
            g = golden
            arrs = pack(g, False)
            b = _lib.BhBatch(*[a.ctypes.data for a in arrs])
            bm6, rs6 = B.outputs(len(g))
            j6 = ctypes.c_void_p()
            _lib.check(L.bh_verify_submit(0, ctypes.byref(b), len(g), 0, bm6.ctypes.data,
                                          rs6.ctypes.data, ctypes.byref(j6)))
            p256 = (j6, bm6, rs6, len(g), arrs, np.array([r["reason"] for r in g], np.uint8))
    for (job, bm, rs, n), (_, _, want_k) in reversed(list(zip(jobs, parts))):
        _lib.check(L.bh_verify_wait(job))   # frees the job: once each
        got, bits = B.check_out(bm, rs, n)
        assert (got == want_k).all() and (bits == (want_k == O.R_OK)).all()
    j6, bm6, rs6, n6, _, want6 = p256
    _lib.check(L.bh_verify_wait(j6))
    got, bits = B.check_out(bm6, rs6, n6)
    assert (got == want6).all() and (bits == (want6 == O.R_OK)).all()


def test_empty_submit_returns_a_job(L):
    cb = B.compact([], False)
    job = ctypes.c_void_p()
    _lib.check(L.bh_verify384_compact_submit(ctypes.byref(cb.c), 0, 0, None, None,
                                             ctypes.byref(job)))
    assert job.value
    _lib.check(L.bh_verify_wait(job))
    pb = B.ptrs([], False)
    _lib.check(L.bh_batch_verify384_ptrs_submit(ctypes.byref(pb.p), 0, 0, None, None,
                                                ctypes.byref(job)))
    assert job.value
    _lib.check(L.bh_verify_wait(job))


def test_registry_half_the_keys(L, signed):
    recs, want = signed["SHA2"]
    table, _ = B.key_table(recs)
    half = [k for k in table if O.on_curve(U.P384, int.from_bytes(k[:48], "big"),
                                              int.from_bytes(k[48:], "big"))][::2]
    assert len(half) >= 10
    buf = np.frombuffer(b"".join(half), np.uint8)
    st = np.full(len(half), 255, np.uint8)
    try:
        _lib.check(L.bh_keys384_register(-1, buf.ctypes.data, len(half), st.ctypes.data))
        assert (st == 0).all()
        for flags in (SHA2, SHA2 | BK):
            for form, run in ((B.compact(recs, True, seed=9), B.run_compact),
                              (B.compact(recs, True, indexed=False), B.run_compact),
                              (B.ptrs(recs, True), B.run_ptrs)):
                rs, bits = run(L, form, flags)
                assert (rs == want).all() and (bits == (want == O.R_OK)).all(), flags
    finally:
        _lib.check(L.bh_keys384_clear(-1))
    cnt = ctypes.c_size_t(99)
    _lib.check(L.bh_keys384_count(0, ctypes.byref(cnt)))
    assert cnt.value == 0


def test_null_pointers_and_released_buffers(L, signed):
    """The staged form's NULL pointers, and the caller's buffers overwritten
    between the submit call's return and the wait."""
    lc = U.LibCrypto()
    recs, want = signed["SHA2"]
    recs, want = recs[:64], want[:64].copy()
    keys = [B.key_bytes(r) for r in recs]
    for fused, flags in ((True, SHA2), (False, 0)):
        sigs, msgs = B.fields(recs, fused)
        w = want.copy()
        keys2, sigs2, msgs2 = list(keys), list(sigs), list(msgs)
        sigs2[1], w[1] = None, O.R_EMPTY_SIG
        keys2[2], w[2] = None, O.R_BAD_KEY
        msgs2[4] = None
        if fused:   # the hash of the empty message, signed so: verifies
            d = 4242
            qx, qy = O.pubkey(U.P384, d)
            k = lc.key(d, qx, qy)
            r_, s_ = lc.sign(k, U.family_hash("SHA2", b""))
            lc.free_key(k)
            keys2[4] = qx.to_bytes(48, "big") + qy.to_bytes(48, "big")
            sigs2[4] = O.marshal_ecdsa_signature(r_, min(s_, U.N - s_))
            w[4] = O.R_OK
        else:
            w[4] = O.R_EMPTY_DIGEST
        sigs2[5], keys2[5], w[5] = None, None, O.R_EMPTY_SIG   # precedence: the signature first
        pb = B.Ptrs(keys2, sigs2, msgs2)
        rs, bits = B.run_ptrs(L, pb, flags)
        assert (rs == w).all() and (bits == (w == O.R_OK)).all(), (fused, rs[:8], w[:8])
        bm, out = B.outputs(pb.n)
        job = ctypes.c_void_p()
        _lib.check(L.bh_batch_verify384_ptrs_submit(ctypes.byref(pb.p), pb.n, flags | BK,
                                                    bm.ctypes.data, out.ctypes.data,
                                                    ctypes.byref(job)))
        pb.scribble()
        _lib.check(L.bh_verify_wait(job))
        got, bits = B.check_out(bm, out, pb.n)
        assert (got == w).all() and (bits == (w == O.R_OK)).all()
