"""GPU: the per-batch comb tables built with sign-paired entries (verify.h
lltab_build: k_ktab_ladder's build lanes, k_reg_win's LDS-scratch build) read
by k_keycomb, at the smallest shapes that take the one-lane comb route.

  (a) P-256, 40,960 records with fused SHA-256: generator records on keys used
      4 to 16 times (1/16 corrupted), plus one key with 64 records whose
      signatures are chosen so that their u2 = r / s -- recoded as verify.h
      ll_slices / ll_column do -- read every entry index of the key's table
      with both signs (asserted in Python before the device call).
  (b) a secp256k1 BDLS batch just above 32,768 records through the comb.
  (c) 57 keys registered (k_reg_win), then a 2,000-record batch of those keys
      (the slots' affine windows) and a 40,960-record one (the slots' combs).
Bitmap and reasons equal the generator's expectation and, for the chosen
records, the C oracle; every record that reaches the group equation went
through the key tables.
"""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

from bdls_amd import _lib, workload
from oracle import ecdsa_ref as O
from oracle import orc
from tests.test_gpu_comb import _dev_verify

pytestmark = pytest.mark.gpu
T, S = 7, 37  # the comb's shape (verify.h BH_LL_T; tests/test_lltab_cpu.py checks it on the build)


@pytest.fixture(scope="module")
def L():
    _lib.ensure_init()
    return _lib.lib()


def comb_reads(u2, n, t=T, s=S):
    """{(entry index, negated)} that the signed comb reads for the scalar u2
    (verify.h ll_slices / ll_column)"""
    k = u2 if u2 & 1 else u2 + n
    c = (k >> 1) | (1 << (t * s - 1))
    out = set()
    for j in range(s):
        bits = [(c >> (s * i + j)) & 1 for i in range(t)]
        m = sum(b << i for i, b in enumerate(bits[:-1]))
        neg = bits[-1] == 0
        out.add(((~m & ((1 << (t - 1)) - 1)) if neg else m, neg))
    return out


def chosen_records(c, seed):
    """64 records of one key: (pub64, sig, msg, reason by the C oracle); nonces
    are taken while they add (entry, sign) pairs the records so far never read."""
    rng = random.Random(seed)
    d = rng.randrange(1, c.n)
    pub = b"".join(v.to_bytes(32, "big") for v in O.pubkey(c, d))
    recs, seen = [], set()
    want_all = {(m, neg) for m in range(1 << (T - 1)) for neg in (False, True)}
    while len(recs) < 64:
        msg = rng.randbytes(64)
        r, s = O.sign_digest(c, d, hashlib.sha256(msg).digest(), rng.randrange(1, c.n))
        reads = comb_reads(r * pow(s, -1, c.n) % c.n, c.n)
        if seen != want_all and not (reads - seen):
            continue
        seen |= reads
        if len(recs) % 8 == 7:  # same r, s (the same u2), another message: R_MATH
            msg = bytes([msg[0] ^ 1]) + msg[1:]
        sig = O.marshal_ecdsa_signature(r, s)
        recs.append((pub, sig, msg, orc.csp_verify(pub, sig, hashlib.sha256(msg).digest())))
    assert seen == want_all  # every entry index with both signs
    return recs


def keys_used_4_to_16(n_want, seed):
    """indices into a generated pool: whole keys, each with 4..16 records of
    which at least 4 reach the group equation (so each gets a table)"""
    pool = workload.generate(98_304, 6_144, 64, 16, seed=seed)
    keys = pool.pub.reshape(-1, 64)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind="stable")
    bounds = np.flatnonzero(np.diff(inv.reshape(-1)[order])) + 1
    sel = []
    for kn, idx in enumerate(np.split(order, bounds)):
        take = idx[:4 + kn % 13]
        usable = int(((pool.reason[take] == 0) | (pool.reason[take] == 9)).sum())
        if len(take) < 4 or usable < 4 or len(sel) + len(take) > n_want:
            continue
        sel += list(take)
    sel = np.array(sel)
    assert len(sel) > n_want - 16
    return pool, np.sort(sel)


def test_p256_fused_chosen_u2_every_entry_both_signs(L):
    c = O.P256
    crafted = chosen_records(c, seed=2647)
    pool, sel = keys_used_4_to_16(40_960 - 64, seed=53)
    fill = 40_960 - 64 - len(sel)  # the last few records: keys of their own (the ladder)
    extra = workload.generate(max(fill, 1), max(fill, 1), 64, 16, seed=54)
    n = 40_960
    pub = np.concatenate([pool.pub.reshape(-1, 64)[sel].reshape(-1), extra.pub[:64 * fill],
                          np.frombuffer(b"".join(r[0] for r in crafted), np.uint8)])
    msg = np.concatenate([pool.msg, extra.msg,
                          np.frombuffer(b"".join(r[2] for r in crafted), np.uint8)])
    sig = np.concatenate([pool.sig, extra.sig,
                          np.frombuffer(b"".join(r[1] for r in crafted) + b"\0", np.uint8)])
    cl = np.array([len(r[1]) for r in crafted], np.uint64)
    mo = np.concatenate([pool.msg_off[sel], extra.msg_off[:fill] + len(pool.msg),
                         len(pool.msg) + len(extra.msg) + 64 * np.arange(64, dtype=np.uint64)])
    so = np.concatenate([pool.sig_off[sel], extra.sig_off[:fill] + len(pool.sig),
                         len(pool.sig) + len(extra.sig) + np.cumsum(cl) - cl])
    ml = np.concatenate([pool.msg_len[sel], extra.msg_len[:fill], np.full(64, 64, np.uint32)])
    sl = np.concatenate([pool.sig_len[sel], extra.sig_len[:fill], cl.astype(np.uint32)])
    want = np.concatenate([pool.reason[sel], extra.reason[:fill],
                           np.array([r[3] for r in crafted], np.uint8)])
    assert len(want) == n == len(ml) and set(want[-64:]) == {0, 9}
    arrs = (pub, sig, so.astype(np.uint64), sl.astype(np.uint32), msg, mo.astype(np.uint64),
            ml.astype(np.uint32))
    # the assembled batch against the C oracle: the chosen records and a sample
    for i in list(range(n - 64, n)) + list(np.random.default_rng(6).choice(n - 64, 100, False)):
        dg = hashlib.sha256(bytes(msg[int(mo[i]):int(mo[i]) + int(ml[i])])).digest()
        assert orc.csp_verify(bytes(pub[64 * i:64 * i + 64]),
                              bytes(sig[int(so[i]):int(so[i]) + int(sl[i])]), dg) == want[i], i
    bits, reason, tm = _dev_verify(L, arrs, n, flags=_lib.BH_F_HASH_SHA256)
    bad = np.nonzero(reason != want)[0]
    assert not len(bad), [(int(i), int(reason[i]), int(want[i])) for i in bad[:10]]
    assert (bits == (want == 0)).all()
    math = (want == 0) | (want == 9)
    assert tm.wide == 1
    assert tm.n_keycomb == int(math.sum()) - int(math[len(sel):len(sel) + fill].sum())
    assert tm.n_ladder == int(math[len(sel):len(sel) + fill].sum())
    assert tm.n_keytables == len(np.unique(pool.pub.reshape(-1, 64)[sel], axis=0)) + 1


def test_k1_bdls_just_above_32768_through_the_comb(L):
    from tests.bdls_util import pack_bdls
    from tests.conftest import ROOT
    from tests.test_bdls import _round_records
    with open(os.path.join(ROOT, "tests", "golden", "bdls_vectors.jsonl")) as f:
        gold = [r for r in map(json.loads, f) if r["curve"] == "secp256k1"]
    rb = workload.generate_bdls_round(nval=100, curve=1, seed=31)
    rnd = [dict(x=d["x"].hex(), y=d["y"].hex(), r=d["r"].hex(), s=d["s"].hex(),
                msg=d["msg"].hex(), version=d["version"]) for d in _round_records(rb, range(rb.n))]
    reps = (32_768 - rb.n) // len(gold) + 1
    recs = gold * reps + rnd
    n = len(recs)
    assert 32_768 < n <= 32_768 + len(gold)
    want = np.array([r["reason"] for r in gold] * reps + [0] * rb.n, np.uint8)
    DA = _lib.DeviceArray
    d = [DA.from_numpy(0, x) for x in pack_bdls(recs)]
    words = DA(0, ((n + 63) // 64) * 8)
    reason = DA(0, n)
    tm = _lib.BhTiming()
    b = _lib.BhBdlsBatch(*[x.ptr for x in d])
    _lib.check(L.bh_verify_bdls_dev(0, 1, ctypes.byref(b), n, words.ptr, reason.ptr, None, 1,
                                    ctypes.byref(tm)))
    got = reason.to_numpy(np.uint8, n)
    bits = np.unpackbits(words.to_numpy(np.uint64, (n + 63) // 64).view(np.uint8),
                         bitorder="little")[:n].astype(bool)
    for x in d + [words, reason]:
        x.free()
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:10]]
    assert (bits == (want == 0)).all()
    assert tm.wide == 1 and tm.n_keytables > 0
    assert tm.n_keycomb > 0.9 * int(((want == 0) | (want == 9)).sum())


def test_57_registered_keys_then_batches(L):
    from tests.test_registry import count, register
    for cv in (0, 1):
        _lib.check(L.bh_keys_clear(-1, cv))
    try:
        w = workload.generate(2_000, 57, 64, 16, seed=57)
        # (a record with a corrupted key is reason 7 and carries a key of its own)
        keys = np.unique(w.pub.reshape(-1, 64)[w.reason != 7], axis=0)
        assert len(keys) == 57
        assert (register(L, 0, keys.reshape(-1)) == 0).all() and count(L, 0) == 57
        big = workload.generate(40_960, 57, 64, 16, seed=57)  # the same 57 keys
        assert len(np.unique(np.concatenate([keys, big.pub.reshape(-1, 64)[big.reason != 7]]),
                             axis=0)) == 57
        for b, wide in ((w, 16), (big, 1)):
            bits, reason, tm = _dev_verify(L, b.arrays(), b.n, flags=_lib.BH_F_HASH_SHA256)
            assert (reason == b.reason).all() and (bits == b.expected_valid).all()
            assert tm.wide == wide and tm.n_keytables == 0 and tm.n_ladder == 0
            assert tm.n_keycomb == int(((b.reason == 0) | (b.reason == 9)).sum())
    finally:
        for cv in (0, 1):
            _lib.check(L.bh_keys_clear(-1, cv))
