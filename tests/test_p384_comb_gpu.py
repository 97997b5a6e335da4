"""GPU: per-pass key combs of the P-384 pass (BH_F_BATCH_KEYS: k384_comb_group,
_assign, _plan, _bases, _rows, k384_comb), against the crafted fixture
tests/golden/p384_comb_vectors.jsonl, the golden fixture, libcrypto-signed
batches and the same calls without the flag: results never depend on it, the
routing counts are what the rule says. Every test leaves the registry empty."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from bdls_amd.bccsp import ECDSAPublicKey, HipCSP, verify_packed
from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests.conftest import ROOT
from tests.test_p384_keys_gpu import count, distinct_keys, expect, key_bytes, load, register, run_dev

pytestmark = pytest.mark.gpu
C384 = _lib.BH_CURVE_P384
COMB = os.path.join(ROOT, "tests", "golden", "p384_comb_vectors.jsonl")
BK = _lib.BH_F_BATCH_KEYS


@pytest.fixture(scope="module")
def csp():
    return HipCSP()


@pytest.fixture
def reg(csp, request):
    """The library, with the P-384 registry empty before and after."""
    L = _lib.lib()
    request.addfinalizer(lambda: _lib.check(L.bh_keys384_clear(-1)))
    _lib.check(L.bh_keys384_clear(-1))
    assert count(L) == 0
    return L


@pytest.fixture(scope="module")
def mixed_counts():
    """600 records over 24 keys (25 each) then 60 over 30 other keys (2 each)."""
    lc = U.LibCrypto()
    r1, w1 = U.signed_batch(lc, 600, 24, seed=600, family="SHA2")
    r2, w2 = U.signed_batch(lc, 60, 30, seed=6060, family="SHA2")
    return r1 + r2, np.concatenate([w1, w2])


def routing(recs, want, chunk=None, registered=()):
    """(records on a table route, combs built) by the rule, per chunk."""
    chunk = chunk or len(recs)
    on, tables = 0, 0
    for base in range(0, len(recs), chunk):
        part = [(key_bytes(r), w) for r, w in zip(recs[base:base + chunk], want[base:base + chunk])
                if w in (O.R_OK, O.R_MATH)]
        uses = {}
        for k, _ in part:
            uses[k] = uses.get(k, 0) + 1
        on += sum(1 for k, _ in part if k in registered or uses[k] >= 4)
        tables += sum(1 for k, v in uses.items() if v >= 4 and k not in registered)
    return on, tables


def check(L, recs, fused, flags, want, registered=()):
    """The flagged resident call against `want` and the rule, then the unflagged one."""
    arrs = U.pack384(recs, fused)
    reason, bits, t = run_dev(L, arrs, len(recs), flags | BK)
    bad = [(r.get("tag"), int(g), int(w)) for r, g, w in zip(recs, reason, want) if g != w]
    assert not bad, bad[:8]
    assert (bits == (want == 0)).all()
    on, tables = routing(recs, want, registered=registered)
    assert (t.n_keycomb, t.n_keytables, t.n_ladder) == (on, tables, len(recs) - on)
    if on:
        assert t.keycomb_ms > 0 and t.plan_ms > 0
    if not registered:
        r0, b0, t0 = run_dev(L, arrs, len(recs), flags)
        assert (r0 == reason).all() and (b0 == bits).all()
        assert (t0.n_keycomb, t0.n_keytables, t0.n_ladder) == (0, 0, len(recs))
    return t


def test_comb_fixture(reg):
    recs = load(COMB)
    nkeys = len(distinct_keys(recs))
    for no_low_s in (False, True):
        f = _lib.BH_F_NO_LOW_S if no_low_s else 0
        want = expect(recs, no_low_s)
        t = check(reg, recs, False, f, want)
        assert t.n_keycomb == int(np.isin(want, (O.R_OK, O.R_MATH)).sum()) == len(recs)
        assert t.n_keytables == nkeys and t.keycomb_ms > 0
        valid, reason = verify_packed(*U.pack384(recs, False), curve=C384, flags=f | BK)
        assert (reason == want).all() and (valid == (want == 0)).all()


def test_golden_times_four(reg):
    base = U.load_golden384()
    recs = [dict(r, tag=f"{r['tag']}#{k}") for k in range(4) for r in base]
    assert len(recs) == 788
    for no_low_s in (False, True):
        check(reg, recs, False, _lib.BH_F_NO_LOW_S if no_low_s else 0, expect(recs, no_low_s))
    for family, flag in (("SHA2", _lib.BH_F_HASH_SHA256), ("SHA3", _lib.BH_F_HASH_SHA3_256)):
        fused = [r for r in recs if r.get("family") == family]
        assert len(fused) >= 44
        t = check(reg, fused, True, flag, expect(fused, False))
        assert t.n_keycomb > 0
        valid, reason = verify_packed(*U.pack384(fused, True), curve=C384, flags=flag | BK)
        assert (reason == expect(fused, False)).all()


def test_sha384_digest_pass(reg):
    """BH_F_HASH_SHA384: the digest pass, then the flagged curve pass in digest mode."""
    import hashlib
    lc = U.LibCrypto()
    rng = np.random.default_rng(3841)
    recs, want = [], []
    for i in range(100):
        d = 2000 + (i % 5 if i < 90 else i)  # five keys of 18 records, ten of one
        qx, qy = O.pubkey(U.P384, d)
        msg = rng.integers(0, 256, 40 + i, dtype=np.uint8).tobytes()
        k = lc.key(d, qx, qy)
        r_, s_ = lc.sign(k, hashlib.sha384(msg).digest())
        lc.free_key(k)
        s_ = min(s_, U.N - s_)
        if i % 7 == 2:
            msg = msg[:-1] + bytes([msg[-1] ^ 1])
        recs.append({"qx": U.h48(qx), "qy": U.h48(qy), "msg": msg.hex(),
                     "sig": O.marshal_ecdsa_signature(r_, s_).hex()})
        want.append(O.R_MATH if i % 7 == 2 else O.R_OK)
    want = np.array(want, np.uint8)
    t = check(reg, recs, True, _lib.BH_F_HASH_SHA384, want)
    assert (t.n_keycomb, t.n_keytables, t.n_ladder) == (90, 5, 10)
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384,
                                  flags=_lib.BH_F_HASH_SHA384 | BK)
    assert (reason == want).all() and (valid == (want == 0)).all()


def chain_batch(nkeys, copies, seed, msg_len=40):
    """nkeys keys d, d + 1, ... (a chain of additions of G), one libcrypto-signed
    record each, every fifth spoiled (message bit, then r + 1, in turn), the
    whole repeated `copies` times. Returns (recs, want)."""
    import random
    lc = U.LibCrypto()
    rng = random.Random(seed)
    d = rng.randrange(1, U.N - nkeys)
    pt = O.pubkey(U.P384, d)
    recs, want = [], []
    for k in range(nkeys):
        key = lc.key(d + k, *pt)
        msg = bytes(rng.getrandbits(8) for _ in range(msg_len + k % 5))
        r, s_ = lc.sign(key, U.family_hash("SHA2", msg))
        lc.free_key(key)
        s_ = min(s_, U.N - s_)
        reason = O.R_OK
        if k % 5 == 3:
            reason = O.R_MATH
            if k % 2:
                msg = msg[:-1] + bytes([msg[-1] ^ 4])
            else:
                r = (r + 1) % U.N or 1
        recs.append({"qx": U.h48(pt[0]), "qy": U.h48(pt[1]), "msg": msg.hex(),
                     "sig": O.marshal_ecdsa_signature(r, s_).hex()})
        want.append(reason)
        pt = O.point_add(U.P384, pt, (U.P384.gx, U.P384.gy))
    return recs * copies, np.tile(np.array(want, np.uint8), copies)


@pytest.mark.parametrize("n", [4, 63, 64, 65, 257])
def test_one_key_sizes(reg, n):
    """All records under one key: one table, every record on the comb route."""
    one, w1 = chain_batch(1, 1, seed=77)
    other, w2 = chain_batch(5, 1, seed=78)  # its fourth record is spoiled
    recs = [dict(other[i % 5], qx=one[0]["qx"], qy=one[0]["qy"]) if i % 9 == 4 else one[0]
            for i in range(n)]
    want = np.array([O.R_MATH if i % 9 == 4 else O.R_OK for i in range(n)], np.uint8)
    assert len(distinct_keys(recs)) == 1
    t = check(reg, recs, True, _lib.BH_F_HASH_SHA256, want)
    assert (t.n_keycomb, t.n_keytables, t.n_ladder) == (n, 1, 0)


def test_mixed_counts(reg, mixed_counts):
    recs, want = mixed_counts
    t = check(reg, recs, True, _lib.BH_F_HASH_SHA256, want)
    first = int(np.isin(want[:600], (O.R_OK, O.R_MATH)).sum())
    assert (t.n_keycomb, t.n_keytables, t.n_ladder) == (first, 24, 660 - first)
    assert t.build_ladder_ms > 0


def test_chunks_child_process(mixed_counts, tmp_path):
    """BH_P384_CHUNK=128 in a fresh child: grouping is per chunk."""
    recs, want = mixed_counts
    path = tmp_path / "recs.json"
    path.write_text(json.dumps(recs))
    code = (
        "import json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "from bdls_amd.bccsp import HipCSP\n"
        "from tests import p384_util as U\n"
        "from tests.test_p384_keys_gpu import run_dev\n"
        f"recs = json.load(open({str(path)!r}))\n"
        "HipCSP()\n"
        "L = _lib.lib()\n"
        "s0 = _lib.device_stats()\n"
        "f = _lib.BH_F_HASH_SHA256 | _lib.BH_F_BATCH_KEYS\n"
        "reason, bits, t = run_dev(L, U.pack384(recs, True), len(recs), f)\n"
        "s1 = _lib.device_stats()\n"
        "print(json.dumps({'reason': reason.tolist(), 'bits': bits.tolist(), 'kc': t.n_keycomb,\n"
        "                  'kt': t.n_keytables, 'lad': t.n_ladder, 'batches': s1[0] - s0[0]}))\n")
    env = dict(os.environ, BH_P384_CHUNK="128")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["reason"] == want.tolist() and res["bits"] == (want == 0).tolist()
    on, tables = routing(recs, want, chunk=128)
    assert (res["kc"], res["kt"], res["lad"]) == (on, tables, 660 - on)
    assert tables > 24 and res["batches"] == 1


def test_many_keys(reg):
    """1,024 keys x 4 copies of one signed record each: the build grid and the
    hash table over many workgroups."""
    recs, want = chain_batch(1024, 4, seed=4096)
    t = check(reg, recs, True, _lib.BH_F_HASH_SHA256, want)
    assert (t.n_keytables, t.n_keycomb, t.n_ladder) == (1024, 4096, 0)
    assert int((want == O.R_MATH).sum()) == 4 * 205


def test_registry_and_comb(reg, mixed_counts):
    recs, want = mixed_counts
    arrs = U.pack384(recs, True)
    r0, b0, t0 = run_dev(reg, arrs, 660, _lib.BH_F_HASH_SHA256 | BK)
    two = distinct_keys(recs[:24])[:2]
    assert (register(reg, two) == 0).all() and count(reg) == 2
    t1 = check(reg, recs, True, _lib.BH_F_HASH_SHA256, want, registered=set(two))
    assert t1.n_keytables == 22 and t1.n_keycomb == t0.n_keycomb
    _lib.check(reg.bh_keys384_clear(0))
    r2, b2, t2 = run_dev(reg, arrs, 660, _lib.BH_F_HASH_SHA256 | BK)
    assert (r2 == r0).all() and (b2 == b0).all() and (r2 == want).all()
    assert t2.n_keytables == 24 and t2.n_keycomb == t0.n_keycomb


@pytest.mark.parametrize("two_span", [False, True])
def test_verify_mixed(reg, two_span):
    """An alternating P-256 / P-384 batch (the P-384 pool cycled, so its keys
    repeat): the flagged call equals the unflagged one bit for bit."""
    from bdls_amd.bccsp import verify_mixed
    from tests import mixed_util as M
    p256, p384 = M.pool("SHA2")
    recs = M.pick(M.pattern("alternating", 8 * len(p384)), p256, p384)
    args = M.build_mixed(recs, two_span)
    want = np.array([M.expect(r, False) for r in recs], np.uint8)
    v0, x0 = verify_mixed(*args, flags=_lib.BH_F_HASH_SHA256)
    v1, x1 = verify_mixed(*args, flags=_lib.BH_F_HASH_SHA256 | BK)
    assert (v0 == v1).all() and (x0 == x1).all() and (x1 == want).all()


def test_csp_batch_keys(reg, mixed_counts):
    recs, want = mixed_counts
    keys = [ECDSAPublicKey(int(r["qx"], 16), int(r["qy"], 16), curve="P-384") for r in recs]
    sigs = [bytes.fromhex(r["sig"]) for r in recs]
    msgs = [bytes.fromhex(r["msg"]) for r in recs]
    dgs = [bytes.fromhex(r["digest"]) for r in recs]
    a, b = HipCSP(batch_keys=True), HipCSP(batch_keys=False)
    va, ra = a.batch_verify(keys, sigs, dgs)
    vb, rb = b.batch_verify(keys, sigs, dgs)
    assert (va == vb).all() and (ra == rb).all() and (ra == want).all()
    va, ra = a.batch_identity_verify(keys, msgs, sigs)
    vb, rb = b.batch_identity_verify(keys, msgs, sigs)
    assert (va == vb).all() and (ra == rb).all() and (ra == want).all()
