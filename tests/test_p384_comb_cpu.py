"""CPU: the per-pass key combs of the P-384 pass (bdls_amd/csrc/comb384.h,
BH_F_BATCH_KEYS: grouping, routing, comb build, the comb route
stage384_comb) compiled for the host by the TEST-ONLY harness
tests/native_p384comb/hostsim384_comb.cpp, checked against Python integers and
the oracle on the P-384 curve; and the host-only parts of the flag. A missing
harness FAILS these tests: `make` builds it."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests.conftest import ROOT
from tests.p384_util import N, P, P384

HOSTSIM384C = os.path.join(ROOT, "tests", "native", "build", "libhostsim384c.so")
SELFTEST = os.path.join(ROOT, "tests", "native", "build", "comb384_selftest")
COMB = os.path.join(ROOT, "tests", "golden", "p384_comb_vectors.jsonl")
G = (P384.gx, P384.gy)
BH_E_INVALID, BH_E_NOT_INIT = -1, -2
R_INV = pow(1 << 392, -1, P)  # 14 limbs of 28 bits: Montgomery R = 2^392


@pytest.fixture(scope="module")
def hc():
    assert os.path.exists(HOSTSIM384C), "tests/native/build/libhostsim384c.so is not built (make)"
    L = ctypes.CDLL(HOSTSIM384C)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.hs384c_hash.argtypes = [vp]
    L.hs384c_hash.restype = u32
    L.hs384c_buckets.argtypes = [u32, u32]
    L.hs384c_buckets.restype = u32
    L.hs384c_plan.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.hs384c_plan.restype = u32
    L.hs384c_table_raw.argtypes = [vp, vp]
    L.hs384c_gcomb_raw.argtypes = [vp]
    L.hs384c_verify.argtypes = [vp] * 7 + [u32] * 5 + [vp, u32, vp, vp]
    L.hs384c_verify.restype = u32
    return L


@pytest.fixture(scope="module")
def mixed_counts():
    """600 records over 24 keys, then 60 over 30 other keys (2 each)."""
    lc = U.LibCrypto()
    r1, w1 = U.signed_batch(lc, 600, 24, seed=600, family="SHA2")
    r2, w2 = U.signed_batch(lc, 60, 30, seed=6060, family="SHA2")
    return r1 + r2, np.concatenate([w1, w2])


def raw(q):
    return q[0].to_bytes(48, "big") + q[1].to_bytes(48, "big")


def key_bytes(r):
    return bytes.fromhex(r["qx"] + r["qy"])


def load_comb():
    with open(COMB) as f:
        return [json.loads(l) for l in f]


def expect(recs, no_low_s):
    return np.array([r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]
                     for r in recs], np.uint8)


def run(hc, arrs, flags, pass_chunk=0, inv_chunk=7, reg=()):
    pub, sig, so, sl, msg, mo, ml = arrs
    n = len(sl)
    out, route = np.full(n, 255, np.uint8), np.full(n, 255, np.uint8)
    regb = b"".join(reg)
    tables = hc.hs384c_verify(pub.ctypes.data, sig.ctypes.data, so.ctypes.data, sl.ctypes.data,
                              msg.ctypes.data, mo.ctypes.data, ml.ctypes.data, n, flags,
                              pass_chunk, inv_chunk, 4, regb or None, len(reg), out.ctypes.data,
                              route.ctypes.data)
    return out, route, tables


def rule(recs, want, chunk=None, registered=()):
    """Per record 0 ladder / 1 comb / 2 registry, and the combs built, per chunk."""
    chunk = chunk or len(recs)
    route, tables = [], 0
    for base in range(0, len(recs), chunk):
        part = list(zip(recs[base:base + chunk], want[base:base + chunk]))
        uses = {}
        for r, w in part:
            if w in (O.R_OK, O.R_MATH):
                uses[key_bytes(r)] = uses.get(key_bytes(r), 0) + 1
        for r, w in part:
            k = key_bytes(r)
            route.append(0 if w not in (O.R_OK, O.R_MATH) else 2 if k in registered
                         else 1 if uses[k] >= 4 else 0)
        tables += sum(1 for k, v in uses.items() if v >= 4 and k not in registered)
    return np.array(route, np.uint8), tables


def test_table_entries(hc):
    """Every entry of the comb of a random key, of G and of -G is k_m Q with
    k_m = sum of 2^(64 j) over the bits of m; stored limbs are 28 bits and the
    coordinates canonical (< p). G's comb is the one the pass uses."""
    rng = random.Random(3843)
    j = rng.randrange(2, N)
    for name, scalar in (("random", j), ("G", 1), ("-G", N - 1)):
        q = O.pubkey(P384, scalar)
        tab = np.zeros(63 * 28, np.uint32)
        assert hc.hs384c_table_raw(raw(q), tab.ctypes.data) == 0
        assert (tab < (1 << 28)).all()
        for m in range(1, 64):
            km = sum(1 << (64 * t) for t in range(6) if (m >> t) & 1)
            row = tab[(m - 1) * 28:m * 28]
            xm = sum(int(v) << (28 * i) for i, v in enumerate(row[:14]))
            ym = sum(int(v) << (28 * i) for i, v in enumerate(row[14:]))
            assert xm < P and ym < P, (name, m)
            assert (xm * R_INV % P, ym * R_INV % P) == O.scalar_mult(P384, km * scalar, G), (name, m)
        if name == "G":
            g = np.zeros(63 * 28, np.uint32)
            hc.hs384c_gcomb_raw(g.ctypes.data)
            assert (g == tab).all()
    off = bytearray(raw(G))
    off[95] ^= 1
    assert hc.hs384c_table_raw(bytes(off), tab.ctypes.data) == -1


def test_grouping(hc):
    """300 records over keys with 1, 2, 3, 4, 5 and 64 prep-passing records, prep-rejected
    records of a frequent key and of a key that would reach 4 only with them,
    and two keys that collide in the bucket index."""
    rng = random.Random(3844)
    n = 300
    buckets = hc.hs384c_buckets(n, 4)
    assert buckets == 1024
    pts = [raw(O.point_add(P384, O.pubkey(P384, 5), O.pubkey(P384, k))) for k in range(10, 210)]
    by_bucket = {}
    for q in pts:
        by_bucket.setdefault(hc.hs384c_hash(q) & (buckets - 1), []).append(q)
    a, b = next(v for v in by_bucket.values() if len(v) >= 2)[:2]
    others = [q for q in pts if q not in (a, b)]
    counts = [(a, 5), (b, 4), (others[0], 1), (others[1], 2), (others[2], 3), (others[3], 64),
              (others[4], 3)]
    recs = [(k, 1) for k, c in counts for _ in range(c)]
    recs += [(others[3], 0)] * 6 + [(others[4], 0)] * 2   # rejected by prep: not counted
    fill = 10
    while len(recs) < n:   # the rest: keys of their own, 1 to 3 records each
        c = min(1 + len(recs) % 3, n - len(recs))
        recs += [(others[fill], 1)] * c
        fill += 1
    rng.shuffle(recs)
    pub = np.frombuffer(b"".join(k for k, _ in recs), np.uint8)
    ok = np.array([o for _, o in recs], np.uint8)
    want_comb = {a, b, others[3]}
    for reg_keys in ((), (others[3], others[1])):
        route, slot, rep = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        regb = b"".join(reg_keys)
        tables = hc.hs384c_plan(pub.ctypes.data, ok.ctypes.data, n, 4, regb or None,
                                len(reg_keys), route.ctypes.data, slot.ctypes.data,
                                rep.ctypes.data)
        assert tables == len(want_comb - set(reg_keys))
        slots = {}
        for i, (k, o) in enumerate(recs):
            want = 0 if not o else 2 if k in reg_keys else 1 if k in want_comb else 0
            assert route[i] == want, (i, o, route[i], want)
            if o:   # the representative is the first record of the key that passed prep
                assert rep[i] == next(j for j, (k2, o2) in enumerate(recs) if o2 and k2 == k)
            else:
                assert rep[i] == 0xffffffff
            if want == 1:
                assert slots.setdefault(k, slot[i]) == slot[i] and slot[i] < tables
            if want == 2:
                assert slot[i] == reg_keys.index(k)
        assert len(set(slots.values())) == len(slots)


@pytest.mark.parametrize("no_low_s", [False, True])
def test_comb_fixture(hc, no_low_s):
    recs = load_comb()
    assert 80 <= len(recs) <= 400 and os.path.getsize(COMB) < 256 * 1024
    want = expect(recs, no_low_s)
    assert np.isin(want, (O.R_OK, O.R_MATH)).all()
    for r in recs:  # the committed expectations are the oracle's
        assert O.csp_verify(P384, int(r["qx"], 16), int(r["qy"], 16), bytes.fromhex(r["sig"]),
                            bytes.fromhex(r["digest"]))[1] == r["reason"], r["tag"]
    out, route, tables = run(hc, U.pack384(recs, False), _lib.BH_F_NO_LOW_S if no_low_s else 0)
    bad = [(r["tag"], int(o), int(w)) for r, o, w in zip(recs, out, want) if o != w]
    assert not bad
    assert (route == 1).all() and tables == len({key_bytes(r) for r in recs})
    tags = {r["tag"] for r in recs}
    for t in ("q_dbl_c31", "q_dbl_c0", "q_neg_c31", "q_neg_c0", "g_dbl_c63", "g_dbl_c31",
              "g_dbl_c0", "g_neg_c63", "g_neg_c31", "g_neg_c0_final_inf", "g_dbl_c63_qG",
              "g_neg_c63_qnegG", "final_inf", "small", "u2_1", "u2_2", "u2_nm1", "u1_zero",
              "digits", "xwrap0", "xwrap0_wrong_r"):
        assert t in tags, t


def test_comb_fixture_situations():
    """The generator's replay of the walk finds each tag's situation in the committed records."""
    from tests.golden import gen_golden_p384_comb as GEN
    recs = {r["tag"]: r for r in load_comb()}

    def events(tag):
        r = recs[tag]
        _, rr, ss = O.unmarshal_ecdsa_signature(bytes.fromhex(r["sig"]))
        w = pow(ss, -1, N)
        u1, u2 = int(r["digest"], 16) % N * w % N, rr * w % N
        return GEN.walk(u1, u2, (int(r["qx"], 16), int(r["qy"], 16))), u1, u2
    for kind in ("q_dbl", "q_neg", "g_dbl", "g_neg"):
        for c in (63, 31, 0):
            tag = f"{kind}_c{c}" + ("_final_inf" if (kind, c) == ("g_neg", 0) else "")
            if tag in recs:
                assert (kind, c) in events(tag)[0][1], tag
            else:
                assert kind[0] == "q" and c == 63  # the accumulator is empty there
    (A, ev), _, _ = events("g_neg_c63_qnegG")
    assert ev[:3] == [("g_neg", 63), ("inf_dbl", 62), ("add_to_inf", 62)]
    assert ("g_dbl", 63) in events("g_dbl_c63_qG")[0][1]
    assert events("final_inf")[0][0] is None and events("g_neg_c0_final_inf")[0][0] is None
    (_, _), u1, u2 = events("small")
    assert u1 < 1 << 64 and u2 < 1 << 64
    assert [events(t)[2] for t in ("u2_1", "u2_2", "u2_nm1")] == [1, 2, N - 1]
    assert events("u1_zero")[1] == 0
    (_, _), u1, u2 = events("digits")
    assert [GEN.digit(u, c) for u in (u1, u2) for c in (5, 9)] == [63, 32, 63, 32]
    assert events("xwrap0")[0][0][0] >= N


def test_golden_times_four(hc):
    """p384_vectors.jsonl four times over (788 records): digest mode and both
    fused families through a flagged pass."""
    base = U.load_golden384()
    recs = [r for _ in range(4) for r in base]
    assert len(recs) == 788
    for no_low_s in (False, True):
        want = expect(recs, no_low_s)
        out, route, tables = run(hc, U.pack384(recs, False), _lib.BH_F_NO_LOW_S if no_low_s else 0)
        assert (out == want).all(), [r["tag"] for r, o, w in zip(recs, out, want) if o != w][:8]
        wr, wt = rule(recs, want)
        assert (route == wr).all() and tables == wt
        # every key of a prep-passing record occurs four times: all of them ride the comb
        assert (route == np.isin(want, (O.R_OK, O.R_MATH))).all()
    for family, flag in (("SHA2", _lib.BH_F_HASH_SHA256), ("SHA3", _lib.BH_F_HASH_SHA3_256)):
        fused = [r for r in recs if r.get("family") == family]
        want = expect(fused, False)
        out, route, tables = run(hc, U.pack384(fused, True), flag)
        assert (out == want).all()
        assert (route == np.isin(want, (O.R_OK, O.R_MATH))).all() and tables > 0


@pytest.mark.parametrize("chunk", [0, 128])
def test_mixed_counts(hc, mixed_counts, chunk):
    recs, want = mixed_counts
    out, route, tables = run(hc, U.pack384(recs, True), _lib.BH_F_HASH_SHA256, pass_chunk=chunk)
    assert (out == want).all()
    wr, wt = rule(recs, want, chunk=chunk or None)
    assert (route == wr).all() and tables == wt
    if not chunk:
        assert (route[:600] == np.isin(want[:600], (O.R_OK, O.R_MATH))).all()
        assert (route[600:] == 0).all() and tables == 24
    else:
        assert tables > 24 and (route[640:] == 0).all()


def test_registry_and_comb(hc, mixed_counts):
    """Two frequent keys registered: their records take the registry's route, the
    other frequent keys get combs, the reasons are the same."""
    recs, want = mixed_counts
    two = list(dict.fromkeys(key_bytes(r) for r in recs[:24]))[:2]
    out, route, tables = run(hc, U.pack384(recs, True), _lib.BH_F_HASH_SHA256, reg=two)
    assert (out == want).all()
    wr, wt = rule(recs, want, registered=set(two))
    assert (route == wr).all() and tables == wt == 22 and (route == 2).sum() > 40


def _dummy():
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    return buf, p, _lib.BhBatch(*([p] * 7))


def test_flag_abi_before_any_device():
    """128 is a known flag: before bh_init a flagged call answers BH_E_NOT_INIT, not
    BH_E_INVALID; 0x100 | 128 is still an unknown flag; exclusivity is unchanged."""
    assert _lib.BH_F_BATCH_KEYS == 128
    hdr = open(os.path.join(ROOT, "include", "bdls_hip.h")).read()
    assert "#define BH_F_BATCH_KEYS 128u" in hdr
    code = (
        "import ctypes, json, sys\n"
        "sys.path.insert(0, '.')\n"
        "import numpy as np\n"
        "from bdls_amd import _lib\n"
        "L = _lib.lib()\n"
        "buf = np.zeros(256, np.uint8)\n"
        "p = buf.ctypes.data\n"
        "b = _lib.BhBatch(*([p] * 7))\n"
        "out = []\n"
        "for curve in (0, 2):\n"
        "    out.append(L.bh_verify(curve, ctypes.byref(b), 1, 128, p, p))\n"
        "    out.append(L.bh_verify(curve, ctypes.byref(b), 1, 128 | 1, p, p))\n"
        "    out.append(L.bh_verify(curve, ctypes.byref(b), 1, 0x100 | 128, p, p))\n"
        "    e = _lib.last_error()\n"
        "    out.append('unknown flag' in e)\n"
        "    out.append(L.bh_verify(curve, ctypes.byref(b), 1, 128 | 1 | 8, p, p))\n"
        "    out.append('exclusive' in _lib.last_error())\n"
        "    out.append(L.bh_verify(curve, ctypes.byref(b), 1, 128 | 32 | 64, p, p))\n"
        "    out.append('exclusive' in _lib.last_error())\n"
        "out.append(L.bh_verify_2seg(0, ctypes.byref(b), p, p, 1, 128 | 1, p, p))\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    per_curve = [BH_E_NOT_INIT, BH_E_NOT_INIT, BH_E_INVALID, True, BH_E_INVALID, True,
                 BH_E_INVALID, True]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == per_curve * 2 + [BH_E_NOT_INIT]


def test_csp_flag_only_for_p384():
    from bdls_amd.bccsp import HipCSP
    for bk in (False, True):
        csp = HipCSP.__new__(HipCSP)  # no device
        csp._flags, csp._batch_keys = 0, bk
        assert csp._batch_flags(_lib.BH_CURVE_P256) == 0
        assert csp._batch_flags(_lib.BH_CURVE_P384) == (128 if bk else 0)


def test_sanitizer_selftest_program():
    """The stand-alone program (address + undefined-behaviour sanitizers, its own
    main) builds, runs a flagged pass over 48 records four ways and exits 0."""
    b = subprocess.run(["make", "-C", ROOT, os.path.relpath(SELFTEST, ROOT)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([SELFTEST], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
