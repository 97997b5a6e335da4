"""CPU: the P-384 key registry (bdls_amd/csrc/keys384.h: table build, hash
table, the table-route stage stage384_keywin) compiled for the host by the
TEST-ONLY harness tests/native_p384keys/hostsim384_keys.cpp, checked against
Python integers, the oracle on the P-384 curve and OpenSSL libcrypto; and the
host-only parts of bh_keys384_*. A missing harness FAILS these tests: `make`
builds it."""
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

HOSTSIM384K = os.path.join(ROOT, "tests", "native", "build", "libhostsim384k.so")
KEYWIN = os.path.join(ROOT, "tests", "golden", "p384_keywin_vectors.jsonl")
G = (P384.gx, P384.gy)
TAB_WORDS = 96 * 15 * 28
BH_E_INVALID, BH_E_NOT_INIT = -1, -2


@pytest.fixture(scope="module")
def hk():
    assert os.path.exists(HOSTSIM384K), "tests/native/build/libhostsim384k.so is not built (make)"
    L = ctypes.CDLL(HOSTSIM384K)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.hs384k_reserve.argtypes = [u32]
    L.hs384k_count.restype = u32
    L.hs384k_buckets.restype = u32
    L.hs384k_register.argtypes = [vp, u32, vp]
    L.hs384k_find.argtypes = [vp]
    L.hs384k_find.restype = i32
    L.hs384k_hash.argtypes = [vp]
    L.hs384k_hash.restype = u32
    L.hs384k_table_raw.argtypes = [u32, vp]
    L.hs384k_gtab_raw.argtypes = [vp]
    L.hs384k_entry.argtypes = [u32, u32, u32, vp]
    L.hs384k_verify.argtypes = [vp] * 7 + [u32] * 3 + [vp, vp]
    return L


def load_keywin():
    with open(KEYWIN) as f:
        return [json.loads(l) for l in f]


def raw(q):
    return q[0].to_bytes(48, "big") + q[1].to_bytes(48, "big")


def register(hk, points):
    buf = b"".join(raw(q) for q in points)
    st = np.full(len(points), 99, np.uint8)
    hk.hs384k_register(buf, len(points), st.ctypes.data)
    return st


def find(hk, q):
    return hk.hs384k_find(raw(q) if isinstance(q, tuple) else q)


def from_words(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def run_hk(hk, arrs, flags, chunk=7):
    pub, sig, so, sl, msg, mo, ml = arrs
    n = len(sl)
    out = np.full(n, 255, np.uint8)
    route = np.full(n, 255, np.uint8)
    hk.hs384k_verify(pub.ctypes.data, sig.ctypes.data, so.ctypes.data, sl.ctypes.data,
                     msg.ctypes.data, mo.ctypes.data, ml.ctypes.data, n, flags, chunk,
                     out.ctypes.data, route.ctypes.data)
    return out, route


def expect(recs, no_low_s):
    return np.array([r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]
                     for r in recs], np.uint8)


def valid_keys(recs):
    """The distinct keys of recs that are points of P-384, in first-seen order."""
    seen = {}
    for r in recs:
        q = (int(r["qx"], 16), int(r["qy"], 16))
        if q[0] < P and q[1] < P and O.on_curve(P384, *q):
            seen.setdefault(q)
    return list(seen)


def test_table_build(hk):
    """Every entry of windows 0, 1, 47 and 95 (the layout has no carry window)
    for Q = G, 2G and two random keys is d 16^w Q; G's table as stored equals
    the fixed-base table of G row for row."""
    rng = random.Random(3841)
    ks = [1, 2, rng.randrange(3, N), rng.randrange(3, N)]
    hk.hs384k_reserve(4)
    assert (register(hk, [O.pubkey(P384, k) for k in ks]) == 0).all()
    for slot, k in enumerate(ks):
        assert find(hk, O.pubkey(P384, k)) == slot
        for w in (0, 1, 47, 95):
            for d in range(1, 16):
                xy = np.zeros(24, np.uint32)
                hk.hs384k_entry(slot, w, d, xy.ctypes.data)
                want = O.scalar_mult(P384, d * 16 ** w * k, G)
                assert (from_words(xy[:12]), from_words(xy[12:])) == want, (k, w, d)
    mine, gtab = np.zeros(TAB_WORDS, np.uint32), np.zeros(TAB_WORDS, np.uint32)
    hk.hs384k_table_raw(0, mine.ctypes.data)
    hk.hs384k_gtab_raw(gtab.ctypes.data)
    assert (mine == gtab).all()


def test_lookup(hk):
    rng = random.Random(3842)
    pts = [O.pubkey(P384, rng.randrange(1, N)) for _ in range(40)]
    hk.hs384k_reserve(4)
    hc = hk.hs384k_buckets()
    assert hc == 8
    # two keys of one bucket, found through the harness's hash
    by_bucket = {}
    for q in pts:
        by_bucket.setdefault(hk.hs384k_hash(raw(q)) & (hc - 1), []).append(q)
    a, b = next(v for v in by_bucket.values() if len(v) >= 2)[:2]
    others = [q for q in pts if q not in (a, b)]
    assert find(hk, a) == -1
    assert list(register(hk, [a])) == [0] and hk.hs384k_count() == 1
    assert find(hk, a) == 0 and find(hk, b) == -1          # same bucket, other key
    assert list(register(hk, [b, a])) == [0, 0] and hk.hs384k_count() == 2   # new, duplicate
    assert (find(hk, a), find(hk, b)) == (0, 1)
    # a key that differs from a registered one in one byte of Y only
    y_only = bytearray(raw(a))
    y_only[95] ^= 1
    assert find(hk, bytes(y_only)) == -1
    y_only = bytearray(raw(a))
    y_only[48] ^= 0x80
    assert find(hk, bytes(y_only)) == -1
    # not a point: status 7, not counted
    off = (a[0], (a[1] + 1) % P)
    assert list(register(hk, [off, (P, 1), (0, 0)])) == [7, 7, 7] and hk.hs384k_count() == 2
    assert find(hk, off) == -1
    # full: capacity 4, the later keys report 255, the earlier ones still hit
    st = register(hk, others[:4] + [a])
    assert list(st) == [0, 0, 255, 255, 0] and hk.hs384k_count() == 4
    assert [find(hk, q) for q in (a, b, others[0], others[1])] == [0, 1, 2, 3]
    assert find(hk, others[2]) == -1 and find(hk, others[3]) == -1
    hk.hs384k_clear()
    assert hk.hs384k_count() == 0 and find(hk, a) == -1
    assert list(register(hk, [b])) == [0] and find(hk, b) == 0


@pytest.fixture(scope="module")
def golden_registered(hk):
    """The golden fixture with every valid key registered in the harness."""
    recs = U.load_golden384()
    keys = valid_keys(recs)
    hk.hs384k_reserve(len(keys))
    assert (register(hk, keys) == 0).all() and hk.hs384k_count() == len(keys)
    return recs


@pytest.mark.parametrize("no_low_s", [False, True])
def test_golden_on_table_route_digest_mode(hk, golden_registered, no_low_s):
    recs = golden_registered
    assert len(recs) == 197
    want = expect(recs, no_low_s)
    out, route = run_hk(hk, U.pack384(recs, False), _lib.BH_F_NO_LOW_S if no_low_s else 0)
    bad = [(r["tag"], int(o), int(w)) for r, o, w in zip(recs, out, want) if o != w]
    assert not bad
    # a record is on the table route exactly when prep let it through (OK or MATH)
    assert (route == np.isin(want, (O.R_OK, O.R_MATH))).all()
    assert int(route.sum()) >= 60


@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_golden_on_table_route_fused(hk, golden_registered, family):
    recs = [r for r in golden_registered if r.get("family") == family]
    assert len(recs) >= 11
    flag = _lib.BH_F_HASH_SHA256 if family == "SHA2" else _lib.BH_F_HASH_SHA3_256
    for no_low_s in (False, True):
        want = expect(recs, no_low_s)
        out, route = run_hk(hk, U.pack384(recs, True), flag | (_lib.BH_F_NO_LOW_S if no_low_s else 0))
        assert (out == want).all(), [r["tag"] for r, o, w in zip(recs, out, want) if o != w]
        assert (route == np.isin(want, (O.R_OK, O.R_MATH))).all()


def test_keywin_fixture_matches_oracle_and_libcrypto():
    """The committed expectations are the oracle's (gen_golden_p384_keywin.py),
    and OpenSSL agrees on every record: arithmetic decides them all."""
    recs = load_keywin()
    assert 40 <= len(recs) <= 60 and os.path.getsize(KEYWIN) < 64 * 1024
    lc = U.LibCrypto()  # a load failure is an error of this test, never a skip
    for r in recs:
        q = (int(r["qx"], 16), int(r["qy"], 16))
        sig, dg = bytes.fromhex(r["sig"]), bytes.fromhex(r["digest"])
        assert O.csp_verify(P384, *q, sig, dg)[1] == r["reason"], r["tag"]
        rc, rr, ss = O.unmarshal_ecdsa_signature(sig)
        assert rc == O.R_OK
        nl = O.go_ecdsa_verify(P384, *q, dg, rr, ss)
        assert nl == r.get("reason_no_low_s", r["reason"]), r["tag"]
        bad = r["tag"].endswith("_wrong_r") or r["tag"].startswith("final_infinity")
        assert nl == (O.R_MATH if bad else O.R_OK), r["tag"]
        k = lc.key(None, *q)
        assert k is not None and lc.verify(k, dg, sig) == (nl == O.R_OK), r["tag"]
        lc.free_key(k)
    tags = {r["tag"] for r in recs}
    for t in ("acc_eq_gentry_w0_qG", "acc_eq_gentry_w0_q2G", "final_infinity", "final_infinity_w95",
              "acc_eq_neg_gentry_w0_then_zeros", "u2_one_digit_w95_d15", "u2_eq_nm1",
              "u2_nibbles_ge8", "u2_all_nibbles_8", "u1_zero", "xwrap0", "xwrap0_wrong_r"):
        assert t in tags, t
    for w in (0, 47, 95):
        for name in ("acc_eq_gentry", "acc_eq_neg_gentry"):
            if (w, name) != (95, "acc_eq_neg_gentry"):
                assert any(t.startswith(f"{name}_w{w}_d") for t in tags), (w, name)


def test_keywin_fixture_situations():
    """The records meet the situations their tags name, for the route's walk
    order (Q upwards from an empty accumulator, then G upwards)."""
    def scalars(r):
        _, rr, ss = O.unmarshal_ecdsa_signature(bytes.fromhex(r["sig"]))
        w = pow(ss, -1, N)
        return int(r["digest"], 16) * w % N, rr * w % N
    recs = {r["tag"]: r for r in load_keywin()}
    for tag, r in recs.items():
        u1, u2 = scalars(r)
        Q = (int(r["qx"], 16), int(r["qy"], 16))
        if tag.startswith(("acc_eq_gentry_w", "acc_eq_neg_gentry_w", "final_infinity_w")):
            w = int(tag.split("_w")[1].split("_")[0])
            acc = O.point_add(P384, O.scalar_mult(P384, u2, Q), O.scalar_mult(P384, u1 % 16 ** w, G)) \
                if u1 % 16 ** w else O.scalar_mult(P384, u2, Q)
            ent = O.scalar_mult(P384, ((u1 >> (4 * w)) & 15) * 16 ** w, G)
            assert ent is not None and acc[0] == ent[0]
            assert (acc[1] == ent[1]) == tag.startswith("acc_eq_gentry")
    assert scalars(recs["u2_eq_nm1"])[1] == N - 1
    assert scalars(recs["u1_zero"])[0] == 0
    assert all(c in "89abcdef" for c in "%096x" % scalars(recs["u2_nibbles_ge8"])[1])
    u1, u2 = scalars(recs["xwrap0"])
    assert O.double_scalar(P384, u1, u2, (int(recs["xwrap0"]["qx"], 16),
                                           int(recs["xwrap0"]["qy"], 16)))[0] >= N
    u1, u2 = scalars(recs["final_infinity"])
    q = (int(recs["final_infinity"]["qx"], 16), int(recs["final_infinity"]["qy"], 16))
    assert O.double_scalar(P384, u1, u2, q) is None


@pytest.mark.parametrize("registered", [True, False])
def test_keywin_fixture_through_harness(hk, registered):
    """Digest mode, with and without the low-S rule: the table route gives the
    oracle's reasons, and so does the ladder for the same records."""
    recs = load_keywin()
    keys = valid_keys(recs)
    hk.hs384k_reserve(len(keys))
    if registered:
        assert (register(hk, keys) == 0).all()
    for no_low_s in (False, True):
        want = expect(recs, no_low_s)
        out, route = run_hk(hk, U.pack384(recs, False), _lib.BH_F_NO_LOW_S if no_low_s else 0,
                            chunk=5)
        bad = [(r["tag"], int(o), int(w)) for r, o, w in zip(recs, out, want) if o != w]
        assert not bad
        assert (route == (np.isin(want, (O.R_OK, O.R_MATH)) if registered else 0)).all()


def test_abi_before_any_device():
    """The four symbols exist with their null checks; valid arguments in a
    process that never called bh_init answer BH_E_NOT_INIT; the old registry
    entry points still refuse the curve."""
    L = _lib.lib()
    for s in ("bh_keys384_reserve", "bh_keys384_register", "bh_keys384_clear", "bh_keys384_count"):
        assert hasattr(L, s) and s in _lib.EXPORTS
        assert s in open(os.path.join(ROOT, "include", "bdls_hip.h")).read()
    key = raw(G)
    cnt = ctypes.c_size_t(77)
    assert L.bh_keys384_register(-1, None, 1, None) == BH_E_INVALID and _lib.last_error()
    assert L.bh_keys384_register(0, None, 3, None) == BH_E_INVALID
    assert L.bh_keys384_count(-1, None) == BH_E_INVALID
    assert L.bh_keys384_count(0, None) == BH_E_INVALID
    C = _lib.BH_CURVE_P384
    assert L.bh_keys_reserve(-1, C, 16) == BH_E_INVALID and "P-384" in _lib.last_error()
    assert L.bh_keys_register(-1, C, key, 1, None) == BH_E_INVALID and "P-384" in _lib.last_error()
    assert L.bh_keys_clear(-1, C) == BH_E_INVALID and "P-384" in _lib.last_error()
    assert L.bh_keys_count(-1, C, ctypes.byref(cnt)) == BH_E_INVALID and "P-384" in _lib.last_error()
    code = (
        "import ctypes, json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "L = _lib.lib()\n"
        f"key = bytes.fromhex({key.hex()!r})\n"
        "st = (ctypes.c_uint8 * 1)()\n"
        "cnt = ctypes.c_size_t(5)\n"
        "out = [L.bh_keys384_reserve(d, 8) for d in (-1, 0)]\n"
        "out += [L.bh_keys384_register(d, key, 1, st) for d in (-1, 0)]\n"
        "out += [L.bh_keys384_register(-1, None, 0, None)]\n"
        "out += [L.bh_keys384_clear(d) for d in (-1, 0)]\n"
        "out += [L.bh_keys384_count(d, ctypes.byref(cnt)) for d in (-1, 0)]\n"
        "out += [L.bh_keys384_count(-1, None), L.bh_keys384_register(-1, None, 1, None)]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [BH_E_NOT_INIT] * 9 + [BH_E_INVALID] * 2


def test_csp_register_refuses_other_curves():
    from bdls_amd.bccsp import BCCSPError, ECDSAPublicKey, HipCSP
    csp = HipCSP.__new__(HipCSP)  # no device: the check comes before the library
    with pytest.raises(BCCSPError):
        csp.register_keys_p384([ECDSAPublicKey(O.P256.gx, O.P256.gy)])
    assert len(csp.register_keys_p384([])) == 0
