"""BH_F_HASH_SHA384 / BH_F_HASH_SHA512 and bh_verify_x509_ex without a GPU:
the BH_HD code of bdls_amd/csrc/sha512.h through the host harness
(tests/native_sha512/hostsim_sha512.cpp) against hashlib, the sanitizer
self-test program (where "no byte outside the message is read" is shown), the
fixture tests/golden/x509_p384_vectors.json against the test-side reference
and libcrypto, and the refusals the C ABI makes before it looks for a device.
A missing harness FAILS these tests: `make` builds it."""
import ctypes
import hashlib
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from oracle import ecdsa_ref as O
from tests import sha2wide_util as W

FIPS_ABC = b"abc"
FIPS_TWO_BLOCK = (b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmno"
                  b"ijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu")


@pytest.fixture(scope="module")
def hs():
    assert os.path.exists(W.HOSTSIM512), "tests/native/build/libhostsim512.so is not built (make)"
    L = ctypes.CDLL(W.HOSTSIM512)
    for f in (L.hs_sha384, L.hs_sha512):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        f.restype = None
    L.hs_sha512_block.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.hs_sha512_block.restype = None
    return L


@pytest.fixture(scope="module")
def vectors():
    return W.load_x509_vectors()


def _digests(hs, msg: bytes, align: int = 0):
    """(SHA-384, SHA-512) of msg by the harness, msg placed at an address = align mod 8."""
    buf = np.zeros(len(msg) + 16, np.uint8)
    at = (align - buf.ctypes.data) % 8
    buf[at:at + len(msg)] = np.frombuffer(msg, np.uint8)
    o48, o64 = np.zeros(48, np.uint8), np.zeros(64, np.uint8)
    p = buf.ctypes.data + at if msg else None  # the empty message: a null pointer
    hs.hs_sha384(p, len(msg), o48.ctypes.data)
    hs.hs_sha512(p, len(msg), o64.ctypes.data)
    return o48.tobytes(), o64.tobytes()


def test_fips_vectors(hs):
    # FIPS 180-4 examples (SHA-384 / SHA-512 of "abc" and of the 896-bit message)
    d48, d64 = _digests(hs, FIPS_ABC)
    assert d48.hex().startswith("cb00753f45a35e8bb5a03d699ac65007272c32ab0eded163")
    assert d64.hex().startswith("ddaf35a193617abacc417349ae20413112e6fa4e89a97ea2")
    for m in (FIPS_ABC, FIPS_TWO_BLOCK):
        assert _digests(hs, m) == (hashlib.sha384(m).digest(), hashlib.sha512(m).digest())
    assert _digests(hs, FIPS_TWO_BLOCK)[1].hex().startswith("8e959b75dae313da8cf4f72814fc143f")


def test_every_length_and_alignment(hs):
    """0..300 covers 111 / 112 / 113 (the last length whose padding fits one
    block and the first that spills), 127 / 128 / 129 and 239 / 240 / 241 (the
    same edges of the second block)."""
    rng = np.random.default_rng(512)
    data = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    bad = []
    for n in range(301):
        want = (hashlib.sha384(data[:n]).digest(), hashlib.sha512(data[:n]).digest())
        for a in range(8):
            if _digests(hs, data[:n], a) != want:
                bad.append((n, a))
    assert not bad, bad[:8]


def test_long_message(hs):
    m = np.random.default_rng(10000).integers(0, 256, 10000, dtype=np.uint8).tobytes()
    for a in (0, 3):
        assert _digests(hs, m, a) == (hashlib.sha384(m).digest(), hashlib.sha512(m).digest())


def test_compression_function_alone(hs):
    """hs_sha512_block on a hand-fed block: "abc", 0x80, zeros, bit length 24,
    from SHA-512's and from SHA-384's initial value."""
    w = np.zeros(16, np.uint64)
    w[0], w[15] = 0x6162638000000000, 24
    iv512 = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
             0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]
    iv384 = [0xcbbb9d5dc1059ed8, 0x629a292a367cd507, 0x9159015a3070dd17, 0x152fecd8f70e5939,
             0x67332667ffc00b31, 0x8eb44a8768581511, 0xdb0c2e0d64f98fa7, 0x47b5481dbefa4fa4]
    for iv, want in ((iv512, hashlib.sha512(b"abc").digest()), (iv384, hashlib.sha384(b"abc").digest())):
        h = np.array(iv, np.uint64)
        hs.hs_sha512_block(h.ctypes.data, w.ctypes.data)
        got = b"".join(int(x).to_bytes(8, "big") for x in h)
        assert got[:len(want)] == want
    assert int(w[0]) == 0x6162638000000000  # the caller's block is not written


def test_sanitizer_selftest_program():
    """The stand-alone program (address + undefined-behaviour sanitizers, its own
    main) builds, runs and exits 0: every length 0..300 at every alignment from
    a heap allocation that ends with the message."""
    b = subprocess.run(["make", "-C", W.ROOT, os.path.relpath(W.SELFTEST, W.ROOT)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([W.SELFTEST], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


def test_fixture_conditions(vectors):
    ok = Counter((v["curve"], W.cert_hash(bytes.fromhex(v["cert"]))) for v in vectors
                 if v["reason"] == 0)
    assert set(ok) == {(c, h) for c in W.CURVES for h in W.HASHES}
    assert min(ok.values()) >= 6, ok
    assert {v["reason"] for v in vectors} >= {0, 3, 4, 5, 7, 8, 9, 10, 11}
    assert os.path.getsize(W.X509_P384) <= os.path.getsize(
        os.path.join(W.ROOT, "tests", "golden", "x509_vectors.json"))


def test_fixture_matches_reference(vectors):
    bad = [v["tag"] for v in vectors
           if W.check_signature_from_ex(bytes.fromhex(v["cert"]), W.CURVES[v["curve"]][0],
                                        int(v["qx"], 16), int(v["qy"], 16)) != v["reason"]]
    assert not bad, bad[:5]


def test_fixture_against_libcrypto(vectors):
    """Every vector the engine must decide by arithmetic (BH_R_OK or BH_R_MATH),
    none skipped: P-384 issuers through libcrypto's ECDSA_verify, P-256 ones
    through the oracle library's OpenSSL core, the digest truncated to the
    order's bytes as Go's hashToNat does and (P-256: the sw provider's Verify)
    s folded low, which verifies identically."""
    from oracle import orc
    from oracle import x509_ref as X
    lc = W.LibCrypto()
    checked = Counter()
    for v in vectors:
        if v["reason"] not in (O.R_OK, O.R_MATH):
            continue
        der = bytes.fromhex(v["cert"])
        name = W.cert_hash(der)
        assert name is not None, v["tag"]
        tbs, _, _, sig = X.split_cert(der)
        r, s = X.parse_signature(sig)
        dg = W.HASHES[name][0](tbs).digest()
        qx, qy = int(v["qx"], 16), int(v["qy"], 16)
        if v["curve"] == "P-384":
            k = lc.key(None, qx, qy)
            assert k is not None, v["tag"]
            got = lc.verify(k, dg[:48], O.marshal_ecdsa_signature(r, s))
            lc.free_key(k)
        else:
            n = O.P256.n
            low = O.marshal_ecdsa_signature(r, min(s, n - s))
            got = orc.csp_verify(bytes.fromhex(v["qx"] + v["qy"]), low, dg[:32]) == 0
        assert got == (v["reason"] == O.R_OK), v["tag"]
        checked[(v["curve"], v["reason"])] += 1
    want = Counter((v["curve"], v["reason"]) for v in vectors if v["reason"] in (O.R_OK, O.R_MATH))
    assert checked == want and len(checked) == 4, checked


# ---- refusals made before any device is looked for (this process never calls bh_init)
@pytest.fixture(scope="module")
def abi():
    from bdls_amd import _lib
    return _lib, _lib.lib()


def _dummy(_lib):
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    return buf, p, _lib.BhBatch(*([p] * 7))


def test_hash_flags_are_exclusive(abi):
    _lib, L = abi
    buf, p, b = _dummy(_lib)
    hashes = (_lib.BH_F_HASH_SHA256, _lib.BH_F_HASH_SHA3_256, _lib.BH_F_HASH_SHA384,
              _lib.BH_F_HASH_SHA512)
    for i, f in enumerate(hashes):
        for g in hashes[i + 1:]:
            for curve in (_lib.BH_CURVE_P256, _lib.BH_CURVE_P384):
                assert L.bh_verify(curve, ctypes.byref(b), 1, f | g, p, p) == -1, (f, g)
                assert "exclusive" in _lib.last_error()
                assert L.bh_verify_dev(0, curve, ctypes.byref(b), 1, f | g, p, p, None, 1,
                                       None) == -1, (f, g)
                assert "exclusive" in _lib.last_error()
    # 0x100 stays unknown to callers
    assert L.bh_verify(0, ctypes.byref(b), 1, 0x100 | _lib.BH_F_HASH_SHA384, p, p) == -1
    assert "unknown flag" in _lib.last_error()


@pytest.mark.parametrize("flag_name", ["BH_F_HASH_SHA384", "BH_F_HASH_SHA512"])
def test_other_entry_points_refuse_by_name(abi, flag_name):
    _lib, L = abi
    flag = getattr(_lib, flag_name)
    buf, p, b = _dummy(_lib)
    cb = _lib.BhCBatch(p, None, 1, p, p, p, p, 0)
    ptrs = np.full(4, p, np.uint64)
    pb = _lib.BhPBatch(p, ptrs.ctypes.data, p, ptrs.ctypes.data, p)
    job = ctypes.c_void_p()
    calls = {
        "bh_verify_2seg": lambda: L.bh_verify_2seg(0, ctypes.byref(b), p, p, 1, flag, p, p),
        "bh_verify_submit": lambda: L.bh_verify_submit(0, ctypes.byref(b), 1, flag, p, p,
                                                       ctypes.byref(job)),
        "bh_verify_compact": lambda: L.bh_verify_compact(0, ctypes.byref(cb), 1, flag, p, p),
        "bh_verify_compact_submit": lambda: L.bh_verify_compact_submit(
            0, ctypes.byref(cb), 1, flag, p, p, ctypes.byref(job)),
        "bh_batch_verify": lambda: L.bh_batch_verify(0, ctypes.byref(b), 1, flag, p, p),
        "bh_batch_verify_submit": lambda: L.bh_batch_verify_submit(0, ctypes.byref(b), 1, flag, p, p,
                                                                   ctypes.byref(job)),
        "bh_batch_verify_ptrs": lambda: L.bh_batch_verify_ptrs(0, ctypes.byref(pb), 1, flag, p, p),
        "bh_batch_verify_ptrs_submit": lambda: L.bh_batch_verify_ptrs_submit(
            0, ctypes.byref(pb), 1, flag, p, p, ctypes.byref(job)),
    }
    for name, call in calls.items():
        assert call() == -1, name  # BH_E_INVALID
        err = _lib.last_error()
        assert flag_name in err and "not supported" in err, (name, err)
        assert not job.value, name


def test_x509_ex_refuses_other_curves(abi, vectors):
    _lib, L = abi
    certs, off, ln, pub, pub_off, curve = W.pack_x509(vectors[:4])
    bm, rs = np.zeros(1, np.uint8), np.zeros(4, np.uint8)
    for bad in (1, 7):  # BH_CURVE_SECP256K1, an unknown curve
        cv = curve.copy()
        cv[2] = bad
        assert L.bh_verify_x509_ex(certs.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                   pub.ctypes.data, pub_off.ctypes.data, cv.ctypes.data, 4,
                                   bm.ctypes.data, rs.ctypes.data) == -1
        assert "issuer_curve" in _lib.last_error()


def test_python_mirror_constants_and_hash():
    from bdls_amd import _lib, bccsp
    assert (_lib.BH_F_HASH_SHA384, _lib.BH_F_HASH_SHA512) == (32, 64)
    assert bccsp.hash_flag("SHA384") == 32 and bccsp.hash_flag("SHA512") == 64
    with pytest.raises(bccsp.BCCSPError):
        bccsp.hash_flag("SHA1")
    # HipCSP.hash is host-side: no device needed for the method itself
    h = bccsp.HipCSP.hash(None, b"abc", bccsp.SHA384Opts())
    assert h == hashlib.sha384(b"abc").digest()
    assert bccsp.HipCSP.hash(None, b"abc") == hashlib.sha256(b"abc").digest()
