"""GPU: BH_F_HASH_SHA384 / BH_F_HASH_SHA512 through bh_verify and bh_verify_dev
on both NIST curves (by-construction batches, tests/sha2wide_util.py), the
chunked digest buffer in a child process, bh_verify_x509_ex on the fixture
tests/golden/x509_p384_vectors.json, and the Python mirror."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from bdls_amd.bccsp import (BCCSPError, ECDSAPublicKey, HipCSP, verify_packed,
                            x509_check_signatures)
from oracle import ecdsa_ref as O
from tests import sha2wide_util as W
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
N = 257  # the smallest batch that crosses a 64-lane wave and a 256-thread block
COMBOS = [(c, h) for c in ("P-384", "P-256") for h in ("SHA384", "SHA512")]


@pytest.fixture(scope="module")
def csp():
    return HipCSP()


@pytest.fixture(scope="module")
def batches():
    """(records, reasons, reasons without low-S) per (curve, hash), signed once;
    every corrupted record and every 16th other one is put to the oracle."""
    lc = W.LibCrypto()
    out = {}
    for curve, h in COMBOS:
        recs, want, nls = W.signed_batch(curve, h, lc, n=N, nkeys=12)
        c = W.CURVES[curve][0]
        for i in [i for i in range(N) if i % 8 == 3 or i % 16 == 0]:
            r = recs[i]
            assert bytes.fromhex(r["digest"]) == W.HASHES[h][0](bytes.fromhex(r["msg"])).digest()
            got = O.csp_verify(c, int(r["qx"], 16), int(r["qy"], 16), bytes.fromhex(r["sig"]),
                               bytes.fromhex(r["digest"]))
            assert got == (want[i] == 0, want[i]), (curve, h, i)
        assert (want != 0).sum() == len(range(3, N, 8)) and (nls != want).any()
        out[curve, h] = (recs, want, nls)
    return out


@pytest.fixture(scope="module")
def vectors():
    return W.load_x509_vectors()


def check(valid, reason, want):
    bad = [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(reason, want)) if g != w]
    assert not bad, bad[:8]
    assert (valid == (want == 0)).all()


@pytest.mark.parametrize("curve,h", COMBOS)
def test_bh_verify(csp, batches, curve, h):
    recs, want, nls = batches[curve, h]
    cid, flag = W.CURVES[curve][1], W.HASHES[h][1]
    arrs = W.pack_records(recs)
    b0 = _lib.device_stats()
    valid, reason = verify_packed(*arrs, curve=cid, flags=flag)
    assert _lib.device_stats() == (b0[0] + 1, b0[1] + N)
    check(valid, reason, want)
    valid, reason = verify_packed(*arrs, curve=cid, flags=flag | _lib.BH_F_NO_LOW_S)
    check(valid, reason, nls)


@pytest.mark.parametrize("curve,h", COMBOS)
def test_bh_verify_dev(csp, batches, curve, h):
    recs, want, nls = batches[curve, h]
    cid, flag = W.CURVES[curve][1], W.HASHES[h][1]
    dev = [_lib.DeviceArray.from_numpy(0, a) for a in W.pack_records(recs)]
    bm = _lib.DeviceArray(0, 8 * ((N + 63) // 64))
    rs = _lib.DeviceArray(0, N)
    b = _lib.BhBatch(*[d.ptr for d in dev])
    t = _lib.BhTiming()
    b0 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify_dev(0, cid, ctypes.byref(b), N, flag, bm.ptr, rs.ptr, None, 1,
                                        ctypes.byref(t)))
    assert _lib.device_stats() == (b0[0] + 1, b0[1] + N)
    assert t.prep_ms > 0 and t.inv_ms > 0
    reason = rs.to_numpy(np.uint8, N)
    words = bm.to_numpy(np.uint64, (N + 63) // 64)
    check(np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool), reason, want)
    # without the low-S rule, no timing; the keep-keys and any-lane flags are ignored
    _lib.check(_lib.lib().bh_verify_dev(0, cid, ctypes.byref(b), N,
                                        flag | _lib.BH_F_NO_LOW_S | _lib.BH_F_KEEP_KEYS |
                                        _lib.BH_F_ANY_LANE, bm.ptr, rs.ptr, None, 1, None))
    reason = rs.to_numpy(np.uint8, N)
    words = bm.to_numpy(np.uint64, (N + 63) // 64)
    check(np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool), reason, nls)
    # an empty batch zeroes the timing it is given and counts nothing
    t2 = _lib.BhTiming(prep_ms=7.0, n_ladder=9)
    b2 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify_dev(0, cid, ctypes.byref(b), 0, flag, bm.ptr, rs.ptr, None, 1,
                                        ctypes.byref(t2)))
    assert (t2.prep_ms, t2.n_ladder) == (0.0, 0) and _lib.device_stats() == b2
    for d in dev + [bm, rs]:
        d.free()


def test_chunked_digest_buffer_child_process(batches, tmp_path):
    """BH_P384_CHUNK is parsed once per process: a fresh child with chunks of
    64 runs the first 200 P-384 + SHA-384 records in four passes over one
    digest buffer, then the prefixes around one chunk."""
    recs, want, _ = batches["P-384", "SHA384"]
    path = tmp_path / "recs.json"
    path.write_text(json.dumps(recs[:200]))
    code = (
        "import json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "from bdls_amd.bccsp import HipCSP, verify_packed\n"
        "from tests import sha2wide_util as W\n"
        f"recs = json.load(open({str(path)!r}))\n"
        "HipCSP()\n"
        "out = {}\n"
        "for n in (200, 0, 1, 63, 64, 65):\n"
        "    b0 = _lib.device_stats()\n"
        "    valid, reason = verify_packed(*W.pack_records(recs[:n]), curve=_lib.BH_CURVE_P384,\n"
        "                                  flags=_lib.BH_F_HASH_SHA384)\n"
        "    b1 = _lib.device_stats()\n"
        "    out[n] = {'reason': reason.tolist(), 'valid': valid.tolist(),\n"
        "              'stats': [b1[0] - b0[0], b1[1] - b0[1]]}\n"
        "print(json.dumps(out))\n")
    env = dict(os.environ, BH_P384_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for n in (200, 0, 1, 63, 64, 65):
        got = res[str(n)]
        assert got["reason"] == want[:n].tolist(), n
        assert got["valid"] == (want[:n] == 0).tolist(), n
        assert got["stats"] == ([1, n] if n else [0, 0]), n  # one batch, however many chunks


def _x509_ex(vecs):
    certs, off, ln, pub, pub_off, curve = W.pack_x509(vecs)
    n = len(vecs)
    bm = np.zeros((n + 7) // 8, np.uint8)
    rs = np.full(n, 255, np.uint8)
    _lib.check(_lib.lib().bh_verify_x509_ex(certs.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                            pub.ctypes.data, pub_off.ctypes.data, curve.ctypes.data,
                                            n, bm.ctypes.data, rs.ctypes.data))
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool), rs


def test_x509_ex_fixture(csp, vectors):
    """The whole fixture in one call; the generator's order already mixes the
    curves, and a second call interleaves them record by record."""
    bits, rs = _x509_ex(vectors)
    bad = [(v["tag"], int(g), v["reason"]) for v, g in zip(vectors, rs) if g != v["reason"]]
    assert not bad, bad[:5]
    assert (bits == np.array([v["reason"] == 0 for v in vectors])).all()
    p256 = [v for v in vectors if v["curve"] == "P-256"]
    p384 = [v for v in vectors if v["curve"] == "P-384"]
    mixed = [v for pair in zip(p256, p384) for v in pair]
    assert len(mixed) > 100
    bits, rs = _x509_ex(mixed)
    assert rs.tolist() == [v["reason"] for v in mixed]
    assert (bits == np.array([v["reason"] == 0 for v in mixed])).all()


def test_x509_plain_still_reports_unsupported(csp, vectors):
    """bh_verify_x509 does not change: ecdsa-with-SHA384 / -SHA512 certificates are reason 11."""
    vecs = [v for v in vectors if W.cert_hash(bytes.fromhex(v["cert"])) in ("SHA384", "SHA512")]
    assert sum(v["reason"] == 0 for v in vecs) >= 24
    certs, off, ln = W.pack_bytes([bytes.fromhex(v["cert"]) for v in vecs])
    pub = np.frombuffer(b"".join(bytes.fromhex(v["qx"] + v["qy"])[:64] for v in vecs), np.uint8)
    n = len(vecs)
    bm = np.full((n + 7) // 8, 255, np.uint8)
    rs = np.zeros(n, np.uint8)
    _lib.check(_lib.lib().bh_verify_x509(certs.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                         pub.ctypes.data, n, bm.ctypes.data, rs.ctypes.data))
    assert (rs == 11).all() and not bm.any()


def test_python_mirror(csp, batches, vectors):
    recs, want, _ = batches["P-384", "SHA384"]
    r = recs[0]
    assert want[0] == 0
    k = ECDSAPublicKey(int(r["qx"], 16), int(r["qy"], 16), curve="P-384")
    sig = bytes.fromhex(r["sig"])  # record 0 signs the empty message
    r1 = recs[1]  # a one-byte message: its bit-flipped twin must not verify
    k1 = ECDSAPublicKey(int(r1["qx"], 16), int(r1["qy"], 16), curve="P-384")
    m1, s1 = bytes.fromhex(r1["msg"]), bytes.fromhex(r1["sig"])
    valid, reason = csp.batch_identity_verify([k, k1, k1], [bytes.fromhex(r["msg"]), m1,
                                                            bytes([m1[0] ^ 1])],
                                              [sig, s1, s1], hash="SHA384")
    assert valid.tolist() == [True, True, False] and reason.tolist() == [0, 0, O.R_MATH]
    assert csp.identity_verify(k1, m1, s1, hash="SHA384") is None
    with pytest.raises(BCCSPError):
        csp.identity_verify(k1, bytes([m1[0] ^ 1]), s1, hash="SHA384")
    with pytest.raises(BCCSPError):
        csp.batch_identity_verify([k1], [m1], [s1], hash="SHA1")
    vecs = vectors[:12]
    keys = [ECDSAPublicKey(int(v["qx"], 16), int(v["qy"], 16), curve=v["curve"]) for v in vecs]
    valid, reason = x509_check_signatures([bytes.fromhex(v["cert"]) for v in vecs], keys)
    assert reason.tolist() == [v["reason"] for v in vecs]
    assert valid.tolist() == [v["reason"] == 0 for v in vecs]
