"""GPU: BH_CURVE_P384 through the C ABI (bh_verify, bh_verify_dev) and HipCSP,
against the fixture tests/golden/p384_vectors.jsonl (oracle expectations) and a
libcrypto-signed batch checked by construction."""
import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from bdls_amd import _lib
from bdls_amd.bccsp import BCCSPError, ECDSAPublicKey, HipCSP, verify_packed
from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests.conftest import ROOT, pack
from tests.p384_util import HALF, N, P, P384

pytestmark = pytest.mark.gpu
C384 = _lib.BH_CURVE_P384


@pytest.fixture(scope="module")
def csp():
    return HipCSP()


@pytest.fixture(scope="module")
def golden384():
    return U.load_golden384()


@pytest.fixture(scope="module")
def batch600():
    """(records, reasons by construction) per hash family, signed once."""
    lc = U.LibCrypto()
    return {fam: U.signed_batch(lc, 600, 24, seed=600, family=fam) for fam in ("SHA2", "SHA3")}


def expect(recs, no_low_s):
    return np.array([r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]
                     for r in recs], np.uint8)


def check(recs, valid, reason, want):
    bad = [(r.get("tag"), int(g), int(w)) for r, g, w in zip(recs, reason, want) if g != w]
    assert not bad, bad[:8]
    assert (valid == (want == 0)).all()


@pytest.mark.parametrize("no_low_s", [False, True])
def test_golden_digest_mode(csp, golden384, no_low_s):
    valid, reason = verify_packed(*U.pack384(golden384, False), curve=C384,
                                  flags=_lib.BH_F_NO_LOW_S if no_low_s else 0)
    check(golden384, valid, reason, expect(golden384, no_low_s))


@pytest.mark.parametrize("no_low_s", [False, True])
@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_golden_fused_mode(csp, golden384, family, no_low_s):
    recs = [r for r in golden384 if r.get("family") == family]
    flags = (_lib.BH_F_HASH_SHA256 if family == "SHA2" else _lib.BH_F_HASH_SHA3_256) | \
        (_lib.BH_F_NO_LOW_S if no_low_s else 0)
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=flags)
    check(recs, valid, reason, expect(recs, no_low_s))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257])
def test_golden_prefixes(csp, golden384, n):
    """Wave and block edges and the bitmap tail (the fixture repeated past its end)."""
    recs = (golden384 * 2)[:n]
    valid, reason = verify_packed(*U.pack384(recs, False), curve=C384)
    assert len(reason) == n
    check(recs, valid, reason, expect(recs, False))


@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_libcrypto_batch(csp, batch600, family):
    recs, want = batch600[family]
    flag = _lib.BH_F_HASH_SHA256 if family == "SHA2" else _lib.BH_F_HASH_SHA3_256
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=flag)
    check(recs, valid, reason, want)


def test_chunk_boundary_child_process(batch600, tmp_path):
    """BH_P384_CHUNK is parsed once per process: a fresh child with chunks of
    128 crosses four boundaries on the 600 records and must give the reasons
    the batch was built with (the unchunked result of test_libcrypto_batch)."""
    recs, want = batch600["SHA2"]
    path = tmp_path / "recs.json"
    path.write_text(json.dumps(recs))
    code = (
        "import json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "from bdls_amd.bccsp import HipCSP, verify_packed\n"
        "from tests import p384_util as U\n"
        f"recs = json.load(open({str(path)!r}))\n"
        "HipCSP()\n"
        "valid, reason = verify_packed(*U.pack384(recs, True), curve=_lib.BH_CURVE_P384,\n"
        "                              flags=_lib.BH_F_HASH_SHA256)\n"
        "print(json.dumps({'reason': reason.tolist(), 'valid': valid.tolist(),\n"
        "                  'stats': list(_lib.device_stats())}))\n")
    env = dict(os.environ, BH_P384_CHUNK="128")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["reason"] == want.tolist()
    assert res["valid"] == (want == 0).tolist()
    assert res["stats"] == [1, len(recs)]  # five chunks, one batch


def test_all_invalid_and_all_bad_key(csp, golden384):
    """130 records none of which reaches the inverse with its own s: the
    chunked inversion must survive chunks with no valid record."""
    base = next(r for r in golden384 if r["tag"] == "high_s")
    recs = [dict(base) for _ in range(130)]
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=_lib.BH_F_HASH_SHA256)
    assert (reason == O.R_HIGH_S).all() and not valid.any()
    ok = next(r for r in golden384 if r["tag"] == "valid_msg_SHA2_len300")
    recs = [dict(ok, qy=U.h48((int(ok["qy"], 16) + 1 + i) % P)) for i in range(130)]
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=_lib.BH_F_HASH_SHA256)
    assert (reason == O.R_BAD_KEY).all() and not valid.any()
    # and one valid record alone among them
    recs[77] = dict(ok)
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=_lib.BH_F_HASH_SHA256)
    assert reason[77] == 0 and valid[77] and valid.sum() == 1 and (np.delete(reason, 77) == 7).all()


def test_verify_dev_resident(csp, golden384):
    n = len(golden384)
    arrs = U.pack384(golden384, False)
    dev = [_lib.DeviceArray.from_numpy(0, a) for a in arrs]
    bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
    rs = _lib.DeviceArray(0, n)
    b = _lib.BhBatch(*[d.ptr for d in dev])
    t = _lib.BhTiming()
    b0, r0 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify_dev(0, C384, ctypes.byref(b), n, 0, bm.ptr, rs.ptr, None, 1,
                                        ctypes.byref(t)))
    b1, r1 = _lib.device_stats()
    assert (b1 - b0, r1 - r0) == (1, n)
    assert t.n_ladder == n and t.n_keycomb == 0 and t.n_keytables == 0
    assert t.prep_ms > 0 and t.inv_ms > 0 and t.build_ladder_ms > 0
    reason = rs.to_numpy(np.uint8, n)
    words = bm.to_numpy(np.uint64, (n + 63) // 64)
    want = expect(golden384, False)
    assert (reason == want).all()
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert (bits == (want == 0)).all()
    # without timing, synchronous; the keep-keys and any-lane flags are ignored
    _lib.check(_lib.lib().bh_verify_dev(0, C384, ctypes.byref(b), n,
                                        _lib.BH_F_KEEP_KEYS | _lib.BH_F_ANY_LANE, bm.ptr, rs.ptr,
                                        None, 1, None))
    assert (rs.to_numpy(np.uint8, n) == want).all()
    # an empty batch zeroes the timing it is given and counts nothing
    t2 = _lib.BhTiming(prep_ms=7.0, n_ladder=9, wide=3)
    b2 = _lib.device_stats()
    _lib.check(_lib.lib().bh_verify_dev(0, C384, ctypes.byref(b), 0, 0, bm.ptr, rs.ptr, None, 1,
                                        ctypes.byref(t2)))
    assert (t2.prep_ms, t2.n_ladder, t2.wide) == (0.0, 0, 0) and _lib.device_stats() == b2
    assert t.wide == 0
    # a host call is one batch, however many chunks it runs in
    valid, reason = verify_packed(*arrs, curve=C384)
    assert _lib.device_stats() == (b2[0] + 1, b2[1] + n) and (reason == want).all()
    for d in dev + [bm, rs]:
        d.free()


def test_isolation_from_p256(csp, golden, golden384):
    """P-256, P-384, P-256 in one process, then two threads alternating the
    curves: the P-256 results stay those of its fixture, bit for bit."""
    a256 = pack(golden, False)
    a384 = U.pack384(golden384, False)
    w256 = np.array([r["reason"] for r in golden], np.uint8)
    w384 = expect(golden384, False)

    def p256():
        valid, reason = verify_packed(*a256)
        return (reason == w256).all() and (valid == (w256 == 0)).all()

    def p384():
        valid, reason = verify_packed(*a384, curve=C384)
        return (reason == w384).all() and (valid == (w384 == 0)).all()

    assert p256() and p384() and p256()
    fails = []

    def worker(first):
        for k in range(4):
            f = p256 if (k + first) % 2 == 0 else p384
            if not f():
                fails.append((first, k))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not fails
    assert p256()


def test_hipcsp_p384(csp, golden384):
    ok = next(r for r in golden384 if r["tag"] == "digest_len48")
    k = ECDSAPublicKey(int(ok["qx"], 16), int(ok["qy"], 16), curve="P-384")
    sig, dg = bytes.fromhex(ok["sig"]), bytes.fromhex(ok["digest"])
    assert csp.verify(k, sig, dg) is True
    assert csp.verify(k, sig, dg[:-1] + bytes([dg[-1] ^ 1])) is False
    _, r, s = O.unmarshal_ecdsa_signature(sig)
    with pytest.raises(BCCSPError) as ei:
        csp.verify(k, O.marshal_ecdsa_signature(r, N - s), dg)
    assert ei.value.reason == O.R_HIGH_S and f"[{HALF}]" in str(ei.value)
    m = next(r for r in golden384 if r["tag"] == "valid_msg_SHA3_len137")
    km = ECDSAPublicKey(int(m["qx"], 16), int(m["qy"], 16), curve="P-384")
    assert csp.identity_verify(km, bytes.fromhex(m["msg"]), bytes.fromhex(m["sig"]), "SHA3") is None
    with pytest.raises(BCCSPError):
        csp.identity_verify(km, bytes.fromhex(m["msg"]) + b"x", bytes.fromhex(m["sig"]), "SHA3")
    valid, reason = csp.batch_verify([k, k], [sig, sig[:-1]], [dg, dg])
    assert valid.tolist() == [True, False] and reason.tolist() == [0, O.R_DER]
    valid, _ = csp.batch_identity_verify([km], [bytes.fromhex(m["msg"])], [bytes.fromhex(m["sig"])],
                                         "SHA3")
    assert valid.tolist() == [True]
    k256 = ECDSAPublicKey(O.P256.gx, O.P256.gy)
    with pytest.raises(BCCSPError):
        csp.batch_verify([k, k256], [sig, sig], [dg, dg])
