"""CPU: mixed P-256 / P-384 batches and P-384 identities in the Fabric callers.

* two-span fused hashing in the P-384 pass (verify384.h stage384_prep), run on
  the host by the TEST-ONLY harness tests/native_p384seg/hostsim384_seg.cpp;
* bh_verify_mixed's argument checks (no device needed);
* the identity layer's decode against the oracle with its key extraction
  restated for both curves (tests/mixed_util.py), and the generator's P-384
  orgs against that oracle;
* the generator's default blocks, byte for byte.
A missing harness FAILS these tests: `make` builds it."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib, fabric
from bdls_amd.workload import fabric as F
from oracle import ecdsa_ref as O
from oracle import fabric_ref as R
from tests import mixed_util as M
from tests import p384_util as U
from tests.conftest import ROOT

HOSTSIM384S = os.path.join(ROOT, "tests", "native", "build", "libhostsim384s.so")
BH_E_INVALID, BH_E_NOT_INIT = -1, -2
FLAG = {"SHA2": _lib.BH_F_HASH_SHA256, "SHA3": _lib.BH_F_HASH_SHA3_256}


@pytest.fixture(scope="module")
def hs():
    assert os.path.exists(HOSTSIM384S), "tests/native/build/libhostsim384s.so is not built (make)"
    L = ctypes.CDLL(HOSTSIM384S)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.hs384s_verify.argtypes = [vp] * 9 + [u32] * 3 + [vp]
    return L


def run_hs(hs, arrs, flags, chunk=7):
    """arrs: build_mixed's tuple (every record P-384)."""
    _, pub, _, sig, so, sl, msg, mo, ml, mo2, ml2 = arrs
    n = len(sl)
    out = np.full(n, 255, np.uint8)
    hs.hs384s_verify(pub.ctypes.data, sig.ctypes.data, so.ctypes.data, sl.ctypes.data,
                     msg.ctypes.data, mo.ctypes.data, ml.ctypes.data,
                     None if mo2 is None else mo2.ctypes.data,
                     None if ml2 is None else ml2.ctypes.data, n, flags, chunk, out.ctypes.data)
    return out


def _signed_by_length(family):
    """One libcrypto-signed P-384 record per length of SEAM_LENGTHS over the
    family's 32-byte hash; every third one has a message bit flipped after
    signing (BH_R_MATH), so a wrong hash cannot hide behind a reject."""
    lc = U.LibCrypto()
    rng = random.Random(3840 + len(family))
    d = rng.randrange(1, U.N)
    qx, qy = O.pubkey(U.P384, d)
    k = lc.key(d, qx, qy)
    recs = []
    for j, L in enumerate(M.SEAM_LENGTHS):
        msg = bytes(rng.getrandbits(8) for _ in range(L))
        r, s = lc.sign(k, U.family_hash(family, msg))
        if s > U.HALF:
            s = U.N - s
        want = O.R_OK
        if j % 3 == 2 and L:
            b = bytearray(msg)
            b[rng.randrange(L)] ^= 1 << rng.randrange(8)
            msg, want = bytes(b), O.R_MATH
        recs.append({"qx": U.h48(qx), "qy": U.h48(qy), "msg": msg.hex(), "curve": 2,
                     "sig": O.marshal_ecdsa_signature(r, s).hex(), "reason": want})
    lc.free_key(k)
    return recs


@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_two_span_equals_one_span_at_every_seam(hs, family):
    """For every length of SEAM_LENGTHS and every seam 0..len (a first span of
    length 0 with a non-empty second one included), the pass over
    msg[:k] || msg[k:] gives the one-span result of the concatenation."""
    base = _signed_by_length(family)
    one = run_hs(hs, M.build_mixed(base, False), FLAG[family])
    assert list(one) == [r["reason"] for r in base]
    assert O.R_OK in one and O.R_MATH in one
    recs, want = [], []
    for r, w in zip(base, one):
        for k in range(len(r["msg"]) // 2 + 1):
            recs.append(r)
            want.append(w)
    assert len(recs) == sum(L + 1 for L in M.SEAM_LENGTHS)
    curve, pub, pub_off, sig, so, sl, _, _, _, _, _ = M.build_mixed(recs, False)
    buf, mo, ml, mo2, ml2 = bytearray(), [], [], [], []
    k = 0
    for i, r in enumerate(recs):
        m = bytes.fromhex(r["msg"])
        k = 0 if (i == 0 or recs[i - 1] is not r) else k + 1
        mo2.append(len(buf))          # the second span first, apart from the first
        buf += m[k:] + b"\xee" * 3
        mo.append(len(buf))
        buf += m[:k] + b"\x77"
        ml.append(k)
        ml2.append(len(m) - k)
    assert any(a == 0 and b > 0 for a, b in zip(ml, ml2))
    msg = np.frombuffer(bytes(buf) + b"\0", np.uint8)
    arrs = (curve, pub, pub_off, sig, so, sl, msg, np.array(mo, np.uint64), np.array(ml, np.uint32),
            np.array(mo2, np.uint64), np.array(ml2, np.uint32))
    two = run_hs(hs, arrs, FLAG[family], chunk=16)
    bad = [(ml[i], ml2[i], int(two[i]), int(want[i])) for i in range(len(recs)) if two[i] != want[i]]
    assert not bad, bad[:10]


@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_golden_fused_records_cut_at_seams(hs, family):
    recs = [dict(r, curve=2) for r in U.load_golden384() if r.get("family") == family]
    assert len(recs) >= 11
    seams = {M.seam_of(i, len(r["msg"]) // 2) for i, r in enumerate(recs)}
    assert len(seams) > 5
    for no_low_s in (False, True):
        want = [M.expect(r, no_low_s) for r in recs]
        fl = FLAG[family] | (_lib.BH_F_NO_LOW_S if no_low_s else 0)
        for two in (False, True):
            out = run_hs(hs, M.build_mixed(recs, two), fl)
            assert list(out) == want, [r["tag"] for r, o, w in zip(recs, out, want) if o != w]


def test_digest_mode_ignores_second_spans(hs):
    recs = [dict(r, curve=2) for r in U.load_golden384()]
    arrs = list(M.build_mixed(recs, False, fused=False))
    n = len(recs)
    arrs[9] = np.full(n, 1, np.uint64)
    arrs[10] = np.full(n, 5, np.uint32)  # non-empty second spans over the first bytes
    for no_low_s in (False, True):
        out = run_hs(hs, arrs, _lib.BH_F_NO_LOW_S if no_low_s else 0)
        want = [M.expect(r, no_low_s) for r in recs]
        assert list(out) == want


# ---------------------------------------------------------------- bh_verify_mixed, no device
def _mb(n=1, **over):
    """A well-formed bh_mbatch of n records (arrays kept alive in the result)."""
    a = dict(curve=np.zeros(n, np.uint8), pub=np.zeros(96 * n + 1, np.uint8),
             pub_off=np.arange(n, dtype=np.uint64) * 96, sig=np.zeros(8, np.uint8),
             sig_off=np.zeros(n, np.uint64), sig_len=np.ones(n, np.uint32),
             msg=np.zeros(64, np.uint8), msg_off=np.zeros(n, np.uint64),
             msg_len=np.full(n, 32, np.uint32), msg2_off=None, msg2_len=None)
    a.update(over)
    b = _lib.BhMBatch(*[None if a[f] is None else a[f].ctypes.data for f, _ in _lib.BhMBatch._fields_])
    return b, a


def test_verify_mixed_argument_checks():
    L = _lib.lib()
    assert hasattr(L, "bh_verify_mixed") and "bh_verify_mixed" in _lib.EXPORTS
    assert "bh_verify_mixed" in open(os.path.join(ROOT, "include", "bdls_hip.h")).read()
    bm, rs = np.zeros(8, np.uint8), np.zeros(8, np.uint8)

    def call(b, n, flags, bitmap=bm, reason=rs):
        return L.bh_verify_mixed(ctypes.byref(b[0]), n, flags,
                                 None if bitmap is None else bitmap.ctypes.data,
                                 None if reason is None else reason.ctypes.data)

    def invalid(b, n, flags, *words, **kw):
        assert call(b, n, flags, **kw) == BH_E_INVALID
        err = _lib.last_error()
        assert all(w in err for w in words), err

    fused = _lib.BH_F_HASH_SHA256
    for bad in (1, 3, 255):  # secp256k1's number is not a curve of this entry point either
        invalid(_mb(3, curve=np.array([0, 2, bad], np.uint8)), 3, 0, "curve[2]", str(bad))
    invalid(_mb(), 1, _lib.BH_F_HASH_SHA384, "BH_F_HASH_SHA384", "bh_verify_mixed")
    invalid(_mb(), 1, _lib.BH_F_HASH_SHA512, "BH_F_HASH_SHA512", "bh_verify_mixed")
    z64, z32 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    invalid(_mb(msg2_off=z64), 1, fused, "msg2_off", "msg2_len")
    invalid(_mb(msg2_len=z32), 1, fused, "msg2_off", "msg2_len")
    invalid(_mb(msg2_off=z64, msg2_len=z32), 1, 0, "BH_F_HASH_SHA256")
    invalid(_mb(msg2_off=z64, msg2_len=z32), 1, _lib.BH_F_NO_LOW_S, "BH_F_HASH_SHA256")
    for f in ("curve", "pub", "pub_off", "sig_off", "sig_len", "msg_off", "msg_len"):
        invalid(_mb(**{f: None}), 1, 0, "null")
    invalid(_mb(), 1, 0, "null", bitmap=None)
    invalid(_mb(), 1, 0, "null", reason=None)
    assert L.bh_verify_mixed(None, 0, 0, None, None) == BH_E_INVALID
    invalid(_mb(), 1, 1 << 20, "flag")
    invalid(_mb(), 1, _lib.BH_F_HASH_SHA256 | _lib.BH_F_HASH_SHA3_256, "exclusive")
    # n == 0: nothing to do, before or after bh_init, null arrays allowed
    empty = _lib.BhMBatch()
    assert L.bh_verify_mixed(ctypes.byref(empty), 0, fused, None, None) == 0
    # valid arguments in a process that never called bh_init
    code = (
        "import ctypes, json, sys\n"
        "sys.path.insert(0, '.')\n"
        "import numpy as np\n"
        "from bdls_amd import _lib\n"
        "from tests.test_mixed_cpu import _mb\n"
        "L = _lib.lib()\n"
        "bm, rs = np.zeros(8, np.uint8), np.zeros(8, np.uint8)\n"
        "out = []\n"
        "for c in (0, 2):\n"
        "    b = _mb(2, curve=np.array([c, 0], np.uint8))\n"
        "    out.append(L.bh_verify_mixed(ctypes.byref(b[0]), 2, 0, bm.ctypes.data, rs.ctypes.data))\n"
        "b = _mb(1, curve=np.array([7], np.uint8))\n"
        "out.append(L.bh_verify_mixed(ctypes.byref(b[0]), 1, 0, bm.ctypes.data, rs.ctypes.data))\n"
        "out.append(L.bh_verify_mixed(ctypes.byref(_lib.BhMBatch()), 0, 0, None, None))\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [BH_E_NOT_INIT, BH_E_NOT_INIT,
                                                             BH_E_INVALID, 0]


def test_pack_records_still_refuses_mixed_curves():
    from bdls_amd.bccsp import BCCSPError, ECDSAPublicKey, pack_records
    ks = [ECDSAPublicKey(O.P256.gx, O.P256.gy), ECDSAPublicKey(U.P384.gx, U.P384.gy, "P-384")]
    with pytest.raises(BCCSPError):
        pack_records(ks, [b"\x30\x00"] * 2, [b"m"] * 2)


# ---------------------------------------------------------------- identities
def _got(t):
    return (t.status, t.creator, t.endorse, t.valid_endorsers)


def _want(fb, i):
    return (fb.tx_status[i], fb.tx_creator[i], fb.tx_endorse[i], fb.tx_valid_identities[i])


@pytest.fixture(scope="module")
def mixed_classes_block():
    return F.generate_fabric_block(ntx=2 * len(F.CORRUPTIONS), classes=F.CORRUPTIONS,
                                   p384_orgs=2, norgs=4)


def _creators(block):
    """Per transaction: the creator's SerializedIdentity bytes, or None."""
    out = []
    for d in R.unmarshal(block, R.BLOCK_SPEC)["data"]["data"]:
        try:
            env = R.unmarshal(d, R.ENVELOPE_SPEC)
            pl = R.unmarshal(env["payload"] or b"", R.PAYLOAD_SPEC)
            sh = R.unmarshal(pl["header"]["signature_header"] or b"", R.SIGNATURE_HEADER_SPEC)
            out.append(sh["creator"])
        except (R.DecodeError, TypeError):
            out.append(None)
    return out


def test_decode_only_resolves_p384_identities(mixed_classes_block, monkeypatch):
    fb = mixed_classes_block
    assert len(fb.p384_keys) >= 20
    M.patch_oracle(monkeypatch)
    py = R.validate_block(fb.block, None, decode_only=True)
    cc = fabric.block_preverify(fb.block, decode_only=True)
    assert [_got(o) for o in py] == [_got(o) for o in cc]
    p384_ser = {i.serialized for i in fb.identities if i.curve == F.P384}
    n384 = 0
    for ser, t in zip(_creators(fb.block), cc):
        if ser in p384_ser:
            n384 += 1
            assert t.status != F.FAB_CREATOR_IDENTITY
    assert n384 >= 6
    assert any(fb.tx_status[i] == F.FAB_CREATOR_IDENTITY for i in range(fb.ntx))  # (the garbage PEM)


def test_other_curves_stay_unresolved(mixed_classes_block, monkeypatch):
    """A P-521 subject key, and the secp384r1 OID over a 64-byte point, are
    reported as unresolvable identities by the engine and the oracle alike."""
    fb = mixed_classes_block
    M.patch_oracle(monkeypatch)
    peer = next(i for i in fb.identities if i.curve == F.P384)
    name = F.x509_name("Org1MSP", "x")
    p521 = F.SEQ(F.der(0xA0, F.der_int(2)), F.der_int(5), F.SEQ(F.der_oid(F.OID_ECDSA_SHA384)), name,
                 F.SEQ(F.der(0x17, b"250101000000Z"), F.der(0x17, b"350101000000Z")), name,
                 F.SEQ(F.SEQ(F.der_oid(F.OID_EC_PUBKEY), F.der_oid("1.3.132.0.35")),
                       F.der(0x03, b"\x00\x04" + b"\x01" * 132)))
    short = F.x509_tbs(6, name, name, peer.pub[:64], F.P384, F.OID_ECDSA_SHA384)
    sets = []
    for tbs in (p521, short):
        ser = F.serialized_identity("Org1MSP", F.pem(F.x509_cert(tbs, b"\x30\x06\x02\x01\x01\x02\x01\x01",
                                                                   F.OID_ECDSA_SHA384)))
        assert R.deserialize(ser) is None
        sets.append([(ser, b"data", b"\x30\x06\x02\x01\x01\x02\x01\x01"),
                     (peer.serialized, b"data", b"\x30\x06\x02\x01\x01\x02\x01\x01")])
    assert R.deserialize(peer.serialized) is not None
    got = fabric.signature_sets_verify(sets, decode_only=True)
    assert got == [R.signature_set_to_valid_identities(s, None, decode_only=True) for s in sets]
    assert all(g[0][0] == F.E_BAD_IDENTITY and g[0][1] == F.E_NOT_VERIFIED for g in got), got


def test_patched_oracle_matches_construction(mixed_classes_block, monkeypatch):
    fb = mixed_classes_block
    M.patch_oracle(monkeypatch)
    out = R.validate_block(fb.block, M.make_verify(fb.p384_keys))
    assert [_got(o) for o in out] == [_want(fb, i) for i in range(fb.ntx)]
    # both curves met the high-S classes: P-384's half order decides its own
    assert {"creator_high_s", "endorse_high_s", "endorse_dup_after_invalid"} <= set(fb.tx_class)


def test_generator_defaults_unchanged():
    """With p384_orgs = 0 the generator's blocks are byte for byte what they
    were before it knew the second curve (digests taken from that generator)."""
    fb = F.generate_fabric_block()
    assert hashlib.sha256(fb.block).hexdigest() == \
        "2f3925b6415a16b927c210ecf09242f30de9db939727a73eeb0222cdad0d6c97"
    assert not fb.p384_keys
    fb = F.generate_fabric_block(ntx=2 * len(F.CORRUPTIONS), corrupt_den=0, classes=F.CORRUPTIONS,
                                 seed=7)
    assert hashlib.sha256(fb.block).hexdigest() == \
        "bd9a23c8373c43a60754bfe3ffbef2f35b4f730e9cfc5064ab74c91bef9c8d7b"
