"""Test-side helpers for batches and Fabric inputs that mix P-256 and P-384.

* cert_key / patch_oracle: oracle/fabric_ref.py resolves P-256 subject keys
  only; cert_key restates its walk for id-ecPublicKey with prime256v1 or
  secp384r1, and patch_oracle puts it in cert_p256_key's place.
* make_verify: the oracle's identity.Verify under the curve of the key, chosen
  from the set of generated P-384 keys.
* pool / build_mixed: fused golden records of both curves as one bh_mbatch,
  in one-span or two-span form, with the expectations of the fixtures.
"""
from __future__ import annotations

import json
import os

import numpy as np

from bdls_amd import _lib
from oracle import ecdsa_ref as O
from oracle import fabric_ref as R
from tests import p384_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN256 = os.path.join(ROOT, "tests", "golden", "p256_vectors.jsonl")
OID_P384 = bytes.fromhex("2b81040022")
# message lengths around the block and rate boundaries of SHA-256 (64) and SHA3-256 (136)
SEAM_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 135, 136, 137, 200, 272, 273)


def cert_key(der: bytes):
    """(X, Y, tbs_raw, sig_der) of an X.509 certificate whose subject key is
    id-ecPublicKey on prime256v1 (66-byte bit string) or secp384r1 (98), else
    None: oracle/fabric_ref.py cert_p256_key with the second curve."""
    try:
        tag, cert, _, end = R._tlv(der, 0)
        if tag != 0x30 or end != len(der):
            return None
        tag, tbs, tbs_raw, i = R._tlv(cert, 0)
        if tag != 0x30:
            return None
        tag, alg, _, i = R._tlv(cert, i)
        if tag != 0x30:
            return None
        tag, sv, _, i = R._tlv(cert, i)
        if tag != 0x03 or not sv or sv[0] != 0:
            return None
        tag, _, _, _ = R._tlv(alg, 0)
        if tag != 0x06:
            return None
        t = 0
        tag, _, _, t = R._tlv(tbs, t)
        if tag == 0xA0:
            tag, _, _, t = R._tlv(tbs, t)
        if tag != 0x02:
            return None
        for _ in range(4):
            tag, _, _, t = R._tlv(tbs, t)
            if tag != 0x30:
                return None
        tag, spki, _, t = R._tlv(tbs, t)
        if tag != 0x30:
            return None
        tag, algid, _, s = R._tlv(spki, 0)
        if tag != 0x30:
            return None
        tag, bits, _, s = R._tlv(spki, s)
        if tag != 0x03 or s != len(spki):
            return None
        tag, o1, _, a = R._tlv(algid, 0)
        if tag != 0x06:
            return None
        tag2, o2, _, a = R._tlv(algid, a)
    except R.DecodeError:
        return None
    if not (o1 == R.OID_EC_PUB and tag2 == 0x06 and a == len(algid) and len(bits) >= 2
            and bits[0] == 0 and bits[1] == 4):
        return None
    if o2 == R.OID_P256 and len(bits) == 66:
        w = 32
    elif o2 == OID_P384 and len(bits) == 98:
        w = 48
    else:
        return None
    return (int.from_bytes(bits[2:2 + w], "big"), int.from_bytes(bits[2 + w:], "big"), tbs_raw,
            sv[1:])


def patch_oracle(monkeypatch):
    monkeypatch.setattr(R, "cert_p256_key", cert_key)


def make_verify(p384_keys, family="SHA2"):
    """verify(x, y, msg, sig) -> BH_R_* of identity.Verify: P-384 for the keys
    of p384_keys, P-256 otherwise; the MSP's 256-bit hash either way."""
    memo = {}

    def verify(x, y, msg, sig):
        k = (x, y, msg, sig)
        if k not in memo:
            curve = U.P384 if (x, y) in p384_keys else O.P256
            memo[k] = O.identity_verify(curve, x, y, msg, sig, family)[1]
        return memo[k]
    return verify


def p384_keys_of(identities):
    """{(x, y)} of the workload Identity objects on P-384."""
    return {(int.from_bytes(i.pub[:48], "big"), int.from_bytes(i.pub[48:], "big"))
            for i in identities if len(i.pub) == 96}


# ---------------------------------------------------------------- mixed batches
def expect(r, no_low_s):
    return r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]


def pool(family):
    """(p256 records, p384 records) with fused messages for `family`, each with
    "reason" / "reason_no_low_s" as the fixtures state them. The P-256 fixture
    is SHA-256 only: under SHA3 its first records (all rejected there, with the
    oracle's reasons) are joined by records signed over SHA3-256 digests by the
    workload generator, one per length of SEAM_LENGTHS, every fourth with a
    message bit flipped or a high S; their expectations are the oracle's."""
    with open(GOLDEN256) as f:
        g256 = [json.loads(l) for l in f]
    p384 = [r for r in U.load_golden384() if r.get("family") == family]
    p256 = [dict(r) for r in g256 if "msg" in r and len(r["msg"]) <= 2 * 600]
    if family == "SHA2":
        for r in p256:  # the fixture's low-S-rule reason; without the rule, the oracle's
            if r["reason"] == O.R_HIGH_S:
                r["reason_no_low_s"] = _no_low_s(O.P256, r, family)
    else:
        p256 = p256[:20] + _signed_sha3_p256()
        for r in p256:
            q = (int(r["qx"], 16), int(r["qy"], 16))
            r["reason"] = O.identity_verify(O.P256, *q, bytes.fromhex(r["msg"]),
                                            bytes.fromhex(r["sig"]), family)[1]
            r["reason_no_low_s"] = _no_low_s(O.P256, r, family)
    for r in p256:
        r["curve"] = _lib.BH_CURVE_P256
    for r in p384:
        r["curve"] = _lib.BH_CURVE_P384
    return p256, p384


def _signed_sha3_p256():
    import hashlib
    import random
    from bdls_amd.workload import fabric as F
    L = F._gen()
    rng = random.Random(2563)
    recs = []
    for j, n in enumerate(SEAM_LENGTHS):
        priv, pub = F.keypair(L, 2563, j % 5)
        msg = bytes(rng.getrandbits(8) for _ in range(n))
        sg = F.sign_batch(L, [priv], [hashlib.sha3_256(msg).digest()], 2563 + j,
                          high_s=(j % 4 == 1))[0]
        if j % 4 == 3 and n:
            msg = msg[:-1] + bytes([msg[-1] ^ 0x10])
        recs.append({"qx": pub[:32].hex(), "qy": pub[32:].hex(), "sig": sg.hex(), "msg": msg.hex(),
                     "tag": f"sha3_len{n}"})
    return recs


def _no_low_s(curve, r, family):
    rc, rr, ss = O.unmarshal_ecdsa_signature(bytes.fromhex(r["sig"]))
    if rc != O.R_OK:
        return rc
    return O.go_ecdsa_verify(curve, int(r["qx"], 16), int(r["qy"], 16),
                             O.family_digest(family, bytes.fromhex(r["msg"])), rr, ss)


def pattern(name, n):
    """curve byte per record: 0 (P-256) / 2 (P-384)."""
    if name == "alternating":
        c = [2 * (i & 1) for i in range(n)]
    elif name == "p256":
        c = [0] * n
    elif name == "p384":
        c = [2] * n
    else:  # runs of 70, P-384 first
        c = [2 * ((i // 70 + 1) & 1) for i in range(n)]
    return np.array(c, np.uint8)


def pick(curves, p256, p384):
    """Records for a curve pattern, each pool cycled in order."""
    k = [0, 0]
    out = []
    for c in curves:
        g = 1 if c else 0
        src = p384 if g else p256
        out.append(src[k[g] % len(src)])
        k[g] += 1
    return out


def seam_of(i, length):
    """Seam of record i: cycles through 0..length."""
    return (7 * i + i // 3) % (length + 1)


def build_mixed(recs, two_span, fused=True):
    """bh_mbatch arrays for records carrying "curve": (curve, pub, pub_off, sig,
    sig_off, sig_len, msg, msg_off, msg_len, msg2_off, msg2_len). In two-span
    form record i's message is cut at seam_of(i, len) and its second span is
    stored BEFORE its first, away from it, so nothing works by adjacency."""
    curve = np.array([r["curve"] for r in recs], np.uint8)
    keys = [bytes.fromhex(r["qx"] + r["qy"]) for r in recs]
    pub, pub_off, _ = U.pack_bytes(keys)
    sig, so, sl = U.pack_bytes([bytes.fromhex(r["sig"]) for r in recs])
    msgs = [bytes.fromhex(r["msg"] if fused else r["digest"]) for r in recs]
    if not two_span:
        msg, mo, ml = U.pack_bytes(msgs)
        return (curve, pub, pub_off, sig, so, sl, msg, mo, ml, None, None)
    buf = bytearray()
    mo, ml, mo2, ml2 = [], [], [], []
    for i, m in enumerate(msgs):
        k = seam_of(i, len(m))
        buf += b"\xa5" * 3
        mo2.append(len(buf))
        buf += m[k:]
        buf += b"\x5a" * 5
        mo.append(len(buf))
        buf += m[:k]
        ml.append(k)
        ml2.append(len(m) - k)
    msg = np.frombuffer(bytes(buf) + b"\0", np.uint8)
    return (curve, pub, pub_off, sig, so, sl, msg, np.array(mo, np.uint64),
            np.array(ml, np.uint32), np.array(mo2, np.uint64), np.array(ml2, np.uint32))
