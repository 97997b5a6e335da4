"""Test-side reference for BH_F_HASH_SHA384 / BH_F_HASH_SHA512 and
bh_verify_x509_ex.

* check_signature_from_ex: Go 1.21 crypto/x509 Certificate.CheckSignatureFrom
  restated for an ECDSA issuer on P-256 or P-384 and the three SHA-2
  algorithms (checkSignature takes the hash from the certificate's algorithm,
  the curve from the parent's key); oracle/x509_ref.py's walk and strict
  signature parser, oracle/ecdsa_ref.py's verifyNISTEC, hashlib's hashes.
* signed_batch: the by-construction batch of tests/p384_util.py for either
  curve and any of the device's hashes.
* pack_x509 / load_x509_vectors: the fixture tests/golden/x509_p384_vectors.json.
"""
from __future__ import annotations

import hashlib
import json
import os
import random

import numpy as np

from oracle import ecdsa_ref as O
from oracle import x509_ref as X
from tests.p384_util import P384, LibCrypto, pack_bytes  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X509_P384 = os.path.join(ROOT, "tests", "golden", "x509_p384_vectors.json")
HOSTSIM512 = os.path.join(ROOT, "tests", "native", "build", "libhostsim512.so")
SELFTEST = os.path.join(ROOT, "tests", "native", "build", "sha512_selftest")

BH_F_HASH_SHA256, BH_F_NO_LOW_S, BH_F_HASH_SHA384, BH_F_HASH_SHA512 = 1, 2, 32, 64
BH_CURVE_P256, BH_CURVE_P384 = 0, 2
CURVES = {"P-256": (O.P256, BH_CURVE_P256), "P-384": (P384, BH_CURVE_P384)}
HASHES = {"SHA256": (hashlib.sha256, BH_F_HASH_SHA256), "SHA384": (hashlib.sha384, BH_F_HASH_SHA384),
          "SHA512": (hashlib.sha512, BH_F_HASH_SHA512)}
# ecdsa-with-SHA256 / -SHA384 / -SHA512 (1.2.840.10045.4.3.2 / .3 / .4)
OID_HASH = {bytes.fromhex("2a8648ce3d040302"): "SHA256", bytes.fromhex("2a8648ce3d040303"): "SHA384",
            bytes.fromhex("2a8648ce3d040304"): "SHA512"}
# the padding and block edges of a 128-byte block, the empty message, one byte
EDGE_LENS = (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 241, 300)


def cert_hash(der: bytes):
    """Name of the hash of a certificate's (matching) signature algorithm, or None."""
    parts = X.split_cert(der)
    if parts is None:
        return None
    _, inner, outer, _ = parts
    if inner != outer or outer[1] != len(outer) - 2:
        return None
    return OID_HASH.get(outer[2:])


def check_signature_from_ex(der: bytes, curve: O.Curve, qx: int, qy: int) -> int:
    """BH_R_* of Certificate.CheckSignatureFrom(issuer with key (qx, qy) on curve)."""
    name = cert_hash(der)
    if name is None:
        return X.R_UNSUPPORTED
    tbs, _, _, sig = X.split_cert(der)
    rs = X.parse_signature(sig)
    if rs is None:
        return O.R_DER
    r, s = rs
    if r == 0:
        return O.R_R_NONPOS
    if s == 0:
        return O.R_S_NONPOS
    return O.go_ecdsa_verify(curve, qx, qy, HASHES[name][0](tbs).digest(), r, s)


def load_x509_vectors():
    with open(X509_P384) as f:
        return json.load(f)


def pack_x509(vecs):
    """(certs, cert_off, cert_len, issuer_pub, issuer_pub_off, issuer_curve) of fixture vectors."""
    certs, off, ln = pack_bytes([bytes.fromhex(v["cert"]) for v in vecs])
    pub, pub_off, _ = pack_bytes([bytes.fromhex(v["qx"] + v["qy"]) for v in vecs])
    curve = np.array([CURVES[v["curve"]][1] for v in vecs], np.uint8)
    return certs, off, ln, pub, pub_off, curve


def signed_batch(curve_name: str, hash_name: str, lc: LibCrypto | None = None, n=257, nkeys=12,
                 seed=512, lens=EDGE_LENS):
    """n signed records over nkeys keys of one curve, message i of length
    lens[i % len(lens)] hashed with hash_name; one record in eight corrupted by
    construction (message bit -- or, for an empty message, a swapped key -- r,
    high-S, wrong key, off-curve key, in turn). P-384 records are signed by
    libcrypto (lc), P-256 ones by the oracle's signer. Returns (recs, want,
    want_no_low_s): hex fields qx, qy, sig, msg, digest; the reasons with and
    without the low-S rule."""
    c = CURVES[curve_name][0]
    cb = (c.p.bit_length() + 7) // 8
    half = c.n >> 1
    hf = HASHES[hash_name][0]
    rng = random.Random(seed)
    keys = []
    for _ in range(nkeys):
        d = rng.randrange(1, c.n)
        qx, qy = O.pubkey(c, d)
        keys.append((d, qx, qy, lc.key(d, qx, qy) if curve_name == "P-384" else None))
    recs, want, want_nls = [], [], []
    kinds = ("msg_bit", "r_plus1", "high_s", "wrong_key", "offcurve_key")
    for i in range(n):
        d, qx, qy, k = keys[i % nkeys]
        msg = bytes(rng.getrandbits(8) for _ in range(lens[i % len(lens)]))
        dg = hf(msg).digest()
        if curve_name == "P-384":
            r, s = lc.sign(k, dg)
        else:
            r, s = O.sign_digest(c, d, dg, rng.randrange(1, c.n))
        if s > half:
            s = c.n - s
        reason = nls = O.R_OK
        if i % 8 == 3:
            kind = kinds[(i // 8) % len(kinds)]
            if kind == "msg_bit" and not msg:
                kind = "wrong_key"
            if kind == "msg_bit":
                b = bytearray(msg)
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
                msg, reason, nls = bytes(b), O.R_MATH, O.R_MATH
                dg = hf(msg).digest()
            elif kind == "r_plus1":
                r, reason, nls = (r + 1) % c.n or 1, O.R_MATH, O.R_MATH
            elif kind == "high_s":
                s, reason = c.n - s, O.R_HIGH_S  # still a valid signature without the rule
            elif kind == "wrong_key":
                _, qx, qy, _ = keys[(i + 1) % nkeys]
                reason = nls = O.R_MATH
            else:
                qy, reason, nls = (qy + 1) % c.p, O.R_BAD_KEY, O.R_BAD_KEY
        recs.append({"qx": qx.to_bytes(cb, "big").hex(), "qy": qy.to_bytes(cb, "big").hex(),
                     "sig": O.marshal_ecdsa_signature(r, s).hex(), "msg": msg.hex(),
                     "digest": dg.hex()})
        want.append(reason)
        want_nls.append(nls)
    for *_, k in keys:
        if k is not None:
            lc.free_key(k)
    return recs, np.array(want, np.uint8), np.array(want_nls, np.uint8)


def pack_records(recs):
    """SoA numpy packing of signed_batch records, messages in the msg field."""
    pub = np.frombuffer(b"".join(bytes.fromhex(r["qx"] + r["qy"]) for r in recs) + b"\0", np.uint8)
    return (pub,) + pack_bytes([bytes.fromhex(r["sig"]) for r in recs]) + \
        pack_bytes([bytes.fromhex(r["msg"]) for r in recs])
