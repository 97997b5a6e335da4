"""Test-side reference for BH_CURVE_P384.

* P384: the curve as an oracle/ecdsa_ref.py Curve (FIPS 186-4 D.1.2.4), so the
  curve-generic Python restatement of bccsp/sw Verify is the expected value.
* LibCrypto: the machine's OpenSSL libcrypto through ctypes, an independent
  second opinion (ECDSA_verify) and a fast signer (ECDSA_do_sign). The
  reference holds no P-384 vectors, so parity for this curve is "oracle +
  OpenSSL", as it is for secp256k1.
* pack384 / signed_batch: SoA packing and the by-construction batch shared by
  the CPU (host harness) and GPU tests.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import hashlib
import json
import os
import random

import numpy as np

from oracle import ecdsa_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN384 = os.path.join(ROOT, "tests", "golden", "p384_vectors.jsonl")
HOSTSIM384 = os.path.join(ROOT, "tests", "native", "build", "libhostsim384.so")

P384 = O.Curve(
    name="P-384",
    p=2**384 - 2**128 - 2**96 + 2**32 - 1,
    a=-3,
    b=0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF,
    n=0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973,
    gx=0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7,
    gy=0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F,
    nist=True,
)
N, P = P384.n, P384.p
HALF = N >> 1
BH_CURVE_P384 = 2
NID_SECP384R1 = 715


def h48(v: int) -> str:
    return v.to_bytes(48, "big").hex()


def load_golden384():
    with open(GOLDEN384) as f:
        return [json.loads(l) for l in f]


def pack384(recs, fused):
    """SoA numpy packing of fixture records (96-byte keys)."""
    pub = np.frombuffer(b"".join(bytes.fromhex(r["qx"] + r["qy"]) for r in recs) + b"\0", np.uint8)
    sigs = [bytes.fromhex(r["sig"]) for r in recs]
    msgs = [bytes.fromhex(r["msg"] if fused else r["digest"]) for r in recs]
    return (pub,) + pack_bytes(sigs) + pack_bytes(msgs)


def pack_bytes(items):
    ln = np.array([len(s) for s in items], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if items:
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(items) + b"\0", np.uint8)
    return buf, off, ln


class LibCrypto:
    """ctypes wrapper of libcrypto's P-384 ECDSA. Raises OSError if it cannot be loaded."""

    def __init__(self):
        name = ctypes.util.find_library("crypto")
        L = None
        for cand in ("libcrypto.so.3", name, "libcrypto.so"):
            if not cand:
                continue
            try:
                L = ctypes.CDLL(cand)
                break
            except OSError:
                continue
        if L is None:
            raise OSError("libcrypto not found")
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.EC_KEY_new_by_curve_name.restype = vp
        L.EC_KEY_new_by_curve_name.argtypes = [i32]
        L.EC_KEY_free.argtypes = [vp]
        L.BN_bin2bn.restype = vp
        L.BN_bin2bn.argtypes = [ctypes.c_char_p, i32, vp]
        L.BN_free.argtypes = [vp]
        L.BN_bn2binpad.argtypes = [vp, ctypes.c_char_p, i32]
        L.EC_KEY_set_private_key.argtypes = [vp, vp]
        L.EC_KEY_set_public_key_affine_coordinates.argtypes = [vp, vp, vp]
        L.ECDSA_do_sign.restype = vp
        L.ECDSA_do_sign.argtypes = [ctypes.c_char_p, i32, vp]
        L.ECDSA_SIG_get0.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.ECDSA_SIG_free.argtypes = [vp]
        L.ECDSA_verify.argtypes = [i32, ctypes.c_char_p, i32, ctypes.c_char_p, i32, vp]
        L.ECDSA_verify.restype = i32
        L.ERR_clear_error.restype = None
        self.L = L

    def _bn(self, v: int):
        b = v.to_bytes(48, "big")
        return self.L.BN_bin2bn(b, len(b), None)

    def key(self, d: int | None, qx: int, qy: int):
        """EC_KEY* with the public point (qx, qy) and, if given, the private
        scalar; None when libcrypto rejects the point."""
        L = self.L
        k = L.EC_KEY_new_by_curve_name(NID_SECP384R1)
        x, y = self._bn(qx), self._bn(qy)
        ok = L.EC_KEY_set_public_key_affine_coordinates(k, x, y)
        L.BN_free(x)
        L.BN_free(y)
        if ok != 1:
            L.ERR_clear_error()
            L.EC_KEY_free(k)
            return None
        if d is not None:
            bd = self._bn(d)
            L.EC_KEY_set_private_key(k, bd)
            L.BN_free(bd)
        return k

    def free_key(self, k):
        self.L.EC_KEY_free(k)

    def sign(self, k, digest: bytes):
        """(r, s) of a fresh signature over digest (not low-S normalised)."""
        L = self.L
        sig = L.ECDSA_do_sign(digest, len(digest), k)
        assert sig, "ECDSA_do_sign failed"
        r, s = ctypes.c_void_p(), ctypes.c_void_p()
        L.ECDSA_SIG_get0(sig, ctypes.byref(r), ctypes.byref(s))
        br, bs = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48)
        L.BN_bn2binpad(r, br, 48)
        L.BN_bn2binpad(s, bs, 48)
        L.ECDSA_SIG_free(sig)
        return int.from_bytes(br.raw, "big"), int.from_bytes(bs.raw, "big")

    def verify(self, k, digest: bytes, sig: bytes) -> bool:
        rc = self.L.ECDSA_verify(0, digest, len(digest), sig, len(sig), k)
        if rc != 1:
            self.L.ERR_clear_error()
        return rc == 1


def family_hash(family: str, msg: bytes) -> bytes:
    return hashlib.sha256(msg).digest() if family == "SHA2" else hashlib.sha3_256(msg).digest()


def signed_batch(lc: LibCrypto, n=600, nkeys=24, seed=384, family="SHA2", msg_len=200):
    """n libcrypto-signed records over nkeys keys; one in eight corrupted by
    construction (message bit, r, high-S, wrong key, off-curve key, in turn).
    Returns (recs, want): recs with hex fields qx, qy, sig, msg, digest; want
    the reason each must get with the low-S rule."""
    rng = random.Random(seed)
    keys = []
    for _ in range(nkeys):
        d = rng.randrange(1, N)
        qx, qy = O.pubkey(P384, d)
        keys.append((d, qx, qy, lc.key(d, qx, qy)))
    recs, want = [], []
    kinds = ("msg_bit", "r_plus1", "high_s", "wrong_key", "offcurve_key")
    for i in range(n):
        d, qx, qy, k = keys[i % nkeys]
        msg = bytes(rng.getrandbits(8) for _ in range(msg_len + i % 7))
        dg = family_hash(family, msg)
        r, s = lc.sign(k, dg)
        if s > HALF:
            s = N - s
        reason = O.R_OK
        if i % 8 == 3:
            kind = kinds[(i // 8) % len(kinds)]
            if kind == "msg_bit":
                b = bytearray(msg)
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
                msg, reason = bytes(b), O.R_MATH
                dg = family_hash(family, msg)
            elif kind == "r_plus1":
                r, reason = (r + 1) % N or 1, O.R_MATH
            elif kind == "high_s":
                s, reason = N - s, O.R_HIGH_S
            elif kind == "wrong_key":
                _, qx, qy, _ = keys[(i + 1) % nkeys]
                reason = O.R_MATH
            else:
                qy, reason = (qy + 1) % P, O.R_BAD_KEY
        recs.append({"qx": h48(qx), "qy": h48(qy), "sig": O.marshal_ecdsa_signature(r, s).hex(),
                     "msg": msg.hex(), "digest": dg.hex()})
        want.append(reason)
    for *_, k in keys:
        lc.free_key(k)
    return recs, np.array(want, np.uint8)
