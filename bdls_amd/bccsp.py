"""Host-side mirror of the reference's BCCSP provider interface for the verify
hot path, backed by the HIP engine (libbdlship.so).

Mirrors (names, argument meaning, error behaviour):
  bccsp/bccsp.go:90-134        BCCSP.Verify / Hash / KeyImport
  bccsp/sw/impl.go:247-270     CSP.Verify argument checks and error wrapping
  bccsp/sw/ecdsa.go:41-57      verifyECDSA
  bccsp/utils/ecdsa.go:41-89   UnmarshalECDSASignature / IsLowS
  msp/identities.go:170-199    identity.Verify (SHA-256 then Verify)
and adds the batch entry points a `bccsp/hip` provider exposes:
  BatchVerify(keys, signatures, digests)          -> valid[], errors[]
  BatchIdentityVerify(keys, messages, signatures) -> fused SHA-256 + verify

A Go `(false, err)` is raised here as BCCSPError; `(false, nil)` returns False,
exactly as the reference distinguishes them. Batch calls return per-record
reason codes instead of raising.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import (BH_F_BATCH_KEYS, BH_F_HASH_SHA256, BH_F_HASH_SHA3_256, BH_F_HASH_SHA384,
                   BH_F_HASH_SHA512, BH_F_NO_LOW_S, BhBatch)

# reason codes (include/bdls_hip.h)
R_OK, R_EMPTY_SIG, R_EMPTY_DIGEST, R_DER, R_R_NONPOS, R_S_NONPOS, R_HIGH_S = range(7)
R_BAD_KEY, R_R_RANGE, R_MATH, R_S_RANGE = 7, 8, 9, 10
ERROR_REASONS = frozenset({R_EMPTY_SIG, R_EMPTY_DIGEST, R_DER, R_R_NONPOS, R_S_NONPOS, R_HIGH_S})

P256_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
P256_HALF_N = P256_N >> 1
P384_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
P384_HALF_N = P384_N >> 1
# curve name -> (BH_CURVE_*, coordinate bytes, half order): bccsp/utils/ecdsa.go:26-31
_CURVES = {"P-256": (_lib.BH_CURVE_P256, 32, P256_HALF_N),
           "P-384": (_lib.BH_CURVE_P384, 48, P384_HALF_N)}

# Go error strings (bccsp/sw/impl.go, bccsp/sw/ecdsa.go, bccsp/utils/ecdsa.go)
_ERR_TEXT = {
    R_EMPTY_SIG: "Invalid signature. Cannot be empty.",
    R_EMPTY_DIGEST: "Invalid digest. Cannot be empty.",
    R_DER: "Failed verifing with opts [%s]: Failed unmashalling signature [failed unmashalling signature]",
    R_R_NONPOS: "Failed verifing with opts [%s]: Failed unmashalling signature [invalid signature, R must be larger than zero]",
    R_S_NONPOS: "Failed verifing with opts [%s]: Failed unmashalling signature [invalid signature, S must be larger than zero]",
    R_HIGH_S: "Failed verifing with opts [%s]: Invalid S. Must be smaller than half the order [%s][%HALF%].",
}


def _err_text(reason: int, curve: str = "P-256") -> str:
    """The Go error text; the high-S one carries the curve's half order."""
    return _ERR_TEXT[reason].replace("%HALF%", str(_CURVES[curve][2]))


class BCCSPError(Exception):
    """A Go `(false, err)` result of BCCSP.Verify."""

    def __init__(self, reason: int, msg: str):
        super().__init__(msg)
        self.reason = reason


@dataclass(frozen=True)
class ECDSAPublicKey:
    """bccsp/sw/ecdsakey.go:72 ecdsaPublicKey: curve "P-256" or "P-384", the two
    curves of the sw provider (bccsp/sw/conf.go:43-61)."""
    x: int
    y: int
    curve: str = "P-256"

    def raw(self) -> bytes:
        """X || Y big-endian, 64 bytes (P-256) or 96 (P-384): a bh_batch.pub entry."""
        cb = _CURVES[self.curve][1]
        if self.x < 0 or self.y < 0 or self.x.bit_length() > 8 * cb or self.y.bit_length() > 8 * cb:
            # pointFromAffine rejects these; encode an off-curve marker the engine rejects
            return b"\x00" * (2 * cb)
        return self.x.to_bytes(cb, "big") + self.y.to_bytes(cb, "big")

    def raw64(self) -> bytes:
        assert self.curve == "P-256"
        return self.raw()

    def symmetric(self) -> bool:
        return False

    def private(self) -> bool:
        return False


class ECDSAGoPublicKeyImportOpts:
    """bccsp/opts.go ECDSAGoPublicKeyImportOpts (raw = (x, y))."""


class SHA256Opts:
    """bccsp/hashopts.go SHA256Opts."""


class SHA3_256Opts:
    """bccsp/hashopts.go SHA3_256Opts."""


class SHA384Opts:
    """bccsp/hashopts.go SHA384Opts (the sw provider's hash at security level 384)."""


# msp/identities.go:219-227 getHashOpt: MSP SignatureHashFamily -> device hash flag
_FAMILY_FLAG = {"SHA2": BH_F_HASH_SHA256, "SHA3": BH_F_HASH_SHA3_256}
# batch_identity_verify(hash=...): a hash named outright instead of the MSP's family
_HASH_FLAG = {"SHA256": BH_F_HASH_SHA256, "SHA3_256": BH_F_HASH_SHA3_256,
              "SHA384": BH_F_HASH_SHA384, "SHA512": BH_F_HASH_SHA512}


def family_flag(family: str) -> int:
    if family not in _FAMILY_FLAG:
        raise BCCSPError(-1, f"hash family not recognized [{family}]")
    return _FAMILY_FLAG[family]


def hash_flag(name: str) -> int:
    if name not in _HASH_FLAG:
        raise BCCSPError(-1, f"hash function not recognized [{name}]")
    return _HASH_FLAG[name]


def _arr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def batch_curve(keys: Sequence[ECDSAPublicKey]) -> int:
    """The BH_CURVE_* of a batch's keys: all on one curve (P-256 when empty)."""
    names = {k.curve for k in keys}
    if len(names) > 1:
        raise BCCSPError(-1, f"keys of one batch must be on one curve, got {sorted(names)}")
    for name in names:
        if name not in _CURVES:
            raise BCCSPError(-1, f"Unsupported 'VerifyKey' curve [{name}]")
        return _CURVES[name][0]
    return _lib.BH_CURVE_P256


def pack_records(keys: Sequence[ECDSAPublicKey], sigs: Sequence[bytes], msgs: Sequence[bytes]):
    """SoA packing of a batch (host numpy buffers); its keys are on one curve."""
    n = len(keys)
    batch_curve(keys)
    pub = np.frombuffer(b"".join(k.raw() for k in keys) or b"\0", dtype=np.uint8)
    sig_len = np.fromiter((len(s) for s in sigs), dtype=np.uint32, count=n)
    msg_len = np.fromiter((len(m) for m in msgs), dtype=np.uint32, count=n)
    sig_off = np.zeros(n, dtype=np.uint64)
    msg_off = np.zeros(n, dtype=np.uint64)
    if n:
        sig_off[1:] = np.cumsum(sig_len[:-1], dtype=np.uint64)
        msg_off[1:] = np.cumsum(msg_len[:-1], dtype=np.uint64)
    sig = np.frombuffer(b"".join(sigs) + b"\0", dtype=np.uint8)
    msg = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8)
    return pub, sig, sig_off, sig_len, msg, msg_off, msg_len


def verify_packed(pub, sig, sig_off, sig_len, msg, msg_off, msg_len, flags: int = 0,
                  curve: int = _lib.BH_CURVE_P256):
    """Host-buffer batch through bh_verify. Returns (valid bool[n], reason u8[n])."""
    _lib.ensure_init()
    n = len(sig_len)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    reason = np.zeros(n or 1, dtype=np.uint8)
    b = BhBatch(_arr(pub), _arr(sig), _arr(sig_off), _arr(sig_len), _arr(msg), _arr(msg_off),
                _arr(msg_len))
    _lib.check(_lib.lib().bh_verify(curve, ctypes.byref(b), n, flags,
                                    bitmap.ctypes.data, reason.ctypes.data))
    valid = np.unpackbits(bitmap, bitorder="little")[:n].astype(bool)
    return valid, reason[:n]


def verify_packed384(keys: Sequence[bytes], sigs: Sequence[bytes], msgs: Sequence[bytes],
                     flags: int = 0, submit: bool = False):
    """P-384 records as per-record buffers (96-byte keys X || Y, DER signatures,
    messages or digests) through bh_batch_verify384_ptrs: the library
    de-duplicates the keys by content, packs into its own page-locked staging and
    deals the batch over every device. Returns (valid bool[n], reason u8[n]);
    submit=True: a function that waits for the job (bh_verify_wait) and returns
    them, so several batches can be in flight."""
    _lib.ensure_init()
    n = len(sigs)

    def col(items):
        bufs = [np.frombuffer(bytes(b) + b"\0", np.uint8) for b in items]
        return bufs, np.array([a.ctypes.data for a in bufs] or [0], np.uint64)
    kb, kp = col(keys)
    sb, sp = col(sigs)
    mb, mp = col(msgs)
    sig_len = np.array([len(s) for s in sigs] or [0], np.uint32)
    msg_len = np.array([len(m) for m in msgs] or [0], np.uint32)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    reason = np.zeros(n or 1, dtype=np.uint8)
    b = _lib.BhPBatch(kp.ctypes.data, sp.ctypes.data, sig_len.ctypes.data, mp.ctypes.data,
                      msg_len.ctypes.data)

    def result():
        return np.unpackbits(bitmap, bitorder="little")[:n].astype(bool), reason[:n]
    if not submit:
        _lib.check(_lib.lib().bh_batch_verify384_ptrs(ctypes.byref(b), n, flags,
                                                      bitmap.ctypes.data, reason.ctypes.data))
        return result()
    job = ctypes.c_void_p()
    _lib.check(_lib.lib().bh_batch_verify384_ptrs_submit(ctypes.byref(b), n, flags,
                                                         bitmap.ctypes.data, reason.ctypes.data,
                                                         ctypes.byref(job)))

    def wait():   # (everything was copied when the submit call returned)
        _lib.check(_lib.lib().bh_verify_wait(job))
        return result()
    return wait


def verify_mixed(curve, pub, pub_off, sig, sig_off, sig_len, msg, msg_off, msg_len,
                 msg2_off=None, msg2_len=None, flags: int = 0):
    """Host-buffer batch of P-256 and P-384 records through bh_verify_mixed:
    curve u8[n] (BH_CURVE_P256 / BH_CURVE_P384), record i's key at
    pub[pub_off[i]:], optional second message spans (both or neither).
    Returns (valid bool[n], reason u8[n])."""
    _lib.ensure_init()
    n = len(sig_len)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    reason = np.zeros(n or 1, dtype=np.uint8)
    b = _lib.BhMBatch(_arr(curve), _arr(pub), _arr(pub_off), _arr(sig), _arr(sig_off),
                      _arr(sig_len), _arr(msg), _arr(msg_off), _arr(msg_len),
                      None if msg2_off is None else msg2_off.ctypes.data,
                      None if msg2_len is None else msg2_len.ctypes.data)
    _lib.check(_lib.lib().bh_verify_mixed(ctypes.byref(b), n, flags, bitmap.ctypes.data,
                                          reason.ctypes.data))
    valid = np.unpackbits(bitmap, bitorder="little")[:n].astype(bool)
    return valid, reason[:n]


class HipCSP:
    """The `bccsp/hip` provider's verify/hash surface (embeds sw semantics)."""

    def __init__(self, device_mask: int = 0, low_s: bool = True, batch_keys: bool = False):
        """batch_keys: P-384 batch calls set BH_F_BATCH_KEYS, so a key that a pass
        sees at least 4 times gets a comb table for that pass (results are the
        same either way; P-256 batches find their repeated keys unasked)."""
        self._flags = 0 if low_s else BH_F_NO_LOW_S
        self._batch_keys = bool(batch_keys)
        _lib.ensure_init(device_mask)

    def _batch_flags(self, curve: int) -> int:
        keys = getattr(self, "_batch_keys", False) and curve == _lib.BH_CURVE_P384
        return self._flags | (BH_F_BATCH_KEYS if keys else 0)

    # -- BCCSP.Hash (bccsp/sw/hash.go:29-33). Single-message hashing stays on the
    # host like sw; batched hashing is fused into BatchIdentityVerify on device.
    def hash(self, msg: bytes, opts=None) -> bytes:
        if isinstance(opts, SHA3_256Opts):
            return hashlib.sha3_256(msg).digest()
        if isinstance(opts, SHA384Opts):
            return hashlib.sha384(msg).digest()
        return hashlib.sha256(msg).digest()

    # -- BCCSP.Hash as a batch (bccsp/bccsp.go:109, bccsp/sw/impl.go:177-194): the
    # messages hashed on the device in one bh_hash call. SHA2-256 (the default
    # opts) and SHA3-256; the wider digests are not offered by bh_hash.
    def batch_hash(self, msgs: Sequence[bytes], opts=None) -> list[bytes]:
        if isinstance(opts, SHA384Opts):
            raise BCCSPError(-1, f"Unsupported 'HashOpt' provided [{opts}]")
        alg = _lib.BH_HASH_SHA3_256 if isinstance(opts, SHA3_256Opts) else _lib.BH_HASH_SHA256
        n = len(msgs)
        if n == 0:
            return []
        ln = np.array([len(m) for m in msgs], np.uint32)
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        data = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\0", np.uint8)
        out = np.zeros(n * 32, np.uint8)
        b = _lib.BhHBatch(data.ctypes.data, len(data) - 1, off.ctypes.data, ln.ctypes.data, 1,
                          None, None, None)
        _lib.check(_lib.lib().bh_hash(alg, ctypes.byref(b), n, out.ctypes.data, None))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)]

    def key_import(self, raw, opts) -> ECDSAPublicKey:
        if isinstance(opts, ECDSAGoPublicKeyImportOpts):
            x, y = raw
            return ECDSAPublicKey(int(x), int(y))
        raise BCCSPError(-1, f"Unsupported 'KeyImportOpts' provided [{opts}]")

    # -- BCCSP.Verify (bccsp/sw/impl.go:247-270 -> sw/ecdsa.go:41-57)
    def verify(self, k, signature: bytes, digest: bytes, opts=None) -> bool:
        if k is None:
            raise BCCSPError(-1, "Invalid Key. It must not be nil.")
        if not isinstance(k, ECDSAPublicKey) or k.curve not in _CURVES:
            raise BCCSPError(-1, f"Unsupported 'VerifyKey' provided [{k}]")
        sig, dg = bytes(signature or b""), bytes(digest or b"")
        # a no-low-S provider, or a P-384 key (no coalescer for it): a one-record batch
        if self._flags or k.curve != "P-256":
            valid, reason = verify_packed(*pack_records([k], [sig], [dg]), flags=self._flags,
                                          curve=batch_curve([k]))
            return self._result(int(reason[0]), bool(valid[0]), opts, k.curve)
        # bh_csp_verify_p256: concurrent callers share device passes (coalescer);
        # ctypes releases the GIL for the call
        v, r = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().bh_csp_verify_p256(k.raw64(), sig, len(sig), dg, len(dg),
                                                 ctypes.byref(v), ctypes.byref(r)))
        return self._result(r.value, bool(v.value), opts)

    def _result(self, reason: int, valid: bool, opts, curve: str = "P-256") -> bool:
        if reason in ERROR_REASONS:
            txt = _err_text(reason, curve)
            if "%s" in txt:
                txt = txt.replace("%s", str(opts), 1).replace("%s", "", 1)
            raise BCCSPError(reason, txt)
        return valid

    # -- batch extensions
    def batch_verify(self, keys: Sequence[ECDSAPublicKey], signatures: Sequence[bytes],
                     digests: Sequence[bytes], staged: bool = False):
        """Returns (valid bool[n], reason u8[n]); reason in ERROR_REASONS <=> Go error.
        staged=True (P-384 keys only): the batch goes as per-record buffers through
        bh_batch_verify384_ptrs -- every device, keys imported once each."""
        curve = batch_curve(keys)
        if staged and curve == _lib.BH_CURVE_P384:
            return verify_packed384([k.raw() for k in keys], signatures, digests,
                                    self._batch_flags(curve))
        return verify_packed(*pack_records(keys, signatures, digests),
                             flags=self._batch_flags(curve), curve=curve)

    def batch_identity_verify(self, keys: Sequence[ECDSAPublicKey], messages: Sequence[bytes],
                              signatures: Sequence[bytes], family: str = "SHA2",
                              hash: str | None = None, staged: bool = False):
        """msp/identities.go:170-199 for a whole batch with the MSP's hash family
        (SHA2 -> SHA-256, SHA3 -> SHA3-256) fused on device. hash ("SHA256",
        "SHA3_256", "SHA384", "SHA512") names the hash outright and overrides
        family: "SHA384" is the sw provider's level-384 pairing with P-384 keys
        (bccsp/sw/conf.go:43-46); SHA-384 and SHA-512 run as a digest pass ahead
        of the curve's pass."""
        flag = hash_flag(hash) if hash is not None else family_flag(family)
        curve = batch_curve(keys)
        # staged (P-384 keys, a 256-bit hash): bh_batch_verify384_ptrs, as in batch_verify
        if staged and curve == _lib.BH_CURVE_P384 and not flag & (
                _lib.BH_F_HASH_SHA384 | _lib.BH_F_HASH_SHA512):
            return verify_packed384([k.raw() for k in keys], signatures, messages,
                                    self._batch_flags(curve) | flag)
        return verify_packed(*pack_records(keys, signatures, messages),
                             flags=self._batch_flags(curve) | flag, curve=curve)

    def register_keys_p384(self, keys: Sequence[ECDSAPublicKey], device: int = -1) -> np.ndarray:
        """bh_keys384_register: build and keep the fixed-base tables of P-384 keys
        that will verify again and again (the MSP identity cache, msp/cache/cache.go;
        the BDLS participant set). Returns one status byte per key: 0 registered
        or already present, 7 not a point of P-384, 255 registry full. Results of
        verification never depend on it."""
        for k in keys:
            if not isinstance(k, ECDSAPublicKey) or k.curve != "P-384":
                raise BCCSPError(-1, f"Unsupported key for the P-384 registry [{k}]")
        status = np.zeros(len(keys), np.uint8)
        if len(keys):
            raw = b"".join(k.raw() for k in keys)
            _lib.check(_lib.lib().bh_keys384_register(device, raw, len(keys), status.ctypes.data))
        return status

    def identity_verify(self, k, msg: bytes, sig: bytes, family: str = "SHA2",
                        hash: str | None = None) -> None:
        """identity.Verify: raises on error or invalid signature (returns None if valid)."""
        valid, reason = self.batch_identity_verify([k], [msg], [sig], family, hash)
        r = int(reason[0])
        if r in ERROR_REASONS:
            raise BCCSPError(r, "could not determine the validity of the signature: " +
                             _err_text(r, k.curve).replace("%s", "<nil>", 1).replace("%s", "", 1))
        if not valid[0]:
            raise BCCSPError(r, "The signature is invalid")


def x509_check_signatures(certs: Sequence[bytes], issuer_keys: Sequence[ECDSAPublicKey]):
    """bh_verify_x509_ex: certificate i's signature against issuer key i, Go's
    Certificate.CheckSignatureFrom for ECDSA issuers on P-256 or P-384 with
    ecdsa-with-SHA256 / -SHA384 / -SHA512 (a chain link of msp/mspimpl.go:717-722).
    Returns (valid bool[n], reason u8[n]); reason 11 (BH_R_UNSUPPORTED) leaves
    the certificate to Go's x509."""
    _lib.ensure_init()
    n = len(certs)
    if len(issuer_keys) != n:
        raise BCCSPError(-1, "one issuer key per certificate")
    for k in issuer_keys:
        if k.curve not in _CURVES:
            raise BCCSPError(-1, f"Unsupported 'VerifyKey' curve [{k.curve}]")
    raws = [k.raw() for k in issuer_keys]
    pub = np.frombuffer(b"".join(raws) + b"\0", dtype=np.uint8)
    curve = np.array([_CURVES[k.curve][0] for k in issuer_keys], dtype=np.uint8)
    pub_len = np.fromiter((len(r) for r in raws), dtype=np.uint64, count=n)
    cert_len = np.fromiter((len(c) for c in certs), dtype=np.uint32, count=n)
    pub_off = np.zeros(n, dtype=np.uint64)
    cert_off = np.zeros(n, dtype=np.uint64)
    if n:
        pub_off[1:] = np.cumsum(pub_len[:-1], dtype=np.uint64)
        cert_off[1:] = np.cumsum(cert_len[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(certs) + b"\0", dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    reason = np.zeros(n or 1, dtype=np.uint8)
    _lib.check(_lib.lib().bh_verify_x509_ex(buf.ctypes.data, _arr(cert_off), _arr(cert_len),
                                            pub.ctypes.data, _arr(pub_off), _arr(curve), n,
                                            bitmap.ctypes.data, reason.ctypes.data))
    return np.unpackbits(bitmap, bitorder="little")[:n].astype(bool), reason[:n]


def parse_der_sig(der: bytes):
    """bh_parse_der_sig (host, Go-asn1 exact). Returns (reason, r|None, s|None)."""
    L = _lib.lib()
    r = ctypes.create_string_buffer(32)
    s = ctypes.create_string_buffer(32)
    rb, sb = ctypes.c_int(), ctypes.c_int()
    buf = ctypes.create_string_buffer(bytes(der), max(1, len(der)))
    rc = L.bh_parse_der_sig(ctypes.cast(buf, ctypes.c_void_p), len(der), ctypes.cast(r, ctypes.c_void_p),
                            ctypes.cast(s, ctypes.c_void_p), ctypes.byref(rb), ctypes.byref(sb))
    if rc < 0:
        raise _lib.EngineError(_lib.last_error())
    if rc != R_OK:
        return rc, None, None
    rv = None if rb.value else int.from_bytes(r.raw, "big")
    sv = None if sb.value else int.from_bytes(s.raw, "big")
    return rc, rv, sv
