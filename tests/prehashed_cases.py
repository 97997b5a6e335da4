"""Crafted BDLS records for the prehashed entry point
(bh_verify_bdls_prehashed_dev / hs_verify_bdls_prehashed): the caller supplies
SignedProto.Hash(), so e, u1 and u2 can be steered into the curve-level edge
cases that BLAKE2b-hashed messages never reach -- on the kernels production
BDLS batches run.

build(curve) -> [(tag, x32, y32, r_bytes, s_bytes, digest_bytes, expected_reason)]

Every expected reason is oracle.ecdsa_ref.go_ecdsa_verify's on (key, digest,
SetBytes(r), SetBytes(s)); the generators' own idea of a record's verdict is
only asserted against it (accept classes must be accepted), never used. r and
s are minimal big-endian bytes unless the record is about their encoding.
"""
from __future__ import annotations

import ctypes
import json
import os
import random
from collections import Counter

from oracle import ecdsa_ref as O
from tests import comb_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "native", "build", "libhostsim.so")
CURVES = {"secp256k1": O.SECP256K1, "P-256": O.P256}
CURVE_ID = {"P-256": 0, "secp256k1": 1}


def minimal(v: int) -> bytes:
    """big.Int.Bytes(): minimal big-endian, empty for 0."""
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def b32(v: int) -> bytes:
    return v.to_bytes(32, "big")


def library_shape():
    """(comb teeth, comb spacing, G fold, G comb window bits) the library was
    built with, read from the host harness (compiled from the same headers)."""
    L = ctypes.CDLL(HOSTSIM)
    for f in (L.hs_ll_shape, L.hs_gfold, L.hs_gcomb_bits):
        f.restype = ctypes.c_uint32
    sh = L.hs_ll_shape()
    return sh >> 8, sh & 0xFF, L.hs_gfold(), L.hs_gcomb_bits()


def k1_edge_classes(comb_shape=(7, 37)):
    """The secp256k1 digest-level edge cases of tests/test_bdls.py (x wrap,
    infinity, internal doubling, GLV split edges, signed-comb edges) -- the
    very records test_k1_curve_edges_hostsim runs, shared, with the DER
    signature it takes read back to integers:
    [(tag, qx, qy, r, s, digest, reason)]."""
    from tests.test_bdls import _k1_edge_records
    out = []
    for tag, qx, qy, sig, digest, reason in _k1_edge_records(comb_shape):
        r, s, rest = O.asn1_unmarshal_ecdsa_sig(sig)
        assert not rest and O.marshal_ecdsa_signature(r, s) == sig
        out.append((tag, qx, qy, r, s, digest, reason))
    return out


def window_edge_u2(n: int):
    """u2 at the edges of the 4-bit signed key-table windows (registry slots,
    per-batch windowed tables): tests/test_gpu_comb.py's list."""
    from tests.test_gpu_comb import _window_edge_u2
    return _window_edge_u2(n)


class _List:
    """The record list of one curve; the reason of every record is the oracle's."""

    def __init__(self, curve):
        self.c = curve
        self.recs = []

    def add(self, tag, qx, qy, rb, sb, digest):
        rb, sb, digest = bytes(rb), bytes(sb), bytes(digest)
        x32 = qx if isinstance(qx, bytes) else b32(qx)
        y32 = qy if isinstance(qy, bytes) else b32(qy)
        reason = O.go_ecdsa_verify(self.c, int.from_bytes(x32, "big"), int.from_bytes(y32, "big"),
                                   digest, int.from_bytes(rb, "big"), int.from_bytes(sb, "big"))
        self.recs.append((tag, x32, y32, rb, sb, digest, reason))
        return reason

    def add_der(self, tag, qx, qy, sig, digest):
        _, r, s = O.unmarshal_ecdsa_signature(sig)
        return self.add(tag, qx, qy, minimal(r), minimal(s), digest)

    def add_pairs(self, tag, recs):
        """comb_cases.records_for_u2's output: the valid record, then its twin."""
        for k, (qx, qy, sig, dg) in enumerate(recs):
            self.add_der(tag if k % 2 == 0 else tag + "_flip", qx, qy, sig, dg)


def _common_edges(L: _List, seed: int):
    """Digest and signature encodings, the same on both curves."""
    c, n = L.c, L.c.n
    rng = random.Random(seed)
    d = rng.randrange(1, n)
    qx, qy = O.pubkey(c, d)

    def signed(digest):
        r, s = O.sign_digest(c, d, digest, rng.randrange(1, n), low_s=False)
        return minimal(r), minimal(s)

    # ---- digest values: e = 0, and e >= n (one subtraction of n)
    for tag, dg in (("digest_e_zero", b"\0" * 32), ("digest_eq_n", b32(n)),
                    ("digest_n_plus_1", b32(n + 1)), ("digest_2p256m1", b"\xff" * 32)):
        rb, sb = signed(dg)
        L.add(tag, qx, qy, rb, sb, dg)
        L.add(tag + "_flip", qx, qy, rb, sb, dg[:31] + bytes([dg[31] ^ 1]))
    # digest = n is e = 0 and n + 1 is e = 1: the same signature under both spellings
    rb, sb = signed(b"\0" * 32)
    L.add("digest_eq_n_as_zero", qx, qy, rb, sb, b32(n))
    # ---- digest lengths on an otherwise valid signature: short digests are
    # not shifted, long ones are cut to 32 bytes, none is e = 0
    for ln in (0, 1, 31, 33, 64):
        dg = bytes(rng.getrandbits(8) | 1 for _ in range(ln))
        rb, sb = signed(dg)
        L.add(f"digest_len{ln}", qx, qy, rb, sb, dg)
        if ln > 32:   # bytes past the 32nd are not read; the 32nd is
            L.add(f"digest_len{ln}_tail", qx, qy, rb, sb, dg[:32] + bytes(ln - 32))
            L.add(f"digest_len{ln}_flip", qx, qy, rb, sb, dg[:31] + bytes([dg[31] ^ 1]) + dg[32:])
        elif ln:      # the same bytes left-aligned in 32 are another number
            L.add(f"digest_len{ln}_padded", qx, qy, rb, sb, dg + bytes(32 - ln))
            L.add(f"digest_len{ln}_flip", qx, qy, rb, sb, dg[:-1] + bytes([dg[-1] ^ 2]))
        else:         # empty = 32 zero bytes = e 0
            L.add("digest_len0_as_zero32", qx, qy, rb, sb, b"\0" * 32)
            L.add("digest_len0_flip", qx, qy, rb, sb, b"\0" * 31 + b"\1")
    # ---- r / s encodings and ranges
    dg = bytes(rng.getrandbits(8) for _ in range(32))
    rb, sb = signed(dg)
    for tag, r_, s_ in (("r_eq_n", minimal(n), sb), ("s_eq_n", rb, minimal(n)),
                        ("r_zero", b"\0", sb), ("r_zero_32B", b"\0" * 32, sb),
                        ("r_empty", b"", sb), ("s_empty", rb, b""), ("s_zero", rb, b"\0\0"),
                        ("r_33B", b"\x01" + rb.rjust(32, b"\0"), sb),
                        ("s_33B", rb, b"\x01" + sb.rjust(32, b"\0")),
                        ("r_n_plus_r", minimal(n + int.from_bytes(rb, "big")), sb),
                        ("r_nm1", minimal(n - 1), sb), ("s_nm1", rb, minimal(n - 1)),
                        ("r1_s1", b"\1", b"\1"),
                        ("r_leading_zeros", b"\0\0" + rb, sb),
                        ("s_leading_zeros", rb, b"\0" * 5 + sb),
                        ("rs_leading_zeros_40B", rb.rjust(40, b"\0"), sb.rjust(40, b"\0")),
                        ("high_s_accepted", rb, minimal(n - int.from_bytes(sb, "big")))):
        L.add(tag, qx, qy, r_, s_, dg)
    return d


def _key_edges(L: _List, seed: int):
    """A key off the curve and a key with X >= p (X - p is the x of a curve
    point, so only the range check can tell), each also with r = n: P-256
    checks the key first, secp256k1's verifyLegacy the ranges."""
    c, n, p = L.c, L.c.n, L.c.p
    rng = random.Random(seed)
    d = rng.randrange(1, n)
    qx, qy = O.pubkey(c, d)
    dg = bytes(rng.getrandbits(8) for _ in range(32))
    r, s = O.sign_digest(c, d, dg, rng.randrange(1, n), low_s=False)
    x = 0
    while True:
        rhs = (x * x * x + c.a * x + c.b) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs and x + p < 2**256:
            break
        x += 1
    for tag, kx, ky in (("q_offcurve", qx, qy ^ 1), ("q_x_ge_p", x + p, y)):
        L.add(tag, kx, ky, minimal(r), minimal(s), dg)
        L.add(tag + "_r_eq_n", kx, ky, minimal(n), minimal(s), dg)


def _build_k1(shape):
    t, sp, _kgf, gw = shape
    c = O.SECP256K1
    n = c.n
    L = _List(c)
    for tag, qx, qy, r, s, dg, reason in k1_edge_classes((t, sp)):
        assert L.add(tag, qx, qy, minimal(r), minimal(s), dg) == reason
    # registry slots / per-batch windows (4-bit signed digits) and the G comb
    L.add_pairs("window_u2", CC.records_for_u2(c, window_edge_u2(n), seed=101))
    u1s = CC.g_comb_u1(n, gw)
    rng = random.Random(102)
    L.add_pairs("g_comb_u1", CC.records_for_u2(c, [rng.randrange(1, n) for _ in u1s], seed=103,
                                               u1s=u1s))
    # Q = G, -G, 2 G: u2 Q meets the G tables' own points
    for tag, d in (("q_eq_G", 1), ("q_eq_negG", n - 1), ("q_eq_2G", 2)):
        qx, qy = O.pubkey(c, d)
        for k in range(2):
            dg = bytes(rng.getrandbits(8) for _ in range(32))
            r, s = O.sign_digest(c, d, dg, rng.randrange(1, n), low_s=False)
            L.add(tag, qx, qy, minimal(r), minimal(s), dg)
            L.add(tag + "_flip", qx, qy, minimal(r), minimal(s), dg[:31] + bytes([dg[31] ^ 1]))
        # u1 G == u2 Q and u1 G == -u2 Q on these keys: e = r d and e = -r d
        r = rng.randrange(1, n)
        s = rng.randrange(1, n)
        L.add(tag + "_sum_inf", qx, qy, minimal(r), minimal(s), b32((-r * d) % n))
        k = rng.randrange(1, n)
        r = O.scalar_mult(c, k, (c.gx, c.gy))[0] % n
        L.add(tag + "_u1G_eq_u2Q", qx, qy, minimal(r), minimal(2 * r * d * pow(k, -1, n) % n),
              b32(r * d % n))
    _common_edges(L, 104)
    _key_edges(L, 105)
    return L.recs


def _build_p256(shape):
    t, sp, kgf, gw = shape
    c = O.P256
    n = c.n
    L = _List(c)
    # every golden record whose signature is a DER (r, s) that SetBytes can
    # carry (r, s >= 0): re-encoded as bytes, re-judged without the low-S rule
    with open(os.path.join(ROOT, "tests", "golden", "p256_vectors.jsonl")) as f:
        for g in map(json.loads, f):
            try:
                r, s, _ = O.asn1_unmarshal_ecdsa_sig(bytes.fromhex(g["sig"]))
            except O.Asn1Error:
                continue
            if r < 0 or s < 0:
                continue
            L.add("golden_" + g["tag"], bytes.fromhex(g["qx"]), bytes.fromhex(g["qy"]), minimal(r),
                  minimal(s), bytes.fromhex(g["digest"]))
    u2s = CC.signed_comb_u2(n, t, sp) + CC.unsigned_comb_u2(t, sp) + window_edge_u2(n)
    L.add_pairs("comb_u2", CC.records_for_u2(c, u2s, seed=111))
    u1s = CC.g_comb_u1(n, gw)
    rng = random.Random(112)
    L.add_pairs("g_comb_u1", CC.records_for_u2(c, [rng.randrange(1, n) for _ in u1s], seed=113,
                                               u1s=u1s))
    fold = CC.fold_crafted(c, t, sp, seed=33, kgf=kgf)
    assert len(fold) == 8, [f[3] for f in fold]
    for qx, qy, sig, dg, _exp in CC.records_for_fold(c, fold, low_s=False):
        L.add_der("fold_crafted", qx, qy, sig, dg)
    lad = CC.ladder_crafted(c, seed=43, kgf=kgf, t=t, s=sp)
    assert len(lad) == 9 and len({x[2] for x in lad}) == 9
    for qx, qy, sig, dg, _exp in CC.records_for_fold(c, lad, low_s=False):
        L.add_der("ladder_crafted", qx, qy, sig, dg)
    for qx, qy, sig, dg, _exp, tag in CC.distinct_key_classes(c, seed=61, reps=2):
        L.add_der("distinct_" + tag, qx, qy, sig, dg)
    _common_edges(L, 114)
    _key_edges(L, 115)
    return L.recs


# tag -> reason every record of the class must have (accept classes accepted,
# the classes built to fail in the group equation failing there), and the
# fewest records of it
_REQUIRED = {
    "secp256k1": {
        "k1_xwrap_accept": (0, 2), "k1_xwrap_wrong_r": (9, 2), "k1_sum_inf": (9, 2),
        "k1_u1G_eq_u2Q": (0, 3), "k1_u1G_eq_u2Q_high_s": (0, 3), "k1_glv_u2": (0, 30),
        "k1_glv_u2_flip": (9, 30), "k1_valid": (0, 6), "k1_flip": (9, 6),
        "window_u2": (0, 18), "window_u2_flip": (9, 18), "g_comb_u1": (0, 10),
        "g_comb_u1_flip": (9, 10), "q_eq_G": (0, 2), "q_eq_negG": (0, 2), "q_eq_2G": (0, 2),
        "q_eq_G_sum_inf": (9, 1), "q_eq_G_u1G_eq_u2Q": (0, 1), "q_eq_negG_u1G_eq_u2Q": (0, 1),
        "q_eq_2G_u1G_eq_u2Q": (0, 1),
        "q_offcurve": (9, 1), "q_x_ge_p": (9, 1), "q_offcurve_r_eq_n": (8, 1),
        "q_x_ge_p_r_eq_n": (8, 1),
    },
    "P-256": {
        "golden_xwrap_accept": (0, 2), "golden_xwrap_wrong_r": (9, 2),
        "golden_sum_infinity": (9, 2), "golden_u1G_eq_u2Q_accept": (0, 3),
        "golden_high_s": (0, 40), "golden_q_offcurve": (7, 1), "golden_empty_digest": (9, 1),
        "comb_u2": (0, 40), "comb_u2_flip": (9, 40), "g_comb_u1": (0, 10),
        "g_comb_u1_flip": (9, 10), "fold_crafted": (None, 13), "ladder_crafted": (None, 14),
        "distinct_xwrap_accept": (0, 4), "distinct_sum_infinity": (9, 2),
        "distinct_u1G_eq_u2Q_accept": (0, 2),
        "q_offcurve": (7, 1), "q_x_ge_p": (7, 1), "q_offcurve_r_eq_n": (7, 1),
        "q_x_ge_p_r_eq_n": (7, 1),
    },
}
_COMMON_REQUIRED = {
    "digest_e_zero": 0, "digest_eq_n": 0, "digest_n_plus_1": 0, "digest_2p256m1": 0,
    "digest_e_zero_flip": 9, "digest_eq_n_flip": 9, "digest_eq_n_as_zero": 0,
    "digest_len0": 0, "digest_len1": 0, "digest_len31": 0, "digest_len33": 0, "digest_len64": 0,
    "digest_len0_as_zero32": 0, "digest_len0_flip": 9, "digest_len1_padded": 9,
    "digest_len31_padded": 9, "digest_len31_flip": 9, "digest_len33_tail": 0,
    "digest_len64_tail": 0, "digest_len33_flip": 9, "digest_len64_flip": 9,
    "r_eq_n": 8, "s_eq_n": 10, "r_zero": 4, "r_zero_32B": 4, "r_empty": 4, "s_empty": 5,
    "s_zero": 5, "r_33B": 8, "s_33B": 10, "r_n_plus_r": 8, "r_nm1": 9, "s_nm1": 9, "r1_s1": 9,
    "r_leading_zeros": 0, "s_leading_zeros": 0, "rs_leading_zeros_40B": 0, "high_s_accepted": 0,
}


def build(curve: str, shape=None):
    """The crafted list of one curve ("secp256k1" or "P-256") for the comb shape
    / G tables the library was built with (library_shape() by default)."""
    shape = shape or library_shape()
    recs = _build_k1(shape) if curve == "secp256k1" else _build_p256(shape)
    count = Counter(r[0] for r in recs)
    need = dict(_REQUIRED[curve])
    need.update({k: (v, 1) for k, v in _COMMON_REQUIRED.items()})
    for tag, (reason, least) in need.items():
        assert count[tag] >= least, (curve, tag, count[tag], least)
        if reason is not None:
            got = {r[6] for r in recs if r[0] == tag}
            assert got == {reason}, (curve, tag, got, reason)
    # the crafted-event classes hold both verdicts (a finite R accepted with
    # its twin rejected, an R at infinity rejected)
    for tag in ("fold_crafted", "ladder_crafted"):
        if curve == "P-256":
            assert {r[6] for r in recs if r[0] == tag} == {0, 9}, tag
    return recs


def class_counts(recs):
    return Counter(r[0] for r in recs)


def reaches_group_equation(curve: str, rec) -> bool:
    """The record passes every check before the group equation (its key is a
    curve point, 0 < r, s < n): it takes a ladder or a key table."""
    c = CURVES[curve]
    _tag, x32, y32, rb, sb, _dg, reason = rec
    x, y = int.from_bytes(x32, "big"), int.from_bytes(y32, "big")
    return reason in (O.R_OK, O.R_MATH) and x < c.p and y < c.p and O.on_curve(c, x, y)


def pack(recs):
    """bh_bdls_batch-ordered arrays (tests/bdls_util.py pack_bdls) with the
    digest in the message field; version is a constant nobody reads."""
    from tests.bdls_util import pack_bdls
    return pack_bdls([dict(x=x.hex(), y=y.hex(), r=rb.hex(), s=sb.hex(), msg=dg.hex(), version=1)
                      for _tag, x, y, rb, sb, dg, _reason in recs])
