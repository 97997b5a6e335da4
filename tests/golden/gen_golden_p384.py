#!/usr/bin/env python3
"""Generate tests/golden/p384_vectors.jsonl: the fixture of the P-384 verify
path (BH_CURVE_P384). Run from the repo root:  python tests/golden/gen_golden_p384.py

Every expected reason comes from oracle/ecdsa_ref.py run on the P-384 curve of
tests/p384_util.py (the reference holds no P-384 vectors; tests/test_p384_cpu.py
cross-checks the oracle against OpenSSL libcrypto). Fields per record: tag, qx,
qy (48-byte hex), sig, digest, msg + family (fused records), reason (Fabric's
low-S rule applied) and reason_no_low_s where BH_F_NO_LOW_S changes it.
The DER reject / accept vectors are the signature bytes of
tests/golden/p256_vectors.jsonl replayed against a P-384 key.
"""
from __future__ import annotations

import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ecdsa_ref as O  # noqa: E402
from tests.p384_util import HALF, N, P, P384 as C, family_hash, h48  # noqa: E402

G = (C.gx, C.gy)


def verify_no_low_s(qx, qy, sig, digest):
    """bccsp/sw Verify without the IsLowS step (BH_F_NO_LOW_S)."""
    if len(sig) == 0:
        return O.R_EMPTY_SIG
    if len(digest) == 0:
        return O.R_EMPTY_DIGEST
    reason, r, s = O.unmarshal_ecdsa_signature(sig)
    if reason != O.R_OK:
        return reason
    return O.go_ecdsa_verify(C, qx, qy, digest, r, s)


def rec(tag, qx, qy, sig: bytes, digest: bytes | None = None, msg: bytes | None = None,
        family: str = "SHA2"):
    if msg is not None:
        digest = family_hash(family, msg)
    reason = O.csp_verify(C, qx, qy, sig, digest)[1]
    out = {"tag": tag, "qx": h48(qx), "qy": h48(qy), "sig": sig.hex(), "digest": digest.hex(),
           "reason": reason}
    nl = verify_no_low_s(qx, qy, sig, digest)
    if nl != reason:
        out["reason_no_low_s"] = nl
    if msg is not None:
        out["msg"] = msg.hex()
        out["family"] = family
    return out


def b48(v: int) -> bytes:
    return v.to_bytes(48, "big")


def find_wrap_point(rng):
    """A curve point with x in [n, p): p - n ~ 2^190, so pick x there until
    x^3 - 3x + b is a square (p = 3 mod 4)."""
    while True:
        x = N + rng.randrange(P - N)
        rhs = (x * x * x - 3 * x + C.b) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return x, y


def main():
    rng = random.Random(20260384)
    out = []
    sig_of = O.marshal_ecdsa_signature

    keys = []
    for _ in range(6):
        d = rng.randrange(1, N)
        keys.append((d,) + O.pubkey(C, d))

    def signed(d, digest, low=True):
        return O.sign_digest(C, d, digest, rng.randrange(1, N), low_s=low)

    def crafted(d, s_of, tag, qx, qy, low=True):
        """A valid signature with a chosen relation: k random, r = x(kG) mod n,
        s = s_of(r, k), e = s k - r d; retried until s is low when asked."""
        while True:
            k = rng.randrange(1, N)
            r = O.scalar_mult(C, k, G)[0] % N
            s = s_of(r, k) % N
            if s == 0 or (low and s > HALF):
                continue
            e = (s * k - r * d) % N
            return rec(tag, qx, qy, sig_of(r, s), digest=b48(e))

    # --- valid at digest lengths around the 48-byte truncation ---------------
    for i, L in enumerate((1, 20, 32, 47, 48, 49, 64)):
        d, qx, qy = keys[i % len(keys)]
        dg = bytes(rng.getrandbits(8) for _ in range(L))
        out.append(rec(f"digest_len{L}", qx, qy, sig_of(*signed(d, dg)), digest=dg))
    # --- fused messages over the SHA-256 / SHA3-256 padding edges ------------
    for fam in ("SHA2", "SHA3"):
        for i, L in enumerate((0, 55, 56, 63, 64, 119, 120, 135, 136, 137, 300)):
            d, qx, qy = keys[i % len(keys)]
            msg = bytes(rng.getrandbits(8) for _ in range(L))
            r, s = signed(d, family_hash(fam, msg))
            out.append(rec(f"valid_msg_{fam}_len{L}", qx, qy, sig_of(r, s), msg=msg, family=fam))

    d, qx, qy = keys[0]
    dg = family_hash("SHA2", b"fabric p384")
    r, s = signed(d, dg)

    # --- the low-S boundary and high-S ---------------------------------------
    out.append(crafted(d, lambda r_, k: HALF, "s_eq_half_valid", qx, qy))
    out.append(crafted(d, lambda r_, k: HALF + 1, "s_eq_half_plus1", qx, qy, low=False))
    for i in range(3):
        dd, x, y = keys[i]
        m = bytes(rng.getrandbits(8) for _ in range(64))
        rr, ss = signed(dd, family_hash("SHA2", m))
        out.append(rec("high_s", x, y, sig_of(rr, N - ss), msg=m))
    # --- range and sign edges -------------------------------------------------
    for tag, rr, ss in [("r_eq_n", N, s), ("r_n_plus1", N - 1 + 2, s), ("r_nm1", N - 1, s),
                        ("s_eq_n", r, N), ("s_n_plus1", r, N + 1), ("s_2p384m1", r, 2**384 - 1),
                        ("r_2p384m1", 2**384 - 1, s), ("r_49byte", 2**384 + 5, s),
                        ("s_49byte", r, 2**384 + 5), ("r_huge", 2**600 + 1, s),
                        ("s_huge", r, 2**600 + 1), ("r_and_s_huge", 2**500, 2**500),
                        ("r_zero", 0, s), ("s_zero", r, 0), ("r_neg1", -1, s), ("s_neg1", r, -1),
                        ("r_neg_big", -r, s), ("s_neg_big", r, -s), ("r1_s1", 1, 1)]:
        out.append(rec(tag, qx, qy, sig_of(rr, ss), digest=dg))
    # --- DER vectors of the P-256 fixture, replayed against a P-384 key -------
    with open(os.path.join(HERE, "p256_vectors.jsonl")) as f:
        for line in f:
            o = json.loads(line)
            if o["tag"].startswith(("der_", "ref_impl_test_der_", "empty_")):
                digest = b"" if o["tag"] in ("empty_digest", "empty_both") else dg
                out.append(rec("p256_" + o["tag"], qx, qy, bytes.fromhex(o["sig"]), digest=digest))
    # accept-with-trailing forms around a genuine P-384 signature
    whole = O.marshal_ecdsa_signature(r, s)
    body = whole[2:]
    assert whole[1] < 0x80 and len(body) == whole[1]  # two INTEGERs of <= 49 bytes: short form
    out.append(rec("der_trailing_garbage_ok", qx, qy, whole + b"\xde\xad\xbe\xef", digest=dg))
    out.append(rec("der_extra_elem_ok", qx, qy,
                   b"\x30" + O.der_len(len(body) + 3) + body + b"\x02\x01\x07", digest=dg))
    out.append(rec("der_seq_longform_short", qx, qy, b"\x30\x81" + bytes([len(body)]) + body,
                   digest=dg))
    # --- bad public keys --------------------------------------------------------
    sig = sig_of(r, s)
    out.append(rec("q_offcurve", qx, (qy + 1) % P, sig, digest=dg))
    out.append(rec("q_x_eq_p", P, qy, sig, digest=dg))
    out.append(rec("q_y_ge_p", qx, P + 1, sig, digest=dg))
    out.append(rec("q_y_eq_p", qx, P, sig, digest=dg))
    out.append(rec("q_zero", 0, 0, sig, digest=dg))
    out.append(rec("q_all_ones", 2**384 - 1, 2**384 - 1, sig, digest=dg))
    out.append(rec("q_neg_y", qx, P - qy, sig, digest=dg))  # -Q: on curve, math reject
    out.append(rec("q_offcurve_r_range", qx, (qy + 1) % P, sig_of(N + 5, s), digest=dg))
    # --- e = 0 mod n (u1 = 0) ----------------------------------------------------
    for tag, dgx in (("e_zero_digest", b"\x00" * 48), ("e_zero_1B", b"\x00"), ("digest_eq_n", b48(N)),
                     ("digest_n_plus1", b48(N + 1)), ("digest_all_ones", b"\xff" * 48),
                     ("digest_64_ge_n", b"\xff" * 48 + b"\x01" * 16)):
        out.append(rec(tag, qx, qy, sig_of(*signed(d, dgx)), digest=dgx))
    # --- small u2: s = r / u2 -----------------------------------------------------
    for u2 in (1, 2, N - 1):
        inv = pow(u2, -1, N)
        out.append(crafted(d, lambda r_, k, inv=inv: r_ * inv, f"u2_eq_{'nm1' if u2 > 2 else u2}",
                           qx, qy))
    # --- Q in {G, -G, 2G} -----------------------------------------------------------
    for tag, dd in (("q_eq_G", 1), ("q_eq_negG", N - 1), ("q_eq_2G", 2)):
        x, y = O.pubkey(C, dd)
        m = bytes(rng.getrandbits(8) for _ in range(100))
        out.append(rec(tag, x, y, sig_of(*signed(dd, family_hash("SHA2", m))), msg=m))
        out.append(crafted(dd, lambda r_, k: r_, tag + "_u2_1", x, y))
    # --- u1 G == u2 Q as points. An engine that computes the two products apart
    # doubles in its final addition; one that folds u1 G window by window into the
    # u2 Q accumulator (verify384.h) never holds both, so these are ordinary
    # records for it and its doubling cases are the acc_eq_gentry / u2_eq_nm6
    # records at the end of this file ------------------------------------------------
    for j in range(3):
        dd, x, y = keys[j]
        while True:
            k = rng.randrange(1, N)
            rr = O.scalar_mult(C, k, G)[0] % N
            ss = 2 * rr * dd * pow(k, -1, N) % N
            if ss <= HALF:
                break
        e = rr * dd % N
        out.append(rec("u1G_eq_u2Q_accept", x, y, sig_of(rr, ss), digest=b48(e)))
        out.append(rec("u1G_eq_u2Q_wrong_r", x, y, sig_of((rr + 1) % N or 1, ss), digest=b48(e)))
    # --- u1 G == -u2 Q (infinity) ----------------------------------------------------
    for j in range(3):
        dd, x, y = keys[j]
        rr = rng.randrange(1, N)
        ss = rng.randrange(1, HALF)
        out.append(rec("sum_infinity", x, y, sig_of(rr, ss), digest=b48((-rr * dd) % N)))
    # --- x-wrap: R.x = n + t accepted through x mod n == r = t --------------------------
    for j in range(2):
        xw, yw = find_wrap_point(rng)
        t = xw - N
        # Q = R itself: e = 0, r = s = t gives u1 = 0, u2 = 1
        out.append(rec("xwrap_q_is_R", xw, yw, sig_of(t, t), digest=b"\x00" * 48))
        out.append(rec("xwrap_q_is_R_wrong_r", xw, yw, sig_of(t + 1, t), digest=b"\x00" * 48))
        out.append(rec("xwrap_r_eq_x", xw, yw, sig_of(xw, t), digest=b"\x00" * 48))
        # a general one: Q = r^-1 (s R - e G)
        ss = rng.randrange(1, HALF)
        e = rng.randrange(1, N)
        ri = pow(t, -1, N)
        Q = O.point_add(C, O.scalar_mult(C, ri * ss % N, (xw, yw)),
                        O.scalar_mult(C, (-ri * e) % N, G))
        out.append(rec("xwrap_accept", Q[0], Q[1], sig_of(t, ss), digest=b48(e)))
        out.append(rec("xwrap_wrong_r", Q[0], Q[1], sig_of(t + 1, ss), digest=b48(e)))
    # --- one flipped bit in r, s, digest, key ---------------------------------------------
    for j in range(4):
        dd, x, y = keys[j + 1]
        dgx = bytes(rng.getrandbits(8) for _ in range(48))
        rr, ss = signed(dd, dgx)
        out.append(rec("flip_base_valid", x, y, sig_of(rr, ss), digest=dgx))
        out.append(rec("flip_r", x, y, sig_of(rr ^ (1 << rng.randrange(380)), ss), digest=dgx))
        out.append(rec("flip_s", x, y, sig_of(rr, ss ^ (1 << rng.randrange(380))), digest=dgx))
        bd = bytearray(dgx)
        bd[rng.randrange(48)] ^= 1 << rng.randrange(8)
        out.append(rec("flip_digest", x, y, sig_of(rr, ss), digest=bytes(bd)))
        out.append(rec("flip_key_x", x ^ (1 << rng.randrange(380)), y, sig_of(rr, ss), digest=dgx))
        out.append(rec("flip_key_y", x, y ^ (1 << rng.randrange(380)), sig_of(rr, ss), digest=dgx))

    # --- (appended after the classes above so that their records do not move) ---------
    # u2 = n - 6: with 4-bit signed windows the last step adds -3Q to -3Q (16c = n - 3,
    # n = 3 mod 16): a Jacobian addition of equal points
    inv = pow(N - 6, -1, N)
    out.append(crafted(d, lambda r_, k, inv=inv: r_ * inv, "u2_eq_nm6", qx, qy))
    # u1 = dg 16^w (one non-zero nibble) and u2 Q = u1 G with Q = jG, u2 = u1 / j: after
    # the u2 Q ladder the accumulator EQUALS the fixed-base entry dg 16^w G that the u1 G
    # pass adds next (the mixed addition must double). r = x(2 u1 G) mod n, s = r / u2,
    # e = u1 s. s is fixed by the choice, so every j is kept with the reason the low-S
    # rule gives it; the assertions below want an accept at window 0 and at window 95.
    for w, dg_ in ((0, 1), (0, 12), (3, 5), (95, 15), (95, 12)):
        u1 = dg_ << (4 * w)
        for j in (1, 2, 3, 4, 6):
            if u1 % j:
                continue
            u2 = u1 // j
            x, y = O.pubkey(C, j)
            rr = O.scalar_mult(C, 2 * u1 % N, G)[0] % N
            ss = rr * pow(u2, -1, N) % N
            e = u1 * ss % N
            tag = f"acc_eq_gentry_w{w}_d{dg_}_q{j}G"
            out.append(rec(tag, x, y, sig_of(rr, ss), digest=b48(e)))
            out.append(rec(tag + "_wrong_r", x, y, sig_of(rr % (N - 1) + 1, ss), digest=b48(e)))

    path = os.path.join(HERE, "p384_vectors.jsonl")
    with open(path, "w") as f:
        for o in out:
            f.write(json.dumps(o, sort_keys=True) + "\n")
    from collections import Counter
    tags = {o["tag"]: o for o in out}
    for t in ("s_eq_half_valid", "u1G_eq_u2Q_accept", "xwrap_accept", "xwrap_q_is_R", "u2_eq_1",
              "u2_eq_nm1", "der_trailing_garbage_ok", "der_extra_elem_ok", "digest_eq_n"):
        assert tags[t]["reason"] == O.R_OK, t
    assert tags["sum_infinity"]["reason"] == O.R_MATH
    assert tags["u2_eq_nm6"]["reason"] == O.R_OK
    for w in (0, 95):
        acc = [o for o in out if o["tag"].startswith(f"acc_eq_gentry_w{w}_") and
               not o["tag"].endswith("_wrong_r")]
        assert any(o["reason"] == O.R_OK for o in acc), w
        assert all(o.get("reason_no_low_s", o["reason"]) == O.R_OK for o in acc), w
    assert tags["s_eq_n"]["reason_no_low_s"] == O.R_S_RANGE
    print(len(out), "records,", os.path.getsize(path), "bytes;",
          dict(Counter(O.REASON_NAMES[o["reason"]] for o in out)))


if __name__ == "__main__":
    main()
