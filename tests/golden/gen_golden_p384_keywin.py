#!/usr/bin/env python3
"""Generate tests/golden/p384_keywin_vectors.jsonl: crafted records for the
table route of the P-384 pass (stage384_keywin, bdls_amd/csrc/keys384.h). Run
from the repo root:  python tests/golden/gen_golden_p384_keywin.py

The route adds u2 Q window by window (upwards, from an empty accumulator) and
then u1 G window by window. Each record fixes u1, u2 and Q = j G, so the walk
meets a chosen situation: R = u1 G + u2 Q, r = x(R) mod n, s = r / u2,
e = u1 s, the digest is e's 48 bytes. s is whatever it comes out as, so the
fixture carries reason (Fabric's low-S rule) and reason_no_low_s; the tests
run it both ways. Expectations come from oracle/ecdsa_ref.py on the P-384
curve; every record that arithmetic decides is re-checked against OpenSSL
libcrypto here and in tests/test_p384_keys_cpu.py.

Situations (w: the window of G's walk at which it happens):
  acc_eq_gentry_w*      accumulator == the G entry being added (doubling branch)
  acc_eq_neg_gentry_w*  accumulator == -entry: infinity mid-walk, the walk goes on
  final_infinity*       u1 G = -u2 Q: infinity at the end, BH_R_MATH
  u2_one_digit_*        u2 = d 16^w
  u2_eq_nm1, u2_nibbles_ge8   the scalars whose signed recoding carries to the top
  u1_zero               e = 0: nothing from the table of G
  xwrap*                x(R) in [n, p): the r + n candidate decides
  *_wrong_r             the same walk against r + 1: BH_R_MATH
The accumulator cannot equal a Q entry or its negative, so no
record aims at that.
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
from tests import p384_util as U  # noqa: E402
from tests.golden.gen_golden_p384 import b48, find_wrap_point, rec  # noqa: E402
from tests.p384_util import N, P, P384 as C  # noqa: E402

G = (C.gx, C.gy)
OUT = os.path.join(HERE, "p384_keywin_vectors.jsonl")


def nib(v: int, w: int) -> int:
    return (v >> (4 * w)) & 15


def records():
    rng = random.Random(384_2026)
    out = []
    sig_of = O.marshal_ecdsa_signature

    def emit(tag, Q, u1, u2, r=None, twin=True):
        """The record whose verification computes exactly u1 and u2; r defaults
        to x(u1 G + u2 Q) mod n (any r when that sum is infinite)."""
        assert 0 <= u1 < N and 0 < u2 < N
        if r is None:
            R = O.point_add(C, O.scalar_mult(C, u1, G), O.scalar_mult(C, u2, Q))
            r = (R[0] % N) if R is not None else rng.randrange(1, N)
            assert r != 0
        s = r * pow(u2, -1, N) % N
        e = u1 * s % N
        out.append(rec(tag, Q[0], Q[1], sig_of(r, s), digest=b48(e)))
        if twin:
            r2 = r + 1 if r + 1 < N else 1
            s2 = r2 * pow(u2, -1, N) % N
            out.append(rec(tag + "_wrong_r", Q[0], Q[1], sig_of(r2, s2), digest=b48(u1 * s2 % N)))

    def key():
        j = rng.randrange(2, N)
        return j, O.pubkey(C, j)

    def u1_with_digit(w):
        while True:
            u1 = rng.randrange(16 ** 95, N)
            if nib(u1, w) and nib(u1, 0):
                return u1

    # accumulator == +/- the G entry at the first, a middle and the last window
    for w in (0, 47, 95):
        for sign, name in ((1, "acc_eq_gentry"), (-1, "acc_eq_neg_gentry")):
            j, Q = key()
            u1 = u1_with_digit(w)
            low = u1 % (16 ** w)
            u2 = (sign * nib(u1, w) * 16 ** w - low) * pow(j, -1, N) % N
            tag = f"{name}_w{w}_d{nib(u1, w)}"
            if sign < 0 and w == 95:
                tag = "final_infinity_w95"  # the top window is the last addition
            emit(tag, Q, u1, u2)
    # the same through Q = G and Q = 2G, whose tables the build test looks at
    emit("acc_eq_gentry_w0_qG", G, 7, 7)
    emit("acc_eq_gentry_w0_q2G", O.pubkey(C, 2), 10, 5)
    # infinity mid-walk, then a run of zero digits before the walk resumes
    j, Q = key()
    u1 = (rng.randrange(16 ** 95, N) >> 80 << 80) | 0x3
    emit("acc_eq_neg_gentry_w0_then_zeros", Q, u1, (-3) * pow(j, -1, N) % N)
    # a final infinity with nothing special before it
    j, Q = key()
    u2 = rng.randrange(1, N)
    emit("final_infinity", Q, (-u2 * j) % N, u2, twin=False)
    # u2 with a single non-zero digit
    for w, d in ((0, 1), (0, 15), (50, 9), (95, 15), (95, 1)):
        j, Q = key()
        emit(f"u2_one_digit_w{w}_d{d}", Q, rng.randrange(1, N), d * 16 ** w, twin=(w == 50))
    # u2 whose signed recoding carries into the top window
    j, Q = key()
    emit("u2_eq_nm1", Q, rng.randrange(1, N), N - 1)
    j, Q = key()
    u2 = sum(rng.randrange(8, 16) << (4 * w) for w in range(95)) | (rng.randrange(8, 15) << 380)
    emit("u2_nibbles_ge8", Q, rng.randrange(1, N), u2)
    j, Q = key()
    emit("u2_all_nibbles_8", Q, rng.randrange(1, N), int("8" * 96, 16))
    # u1 = 0 (e = 0 mod n)
    j, Q = key()
    emit("u1_zero", Q, 0, rng.randrange(1, N))
    j, Q = key()
    emit("u1_zero_u2_one_digit", Q, 0, 11 * 16 ** 33, twin=False)
    # x(R) in [n, p): Q = (W - u1 G) / u2 for a point W with such an x
    for i in range(2):
        W = find_wrap_point(rng)
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        m = O.scalar_mult(C, u1, G)
        D = O.point_add(C, W, (m[0], (-m[1]) % P))
        Q = O.scalar_mult(C, pow(u2, -1, N), D)
        assert O.on_curve(C, *Q)
        assert O.point_add(C, m, O.scalar_mult(C, u2, Q)) == W and N <= W[0] < P
        emit(f"xwrap{i}", Q, u1, u2)
    # ordinary records among them
    for i in range(4):
        j, Q = key()
        emit(f"random{i}", Q, rng.randrange(1, N), rng.randrange(1, N), twin=(i == 0))
    return out


def check_libcrypto(recs):
    """OpenSSL's verdict on every record (it knows no low-S rule)."""
    lc = U.LibCrypto()
    for r in recs:
        k = lc.key(None, int(r["qx"], 16), int(r["qy"], 16))
        assert k is not None, r["tag"]
        want = r.get("reason_no_low_s", r["reason"]) == O.R_OK
        assert lc.verify(k, bytes.fromhex(r["digest"]), bytes.fromhex(r["sig"])) == want, r["tag"]
        lc.free_key(k)


def main():
    recs = records()
    tags = [r["tag"] for r in recs]
    assert len(set(tags)) == len(tags)
    for r in recs:
        nl = r.get("reason_no_low_s", r["reason"])
        bad = r["tag"].endswith("_wrong_r") or r["tag"].startswith("final_infinity")
        assert nl == (O.R_MATH if bad else O.R_OK), (r["tag"], nl)
    check_libcrypto(recs)
    with open(OUT, "w") as f:
        for r in recs:
            f.write(json.dumps(r, sort_keys=True) + "\n")
    print(f"{len(recs)} records -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
