#!/usr/bin/env python3
"""Generate tests/golden/p384_comb_vectors.jsonl: crafted records for the comb
route of the P-384 pass (stage384_comb, bdls_amd/csrc/comb384.h,
BH_F_BATCH_KEYS). Run from the repo root:
    python tests/golden/gen_golden_p384_comb.py

The route starts from A = infinity and, for column c = 63..0, doubles A, adds
TQ[dq] (dq: bit c of the six 64-bit chunks of u2) and adds TG[dg] (the same of
u1), where T[d] = K(d) * base, K(d) = sum of 2^(64 j) over the bits j of d. u1 G
is folded into the walk of u2 Q, so the accumulator is what the input makes
it. Each record fixes u1, u2 and Q = j G so that the walk meets a chosen
situation: R = u1 G + u2 Q, r = x(R) mod n, s = r / u2, e = u1 s, the digest
is e's 48 bytes. The free parameters are drawn again until s (and the wrong-r
twin's s) is at most n / 2: every record passes Fabric's low-S rule, so with
four records per key the whole file rides the comb route. Expectations come
from oracle/ecdsa_ref.py on the P-384 curve; walk() replays the column walk on
Python integers and main() asserts that each situation named by a tag occurs.

Situations (c: the column):
  q_dbl_c*      the Q addition finds 2A == TQ[dq]: the doubling branch
  q_neg_c*      the Q addition finds 2A == -TQ[dq]: infinity mid-walk
  g_dbl_c*      the G addition finds A == TG[dg]  (c63_qG: Q = G, equal top digits)
  g_neg_c*      the G addition finds A == -TG[dg] (c63_qnegG: Q = -G; infinity is
                then doubled and added to again; c0: the walk's last addition, so
                the sum is infinite)
  final_inf     u1 G = -u2 Q: infinity at the end, BH_R_MATH
  small         u1, u2 < 2^64: five of the six chunks are zero
  u2_1, u2_2, u2_nm1, u1_zero (e = 0: the walk is Q's alone)
  digits        digit 63 (all teeth) and digit 32 (the top tooth alone) in both scalars
  xwrap*        x(R) in [n, p): the r + n candidate decides
  *_wrong_r     the same walk against a slightly larger r: BH_R_MATH
  *_rep         a second copy, so that every key has four records
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
from tests.golden.gen_golden_p384 import b48, find_wrap_point, rec  # noqa: E402
from tests.p384_util import HALF, N, P, P384 as C  # noqa: E402

G = (C.gx, C.gy)
OUT = os.path.join(HERE, "p384_comb_vectors.jsonl")


def K(d: int) -> int:
    return sum(1 << (64 * j) for j in range(6) if (d >> j) & 1)


def digit(u: int, c: int) -> int:
    return sum(((u >> (64 * j + c)) & 1) << j for j in range(6))


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def walk(u1: int, u2: int, Q):
    """The comb route's walk on affine points: (final point, events). Events:
    (kind, column) with kind q_dbl / q_neg / g_dbl / g_neg for an addition whose
    operands are equal / opposite, inf_dbl for a doubling of an infinity that
    arose mid-walk, add_to_inf for an addition to such an infinity."""
    A, ev, was_finite = None, [], False
    tab = {}

    def entry(base, d):
        key = (base, d)
        if key not in tab:
            tab[key] = O.scalar_mult(C, K(d), base)
        return tab[key]

    for c in range(63, -1, -1):
        if A is None and was_finite:
            ev.append(("inf_dbl", c))
        A = O.point_add(C, A, A)
        for kind, base, u in (("q", Q, u2), ("g", G, u1)):
            d = digit(u, c)
            if not d:
                continue
            T = entry(base, d)
            if A is None and was_finite:
                ev.append(("add_to_inf", c))
            if A is not None and A == T:
                ev.append((kind + "_dbl", c))
            if A is not None and A == neg(T):
                ev.append((kind + "_neg", c))
            A = O.point_add(C, A, T)
            was_finite = True
    return A, ev


def records():
    rng = random.Random(384_0128)
    out, checks = [], []
    sig_of = O.marshal_ecdsa_signature

    def emit(tag, make, twin=True, want_events=(), final_inf=False, check=None):
        """make() -> (Q, u1, u2, r or None): drawn again until the low-S rule
        passes for the record and its twin. want_events: events the walk must
        show, in order of appearance among its events."""
        while True:
            Q, u1, u2, r = make()
            assert 0 <= u1 < N and 0 < u2 < N and O.on_curve(C, *Q)
            R = O.double_scalar(C, u1, u2, Q)
            if r is None:
                r = (R[0] % N) if R is not None else rng.randrange(1, N)
            if r == 0:
                continue
            s = r * pow(u2, -1, N) % N
            # the twin's r: the nearest above r whose s passes the low-S rule too
            r2, s2 = next(((x, x * pow(u2, -1, N) % N) for x in range(r + 1, r + 9)
                           if x < N and 0 < x * pow(u2, -1, N) % N <= HALF), (0, 0))
            if 0 < s <= HALF and (not twin or r2):
                break
        A, ev = walk(u1, u2, Q)
        assert A == R, tag
        assert (A is None) == final_inf, tag
        it = iter(ev)
        assert all(e in it for e in want_events), (tag, ev, want_events)
        if not want_events and not final_inf:
            assert not ev, (tag, ev)
        if check:
            check(Q, u1, u2, R)
        pair = [rec(tag, Q[0], Q[1], sig_of(r, s), digest=b48(u1 * s % N))]
        if twin:
            pair.append(rec(tag + "_wrong_r", Q[0], Q[1], sig_of(r2, s2), digest=b48(u1 * s2 % N)))
        else:
            pair.append(dict(pair[0], tag=tag + "_again"))
        for x in pair:
            want = O.R_MATH if (final_inf or x["tag"].endswith("_wrong_r")) else O.R_OK
            assert x["reason"] == want and "reason_no_low_s" not in x, x["tag"]
        out.extend(pair)
        out.extend(dict(x, tag=x["tag"] + "_rep") for x in pair)

    def scalar_with_digit(c, lo=0):
        while True:
            u = rng.randrange(1 << 383, N) if not lo else rng.randrange(1, N)
            if digit(u, c):
                return u

    def hi_part(u, c):
        """The scalar that the columns above c have contributed to the accumulator
        by the time it has been doubled at column c: sum 2^(c' - c) K(digit c')."""
        return sum(K(digit(u, cc)) << (cc - c) for cc in range(c + 1, 64))

    def solve(kind, sign, c):
        """(Q = j G, u1, u2, None) whose walk meets `kind` at column c: the
        accumulator's scalar is linear in j, so the coincidence fixes j."""
        def make():
            while True:
                u1, u2 = scalar_with_digit(c), scalar_with_digit(c)
                a1, a2 = hi_part(u1, c), hi_part(u2, c)  # 2A = (a2 j + a1) G
                if kind == "q":    # a2 j + a1 = sign K(dq) j
                    num, den = -a1, a2 - sign * K(digit(u2, c))
                else:              # a2 j + a1 + K(dq) j = sign K(dg)
                    num, den = sign * K(digit(u1, c)) - a1, a2 + K(digit(u2, c))
                if den % N == 0 or num % N == 0:
                    continue
                j = num * pow(den, -1, N) % N
                return O.pubkey(C, j), u1, u2, None
        return make

    # the Q addition: 2A is the entry (doubling) or its negative (infinity)
    for c in (31, 0):
        emit(f"q_dbl_c{c}", solve("q", 1, c), want_events=[("q_dbl", c)])
        emit(f"q_neg_c{c}", solve("q", -1, c), want_events=[("q_neg", c), ("add_to_inf", c)])
    # the G addition
    for c in (63, 31, 0):
        emit(f"g_dbl_c{c}", solve("g", 1, c), want_events=[("g_dbl", c)])
        if c:
            emit(f"g_neg_c{c}", solve("g", -1, c), want_events=[("g_neg", c), ("inf_dbl", c - 1)])
        else:  # the last addition of the walk: the sum is infinite
            emit("g_neg_c0_final_inf", solve("g", -1, 0), twin=False, final_inf=True,
                 want_events=[("g_neg", 0)])

    def same_top(q):
        def make():
            while True:
                u1, u2 = scalar_with_digit(63), scalar_with_digit(63)
                u2 = (u2 & ~sum(1 << (64 * j + 63) for j in range(6))) | \
                    sum(((u1 >> (64 * j + 63)) & 1) << (64 * j + 63) for j in range(6))
                if 0 < u2 < N and digit(u1, 63) == digit(u2, 63):
                    return q, u1, u2, None
        return make
    emit("g_dbl_c63_qG", same_top(G), want_events=[("g_dbl", 63)])
    emit("g_neg_c63_qnegG", same_top(neg(G)),
         want_events=[("g_neg", 63), ("inf_dbl", 62), ("add_to_inf", 62)])

    def key():
        j = rng.randrange(2, N)
        return j, O.pubkey(C, j)

    # infinity at the end
    def final_inf():
        j, Q = key()
        u2 = rng.randrange(1, N)
        return Q, (-u2 * j) % N, u2, None
    emit("final_inf", final_inf, twin=False, final_inf=True)

    # leading zero columns and chunks
    def small():
        return key()[1], rng.randrange(1 << 60, 1 << 64), rng.randrange(1 << 60, 1 << 64), None

    def check_small(Q, u1, u2, R):
        assert u1 < 1 << 64 and u2 < 1 << 64
    emit("small", small, check=check_small)
    for name, v in (("u2_1", 1), ("u2_2", 2), ("u2_nm1", N - 1)):
        emit(name, lambda v=v: (key()[1], rng.randrange(1, N), v, None))
    emit("u1_zero", lambda: (key()[1], 0, rng.randrange(1, N), None))

    # digit 63 (all teeth) and digit 32 (top tooth alone) in both scalars
    def digits():
        def shape(u):
            u &= ~(K(63) << 5) & ~(K(63) << 9)
            return u | (K(63) << 5) | (K(32) << 9)
        while True:
            u1, u2 = shape(rng.randrange(1, 1 << 383)), shape(rng.randrange(1, 1 << 383))
            if u1 < N and u2 < N:
                return key()[1], u1, u2, None

    def check_digits(Q, u1, u2, R):
        for u in (u1, u2):
            assert digit(u, 5) == 63 and digit(u, 9) == 32
    emit("digits", digits, check=check_digits)

    # x(R) in [n, p): Q = (W - u1 G) / u2 for a point W with such an x
    for i in range(2):
        def xwrap():
            W = find_wrap_point(rng)
            u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
            D = O.point_add(C, W, neg(O.scalar_mult(C, u1, G)))
            return O.scalar_mult(C, pow(u2, -1, N), D), u1, u2, None

        def check_wrap(Q, u1, u2, R):
            assert N <= R[0] < P  # r = x - n, and r + n = x < p
        emit(f"xwrap{i}", xwrap, check=check_wrap)

    # ordinary records among them
    for i in range(2):
        emit(f"random{i}", lambda: (key()[1], rng.randrange(1, N), rng.randrange(1, N), None))
    return out


def main():
    recs = records()
    tags = [r["tag"] for r in recs]
    assert len(set(tags)) == len(tags) and len(recs) <= 400
    by_key = {}
    for r in recs:
        assert r["reason"] in (O.R_OK, O.R_MATH)  # every record passes prep
        by_key[r["qx"] + r["qy"]] = by_key.get(r["qx"] + r["qy"], 0) + 1
    assert min(by_key.values()) >= 4
    with open(OUT, "w") as f:
        for r in recs:
            f.write(json.dumps(r, sort_keys=True) + "\n")
    print(f"{len(recs)} records over {len(by_key)} keys -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
