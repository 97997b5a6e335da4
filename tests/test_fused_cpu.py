"""CPU: the fused forms of the radix-2^30 field and point formulas (fp30.h f_mul2,
f_negk, f_dblsub; ec30.h j_madd / j_add with one reduction for Y3, the co-Z
addition without the partner update j_zaddc; verify.h ll_dbladd / j_dbladd on
top of them), compiled for the host by tests/native_fused/hostsim_fused.cpp and
checked against Python integers and affine curve arithmetic.

f_mul2(a, b, c, d) needs beta_a beta_b + beta_c beta_d <= 16000 and returns
t == (a b + c d) 2^-270 (mod p), normalised, t < 2p. It exists on P-256 only:
secp256k1's formulas keep two products (fp30.h says why), and the point tests
below run on both curves. Operands sit
at the contract's edges: beta p - 1, every low limb 2^30 - 1 with the largest
admissible top limb, 0, p -- a 64-bit column overflow shows as a wrong value."""
import ctypes
import os
import random

import pytest

from tests.conftest import ROOT

M = 2**30 - 1
R = 2**270
LIB = os.path.join(ROOT, "tests", "native", "build", "libhostsimfused.so")


class Curve:
    def __init__(self, idx, p, a, b, gx, gy, n):
        self.idx, self.p, self.a, self.b, self.g, self.n = idx, p, a, b, (gx, gy), n
        self.rinv = pow(R, -1, p)

    def add(self, P1, P2):
        if P1 is None:
            return P2
        if P2 is None:
            return P1
        p = self.p
        (x1, y1), (x2, y2) = P1, P2
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = (3 * x1 * x1 + self.a) * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return x3, (lam * (x1 - x3) - y1) % p

    def neg(self, P1):
        return None if P1 is None else (P1[0], (-P1[1]) % self.p)

    def mul(self, k, P1):
        acc = None
        while k:
            if k & 1:
                acc = self.add(acc, P1)
            P1 = self.add(P1, P1)
            k >>= 1
        return acc

    def mont(self, v):
        return v * R % self.p


P256 = Curve(0, 2**256 - 2**224 + 2**192 + 2**96 - 1, -3,
             0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b,
             0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
             0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5,
             0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551)
K1 = Curve(1, 2**256 - 2**32 - 977, 0, 7,
           0x79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798,
           0x483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8,
           0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141)
CURVES = {0: P256, 1: K1}


@pytest.fixture(scope="module")
def L():
    # a missing harness FAILS these tests: nothing here needs hardware
    assert os.path.exists(LIB), "tests/native/build/libhostsimfused.so is not built (make)"
    return ctypes.CDLL(LIB)


def to9(v):
    l = [(v >> (30 * i)) & M for i in range(8)] + [v >> 240]
    assert 0 <= l[8] < 2**32
    return (ctypes.c_uint32 * 9)(*l)


def from9(a, off=0):
    return sum(int(a[off + i]) << (30 * i) for i in range(9))


def normalised(a, off=0):
    return all(int(a[off + i]) <= M for i in range(8))


def all_ones(beta, p):
    """limbs 0..7 at 2^30 - 1 with limb 8 at its maximum for a value < beta p"""
    low = sum(M << (30 * i) for i in range(8))
    top = (beta * p - 1 - low) >> 240
    return low + (top << 240)


def edges(beta, p, rng, k):
    hi = beta * p - 1
    vals = [hi, all_ones(beta, p), 0, p, hi - p + 1]
    for _ in range(2):  # low limbs each 0 or 2^30 - 1, top limb as large as allowed
        low = sum((M if rng.random() < 0.5 else 0) << (30 * i) for i in range(8))
        vals.append(low + (((hi - low) >> 240) << 240))
    vals += [rng.randrange(hi + 1) for _ in range(k)]
    return [v for v in vals if 0 <= v <= hi]


# (beta_a, beta_b, beta_c, beta_d): the formulas' own pairs -- j_madd 98*40 + 97*2
# (Y1 a negated table y), j_add 34*40 + 33*2, j_zaddc 36*66 + 2*34 -- the issue's
# (98, 40) + (94, 2) and (128, 66) + (64, 34), and sums exactly at 16000
MUL2_BETAS = [(98, 40, 97, 2), (98, 40, 94, 2), (34, 40, 33, 2), (36, 66, 2, 34),
              (128, 66, 64, 34), (100, 100, 100, 60), (125, 64, 64, 125), (8000, 1, 1, 8000),
              (2, 2, 2, 2), (16000, 1, 1, 0)]


@pytest.mark.parametrize("betas", MUL2_BETAS)
def test_f_mul2_bounds(L, betas):
    cv = P256
    p = cv.p
    ba, bb, bc, bd = betas
    assert ba * bb + bc * bd <= 16000
    rng = random.Random(hash(betas) % 9973)
    out = (ctypes.c_uint32 * 9)()

    def check(a, b, c, d):
        L.hf_f_mul2(to9(a), to9(b), to9(c), to9(d), out)
        t = from9(out)
        assert normalised(out)
        assert t < 2 * p, betas
        assert t % p == (a * b + c * d) * cv.rinv % p, betas

    A, B = edges(ba, p, rng, 4), edges(bb, p, rng, 1)
    C, D = (edges(bc, p, rng, 1), edges(bd, p, rng, 1)) if bd else ([bc * p - 1, 0], [0])
    # every operand at its largest value, and at all-ones limbs, at once
    check(ba * p - 1, bb * p - 1, bc * p - 1, max(bd * p - 1, 0))
    check(all_ones(ba, p), all_ones(bb, p), all_ones(bc, p), all_ones(bd, p) if bd else 0)
    for a in A:
        for b in B[:5]:
            for c in C[:4]:
                for d in D[:4]:
                    check(a, b, c, d)


@pytest.mark.parametrize("curve", [0, 1])
def test_f_negk_dblsub(L, curve):
    p = CURVES[curve].p
    rng = random.Random(5 + curve)
    out = (ctypes.c_uint32 * 9)()
    for a in edges(94, p, rng, 20) + [96 * p]:
        L.hf_f_negk96(curve, to9(a), out)
        assert normalised(out) and from9(out) == 96 * p - a
    for K in (32, 64):
        for a in edges(2, p, rng, 6) + edges(34, p, rng, 4):
            for b in edges(K, p, rng, 6) + [K * p]:
                L.hf_f_dblsub(curve, K, to9(a), to9(b), out)
                assert normalised(out) and from9(out) == 2 * a - b + K * p


# ---- points ------------------------------------------------------------------

def lift(v, beta, p, rng, top=False):
    """a representative of v mod p below beta p (the largest one when top)"""
    kmax = (beta * p - 1 - v) // p
    return v + (kmax if top else rng.randrange(kmax + 1)) * p


def jac(cv, Pt, rng, bx, by, bz, top=True, z=None):
    """Montgomery-domain Jacobian coordinates of the affine Pt at the given betas"""
    p = cv.p
    z = rng.randrange(1, p) if z is None else z
    x, y = Pt
    return (lift(cv.mont(x * z * z % p), bx, p, rng, top),
            lift(cv.mont(y * z * z * z % p), by, p, rng, top),
            lift(cv.mont(z), bz, p, rng, top))


def xyz(X, Y, Z):
    return (ctypes.c_uint32 * 27)(*(list(to9(X)) + list(to9(Y)) + list(to9(Z))))


def affine_of(cv, buf):
    p = cv.p
    X, Y, Z = (from9(buf, o) * cv.rinv % p for o in (0, 9, 18))
    if Z == 0:
        return None
    zi = pow(Z, -1, p)
    return X * zi * zi % p, Y * zi * zi * zi % p


def out_bounds(cv, buf, fused=True):
    """the output contract: normalised, beta (34, 2, 2) where Y3 is one f_mul2
    (P-256), (34, 34, 2) where it is two products (secp256k1, the ladder's composite)"""
    p = cv.p
    assert all(normalised(buf, o) for o in (0, 9, 18))
    assert from9(buf, 0) < 34 * p and from9(buf, 18) < 2 * p
    assert from9(buf, 9) < (2 if cv.idx == 0 and fused else 34) * p


def rand_point(cv, rng):
    return cv.mul(rng.randrange(1, cv.n), cv.g)


@pytest.mark.parametrize("curve", [0, 1])
def test_j_madd_fused(L, curve):
    """r = p + (x2, +-y2): inputs at the stated limits (X1 63 p, Y1 94 p, Z1 34 p,
    x2 / y2 64 p); Y1 also as a negated table y (64 p - y: the f_csub<96> case)."""
    cv = CURVES[curve]
    p = cv.p
    rng = random.Random(11 + curve)
    out = (ctypes.c_uint32 * 27)()
    for it in range(24):
        A, T = rand_point(cv, rng), rand_point(cv, rng)
        neg = it & 1
        top = it % 3 != 2
        if it % 4 < 2:
            X, Y, Z = jac(cv, A, rng, 63, 94, 34, top)
        else:  # Y1 = 64 p - y': A is the negation of a point whose y is y'
            X, _, Z = jac(cv, A, rng, 63, 2, 34, top)
            zv = Z * cv.rinv % p
            yv = cv.mont((-A[1]) % p * pow(zv, 3, p) % p)  # y' < p
            Y = 64 * p - (yv + (p if it % 4 == 3 else 0))
            assert Y % p == cv.mont(A[1] * pow(zv, 3, p) % p)
        x2 = lift(cv.mont(T[0]), 64, p, rng, top)
        y2 = lift(cv.mont(T[1]), 64, p, rng, top)
        for in_place in (0, 1):
            fl = L.hf_j_madd(curve, xyz(X, Y, Z), to9(x2), to9(y2), neg, in_place, out)
            assert fl == 0
            out_bounds(cv, out)
            assert affine_of(cv, out) == cv.add(A, cv.neg(T) if neg else T)


@pytest.mark.parametrize("curve", [0, 1])
def test_j_madd_degenerate_flags(L, curve):
    """x(p) == x(q): degenerate, same_y says p == +-q (with the sign applied)"""
    cv = CURVES[curve]
    p = cv.p
    rng = random.Random(13 + curve)
    out = (ctypes.c_uint32 * 27)()
    for it in range(8):
        A = rand_point(cv, rng)
        X, Y, Z = jac(cv, A, rng, 63, 94, 34, it & 1)
        for T, neg, want in ((A, 0, 3), (A, 1, 1), (cv.neg(A), 0, 1), (cv.neg(A), 1, 3)):
            fl = L.hf_j_madd(curve, xyz(X, Y, Z), to9(lift(cv.mont(T[0]), 64, p, rng)),
                             to9(lift(cv.mont(T[1]), 64, p, rng)), neg, 0, out)
            assert fl == want


@pytest.mark.parametrize("curve", [0, 1])
def test_j_add_fused(L, curve):
    """r = p + q, both Jacobian at beta (63, 63, 34); flags on q == +-p"""
    cv = CURVES[curve]
    rng = random.Random(17 + curve)
    out = (ctypes.c_uint32 * 27)()
    for it in range(16):
        A, T = rand_point(cv, rng), rand_point(cv, rng)
        top = it % 3 != 2
        a = jac(cv, A, rng, 63, 63, 34, top)
        t = jac(cv, T, rng, 63, 63, 34, top)
        for in_place in (0, 1):
            assert L.hf_j_add(curve, xyz(*a), xyz(*t), in_place, out) == 0
            out_bounds(cv, out)
            assert affine_of(cv, out) == cv.add(A, T)
        assert L.hf_j_add(curve, xyz(*a), xyz(*jac(cv, A, rng, 63, 63, 34, top)), 0, out) == 3
        assert L.hf_j_add(curve, xyz(*a), xyz(*jac(cv, cv.neg(A), rng, 63, 63, 34, top)), 0,
                          out) == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_j_zaddc(L, curve):
    """The co-Z addition without the partner update on its own inputs: P1 = (x1,
    y1, z) and P2 = (x2, sy - y1, z) with dx = x1 - x2, at beta (2, 2, 34, 40, 2, 2)."""
    cv = CURVES[curve]
    p = cv.p
    rng = random.Random(19 + curve)
    out = (ctypes.c_uint32 * 27)()
    for it in range(24):
        A, T = rand_point(cv, rng), rand_point(cv, rng)
        top = it % 3 != 2
        z = rng.randrange(1, p)
        x1, y1, zz = jac(cv, A, rng, 2, 2, 2, top, z)
        x2, y2, _ = jac(cv, T, rng, 34, 1, 2, top, z)
        dx = lift((x1 - x2) % p, 40, p, rng, top)
        sy = lift((y1 + y2) % p, 2, p, rng, top)
        L.hf_j_zaddc(curve, to9(x1), to9(y1), to9(x2), to9(dx), to9(sy), to9(zz), out)
        out_bounds(cv, out)
        assert affine_of(cv, out) == cv.add(A, T)


def composite_cases(cv, rng):
    """(A, a_inf, T, want point, want a_inf) for 2 A + T, T already signed"""
    A, T = rand_point(cv, rng), rand_point(cv, rng)
    yield A, 0, T, cv.add(cv.add(A, A), T), 0
    yield A, 1, T, T, 0                                     # A at infinity -> T
    yield A, 0, A, cv.mul(3, A), 0                          # A == T -> 3 T
    yield A, 0, cv.neg(A), A, 0                             # A == -T -> A, unchanged
    yield A, 0, cv.neg(cv.add(A, A)), None, 1               # A + T == -A -> infinity


@pytest.mark.parametrize("curve", [0, 1])
def test_ll_dbladd(L, curve):
    """A = 2 A + (tx, +-ty) (the comb's Horner step) with its explicit degenerate
    cases; A at beta (63, 94, 34), the table point at 64 p."""
    cv = CURVES[curve]
    p = cv.p
    rng = random.Random(23 + curve)
    for it in range(10):
        top = it % 3 != 2
        for A, a_inf, T, want, want_inf in composite_cases(cv, rng):
            for neg in (0, 1):
                Tin = cv.neg(T) if neg else T  # the table holds -T when the sign is applied
                a = xyz(*jac(cv, A, rng, 63, 94, 34, top))
                before = list(a)
                tx = to9(lift(cv.mont(Tin[0]), 64, p, rng, top))
                ty = to9(lift(cv.mont(Tin[1]), 64 if not neg else 63, p, rng, top))
                got_inf = L.hf_ll_dbladd(curve, a, a_inf, tx, ty, neg)
                assert got_inf == want_inf
                if want_inf:
                    continue
                assert affine_of(cv, a) == want
                if not a_inf and T == cv.neg(A):
                    assert list(a) == before  # A == -T leaves A as it was
                elif not a_inf and T != A:
                    out_bounds(cv, a)


def test_j_dbladd(L):
    """A = 2 A + (+-T) for a Jacobian T (P-256's odd-window ladder)"""
    cv = P256
    rng = random.Random(29)
    for it in range(10):
        top = it % 3 != 2
        for A, a_inf, T, want, want_inf in composite_cases(cv, rng):
            for neg in (0, 1):
                Tin = cv.neg(T) if neg else T
                a = xyz(*jac(cv, A, rng, 63, 63, 34, top))
                before = list(a)
                t = xyz(*jac(cv, Tin, rng, 63, 63 if not neg else 31, 34, top))
                got_inf = L.hf_j_dbladd(a, a_inf, t, neg)
                assert got_inf == want_inf
                if want_inf:
                    continue
                assert affine_of(cv, a) == want
                if not a_inf and T == cv.neg(A):
                    assert list(a) == before
                elif not a_inf and T != A:
                    out_bounds(cv, a, fused=False)  # j_add_da: j_zaddc with two products
