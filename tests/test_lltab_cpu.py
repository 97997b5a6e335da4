"""CPU: the per-batch comb table build with sign-paired entries (verify.h
lltab_build / ll_walk), compiled for the host by the TEST-ONLY harness
tests/native_lltab/hostsim_lltab.cpp, against Python integers and the oracle's
affine point arithmetic; ec30.h j_dbl against the affine doubling on the same
keys; and the stand-alone sanitizer run of the build's scratch layout
(tests/native_lltab/lltab_selftest.cpp). A missing harness FAILS these tests:
`make` builds it.

Entry m of a key Q's table must be the point
    E[m] = (2^(s (t-1)) + sum_(i < t-1) (2 m_i - 1) 2^(s i)) Q,
for all 2^(t-1) entries of every key (none sampled). The expected points come
from a Gray walk over m with the oracle's point_add (E[m ^ 2^i] = E[m] +- 2 B_i,
B_i = 2^(s i) Q by scalar_mult), and for two keys per curve also from one
scalar_mult per entry, so the walk itself is checked.

Keys: 32 seeded random ones, G, keys whose x or y -- as the plain integer and as
the Montgomery value x 2^270 mod p the build loads -- has 30-bit limbs that are
zero or all ones (x chosen, y a square root; y chosen, x a root of the cubic),
and a key with y = p - k for the smallest k that is on the curve.

No new field primitive exists to check here: the fused Y3 of the doubling
(a product plus a square under one reduction) was not built, because its second
product 8 gamma^2 = 2 (2 gamma)^2 is not the square of a normalised operand and
its doubled columns do not fit 64 bits; j_dbl is as it was.
"""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import ecdsa_ref as O
from tests.conftest import ROOT
from tests.test_fused_cpu import (K1, P256, M, R, affine_of, from9, jac, normalised, to9, xyz)

LIB = os.path.join(ROOT, "tests", "native", "build", "libhostsimlltab.so")
SELFTEST = os.path.join(ROOT, "tests", "native", "build", "lltab_selftest")
ORC = {0: O.P256, 1: O.SECP256K1}
CV = {0: P256, 1: K1}


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "tests/native/build/libhostsimlltab.so is not built (make)"
    lib = ctypes.CDLL(LIB)
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.hl_shape.restype = u32
    lib.hl_scratch_words.restype = u32
    lib.hl_lltab.argtypes = [ci, vp, vp, ci, vp, u32, vp]
    lib.hl_lltab.restype = ci
    lib.hl_j_dbl.argtypes = [ci, vp, ci, vp]
    return lib


# ---- roots of a monic cubic mod p (polynomials as coefficient lists, low first) ----
def _trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _pmod(a, m, p):
    a = _trim([x % p for x in a])
    inv = pow(m[-1], -1, p)
    while len(a) >= len(m):
        q = a[-1] * inv % p
        off = len(a) - len(m)
        for i, c in enumerate(m):
            a[off + i] = (a[off + i] - q * c) % p
        _trim(a)
    return a


def _pmulmod(a, b, m, p):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return _pmod(out, m, p)


def _ppowmod(base, e, m, p):
    acc, base = [1], _pmod(base, m, p)
    while e:
        if e & 1:
            acc = _pmulmod(acc, base, m, p)
        base = _pmulmod(base, base, m, p)
        e >>= 1
    return acc


def _pgcd(a, b, p):
    a, b = _trim(list(a)), _trim(list(b))
    while b:
        a, b = b, _pmod(a, b, p)
    inv = pow(a[-1], -1, p)
    return [c * inv % p for c in a]


def _psub(a, b, p):
    n = max(len(a), len(b))
    return _trim([((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % p
                  for i in range(n)])


def cubic_roots(c0, c1, p, rng):
    """the roots in F_p of x^3 + c1 x + c0"""
    f = [c0 % p, c1 % p, 0, 1]
    g = _pgcd(f, _psub(_ppowmod([0, 1], p, f, p), [0, 1], p) or f, p)  # the linear factors
    out, todo = [], [g]
    while todo:
        g = todo.pop()
        if len(g) == 1:
            continue
        if len(g) == 2:
            out.append(-g[0] % p)
            continue
        h = _psub(_ppowmod([rng.randrange(p), 1], (p - 1) // 2, g, p), [1], p)
        d = _pgcd(g, h, p) if h else g
        if 1 < len(d) < len(g):
            todo += [d, _trim(_poly_div(g, d, p))]
        else:
            todo.append(g)  # another shift
    return out


def _poly_div(a, m, p):
    a = [x % p for x in a]
    inv = pow(m[-1], -1, p)
    q = [0] * (len(a) - len(m) + 1)
    while len(a) >= len(m):
        c = a[-1] * inv % p
        off = len(a) - len(m)
        q[off] = c
        for i, x in enumerate(m):
            a[off + i] = (a[off + i] - c * x) % p
        a.pop()
    return q


def _sqrt(v, p):  # p = 3 mod 4 on both curves
    r = pow(v, (p + 1) // 4, p)
    return r if r * r % p == v % p else None


_FIXED_LIMBS = ({0: 0, 4: M, 7: 0}, {0: M, 1: M, 5: 0}, {2: 0, 3: 0, 6: M, 8: 0},
                {1: 0, 2: M, 7: M, 8: 0xfffe})


def _with_limbs(fixed, rng):
    """a value < 2^256 with the given 30-bit limbs (0 or all ones; limbs 0 and 8
    at either edge) and random limbs between, so that a curve point exists"""
    limbs = [fixed.get(i, rng.randrange(1 << 30)) for i in range(8)]
    limbs.append(fixed.get(8, rng.randrange(1 << 16)))
    return sum(l << (30 * i) for i, l in enumerate(limbs))


def special_keys(curve, rng):
    """[(tag, (x, y))]: see the module docstring"""
    c, cv = ORC[curve], CV[curve]
    p = c.p
    out = []

    def from_x(x):
        y = _sqrt((x * x * x + c.a * x + c.b) % p, p)
        return None if y is None else (x, y)

    def from_y(y):
        xs = cubic_roots(c.b - y * y, c.a, p, rng)
        return (xs[0], y) if xs else None

    for mont in (False, True):
        for which, make in (("x", from_x), ("y", from_y)):
            for k, fixed in enumerate(_FIXED_LIMBS):
                pt = None
                while pt is None:
                    v = _with_limbs(fixed, rng)
                    if v < p:
                        pt = make(v * cv.rinv % p if mont else v)
                got = pt[which == "y"]
                assert (cv.mont(got) if mont else got) == v
                out.append((f"{which}{'_mont' if mont else ''}{k}", pt))
    for k in range(1, 200):  # y close to p
        pt = from_y(p - k)
        if pt:
            out.append((f"y=p-{k}", pt))
            break
    assert len(out) == 17 and all(O.on_curve(c, *pt) for _t, pt in out)
    return out


_KEYS = {}


def keys_of(curve):
    if curve not in _KEYS:
        c = ORC[curve]
        rng = random.Random(384 + curve)
        ks = [(f"rand{i}", O.scalar_mult(c, rng.randrange(1, c.n), (c.gx, c.gy)))
              for i in range(32)]
        ks.append(("G", (c.gx, c.gy)))
        _KEYS[curve] = ks + special_keys(curve, rng)
    return _KEYS[curve]


def entry_scalar(m, t, s):
    return (1 << (s * (t - 1))) + sum((2 * ((m >> i) & 1) - 1) << (s * i) for i in range(t - 1))


def expected_table(c, Q, t, s):
    """E[0 .. 2^(t-1)) by a Gray walk of affine additions of +-2 B_i"""
    p = c.p
    B = [O.scalar_mult(c, 1 << (s * i), Q) for i in range(t)]
    D = [O.point_add(c, b, b) for b in B[:-1]]
    E = [None] * (1 << (t - 1))
    cur = B[t - 1]
    for b in B[:-1]:
        cur = O.point_add(c, cur, (b[0], -b[1] % p))
    E[0] = cur
    g = 0
    for w in range(1, 1 << (t - 1)):
        i = (w & -w).bit_length() - 1
        g ^= 1 << i
        d = D[i] if (g >> i) & 1 else (D[i][0], -D[i][1] % p)
        cur = O.point_add(c, cur, d)
        E[g] = cur
    return E


def build(L, curve, Q, sep=0):
    cv = CV[curve]
    words = 64 * 20 if sep else L.hl_scratch_words()
    tab = (ctypes.c_uint32 * words)()
    canon = (ctypes.c_uint32 * (64 * 18))()
    assert L.hl_lltab(curve, to9(cv.mont(Q[0])), to9(cv.mont(Q[1])), sep, tab, words, canon) == 0
    return tab, canon


@pytest.mark.parametrize("curve", [0, 1])
def test_every_entry_of_every_key(L, curve):
    shape = L.hl_shape()
    t, s, a = shape & 0xff, (shape >> 8) & 0xff, shape >> 16
    assert (t, s, a) == (7, 37, 3) and L.hl_scratch_words() == 2500
    c, cv = ORC[curve], CV[curve]
    p = c.p
    keys = keys_of(curve)
    assert len(keys) == 32 + 1 + 17
    for kn, (tag, Q) in enumerate(keys):
        want = expected_table(c, Q, t, s)
        if kn in (0, 32):  # the walk against one scalar_mult per entry
            assert want == [O.scalar_mult(c, entry_scalar(m, t, s), Q) for m in range(64)]
        for sep in ((0, 1) if kn % 8 == 0 else (0,)):
            tab, canon = build(L, curve, Q, sep)
            for m in range(64):
                got = (from9(canon, 18 * m), from9(canon, 18 * m + 9))
                assert got == want[m], (tag, sep, m)
                # as the comb reads them: normalised, beta 34 (<= the comb's 64),
                # the same point in the Montgomery domain
                for o, v in ((20 * m, want[m][0]), (20 * m + 9, want[m][1])):
                    assert normalised(tab, o) and from9(tab, o) < 34 * p
                    assert from9(tab, o) % p == cv.mont(v)


@pytest.mark.parametrize("curve", [0, 1])
def test_j_dbl_on_the_keys(L, curve):
    """r = 2 p against the affine doubling, inputs at j_dbl's stated limits
    (X 100 p, Y + Z 128 p) and at beta 1, in place and not."""
    c, cv = ORC[curve], CV[curve]
    p = c.p
    rng = random.Random(3 + curve)
    out = (ctypes.c_uint32 * 27)()
    for it, (tag, Q) in enumerate(keys_of(curve)):
        want = O.point_add(c, Q, Q)
        for betas, top in (((100, 94, 34), True), ((100, 64, 64), it & 1), ((1, 1, 1), False)):
            Pj = xyz(*jac(cv, Q, rng, *betas, top, z=1 if betas == (1, 1, 1) else None))
            for in_place in (0, 1):
                L.hl_j_dbl(curve, Pj, in_place, out)
                assert affine_of(cv, out) == want, tag
                assert all(normalised(out, o) for o in (0, 9, 18))
                assert from9(out, 0) < 34 * p and from9(out, 9) < 34 * p
                assert from9(out, 18) < (34 if curve == 0 else 4) * p


def test_scratch_layout_selftest():
    """lltab_build into exactly-sized heap buffers under AddressSanitizer and
    UBSan, as a stand-alone program (both curves, both scratch placements)."""
    b = subprocess.run(["make", "-C", ROOT, os.path.relpath(SELFTEST, ROOT)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([SELFTEST], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
