"""CPU: the P-384 device arithmetic (bdls_amd/csrc/{fp384,ec384,verify384}.h, the
functions the gfx950 kernels run) compiled for the host by the TEST-ONLY
harness tests/native/hostsim384.cpp, checked against Python integers, the
oracle (oracle/ecdsa_ref.py on the P-384 curve of tests/p384_util.py) and
OpenSSL libcrypto. Plus the host-only parts of the C ABI for BH_CURVE_P384.
A missing harness FAILS these tests: `make` builds it."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from bdls_amd import _lib
from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests.conftest import GOLDEN
from tests.p384_util import HALF, N, P, P384

W, L14 = 28, 14
R = 1 << (W * L14)
MODS = {0: P, 1: N}


@pytest.fixture(scope="module")
def hs():
    assert os.path.exists(U.HOSTSIM384), "tests/native/build/libhostsim384.so is not built (make)"
    L = ctypes.CDLL(U.HOSTSIM384)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.hs384_field.argtypes = [i32, i32, i32, vp, vp, vp]
    L.hs384_field.restype = i32
    L.hs384_inv.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    L.hs384_gtab_entry.argtypes = [u32, u32, vp]
    L.hs384_verify.argtypes = [vp] * 7 + [u32] * 3 + [vp]
    L.hs384_parse_der.argtypes = [vp, u32, vp, vp, vp]
    L.hs384_parse_der.restype = i32
    L.hs384_point_sum.argtypes = [vp, vp, i32, vp]
    L.hs384_point_sum.restype = i32
    return L


@pytest.fixture(scope="module")
def golden384():
    return U.load_golden384()


def limbs(v):
    assert 0 <= v < R
    return np.array([(v >> (W * i)) & ((1 << W) - 1) for i in range(L14)], np.uint32)


def value(a):
    assert all(int(x) < (1 << W) for x in a), "limb not normalised"
    return sum(int(x) << (W * i) for i, x in enumerate(a))


def words12(v):
    return np.array([(v >> (32 * i)) & 0xffffffff for i in range(12)], np.uint32)


def from_words(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def fop(hs, field, op, a, b=0, k=0):
    """One fp384.h operation through the harness; returns the 14 output limbs."""
    A, B, out = limbs(a), limbs(b), np.zeros(L14, np.uint32)
    assert hs.hs384_field(field, op, k, A.ctypes.data, B.ctypes.data, out.ctypes.data) == 0
    return out


MUL, SQR, ADD, SUB, MULS, CANON, FROM_MONT, TO_MONT, IS_ZERO, IS_ZERO3, COND_SUB, INV = range(12)

# fp384.h's contract: a < alpha m, b < beta m, alpha beta <= 2^15, both < R.
# (23, 69) is the largest pair the point formulas use (the doubling's alpha).
BETA_PAIRS = [(1, 1), (2, 2), (20, 20), (23, 69), (69, 23), (22, 22), (128, 256), (181, 181)]


def edge_values(m, beta, rng):
    top = min(beta * m, R) - 1
    # every limb all-ones below the largest top limb the bound admits
    ones = (top >> (W * 13) << (W * 13)) | ((1 << (W * 13)) - 1)
    if ones > top:
        ones -= 1 << (W * 13)
    vals = [0, 1, m - 1, m, m + 1, top, ones] if beta > 1 else [0, 1, m - 1]
    vals += [rng.randrange(top + 1) for _ in range(6)]
    return [v for v in vals if 0 <= v <= top]


@pytest.mark.parametrize("field", [0, 1])
def test_field_mul_contract(hs, field):
    """Products over the contract's edges for the formulas' largest beta pair
    and for the stated maximum alpha beta = 2^15: the value is a b R^-1 mod m,
    normalised, and below (alpha beta / 256 + 1) m. A column overflow or a
    lost carry would show as a wrong value."""
    m = MODS[field]
    rng = random.Random(384 + field)
    ri = pow(R, -1, m)
    for alpha, beta in BETA_PAIRS:
        assert alpha * beta <= 1 << 15
        for a in edge_values(m, alpha, rng):
            for b in edge_values(m, beta, rng):
                got = value(fop(hs, field, MUL, a, b))
                assert got % m == a * b * ri % m, (alpha, beta, hex(a), hex(b))
                assert got * 256 < (alpha * beta + 256) * m, (alpha, beta, hex(a), hex(b))
                assert got == (a * b + (-(a * b) * pow(m, -1, R) % R) * m) // R
        for a in edge_values(m, min(alpha, 181), rng):
            assert value(fop(hs, field, SQR, a)) % m == a * a * ri % m


@pytest.mark.parametrize("field", [0, 1])
def test_field_add_sub_forms(hs, field):
    m = MODS[field]
    rng = random.Random(3840 + field)
    for k in (2, 3, 6, 8, 9, 16, 18, 20, 32):
        for a in edge_values(m, 200, rng):       # a + k m < R
            for b in edge_values(m, k, rng) + [k * m]:
                out = fop(hs, field, SUB, a, b, k)
                assert value(out) == a + k * m - b, (k, hex(a), hex(b))
    for a in edge_values(m, 100, rng):
        for b in edge_values(m, 100, rng):
            assert value(fop(hs, field, ADD, a, b)) == a + b
    for k in (2, 3, 4, 8):
        for a in edge_values(m, 256 // k - 1, rng):
            assert value(fop(hs, field, MULS, a, k=k)) == k * a
    for a in edge_values(m, 256, rng) + [R - 1]:
        assert value(fop(hs, field, CANON, a)) == a % m
        assert value(fop(hs, field, FROM_MONT, a)) == a * pow(R, -1, m) % m
        assert int(fop(hs, field, IS_ZERO, a)[0]) == (a % m == 0)
    for a in [0, m, 2 * m, 1, m - 1, m + 1, 2 * m - 1, 2 * m + 1, 3 * m - 1]:
        assert int(fop(hs, field, IS_ZERO3, a)[0]) == (a in (0, m, 2 * m)), hex(a)
        assert int(fop(hs, field, IS_ZERO, a)[0]) == (a % m == 0)
    for a in [0, 1, m - 1, m, m + 1, 2 * m - 1]:
        assert value(fop(hs, field, COND_SUB, a)) == a % m
    for a in [0, 1, m - 1, m, 2 * m - 1] + [rng.randrange(2 * m) for _ in range(4)]:
        assert value(fop(hs, field, TO_MONT, a)) % m == a * R % m


def test_scalar_inversion_single(hs):
    rng = random.Random(7)
    for s in [1, 2, N - 1, N - 2, HALF, HALF + 1] + [rng.randrange(1, N) for _ in range(6)]:
        got = value(fop(hs, 1, INV, s * R % N))   # Montgomery form in and out
        assert got * pow(R, -1, N) % N == pow(s, -1, N), hex(s)


def run_inv(hs, e, r, s, valid, chunk):
    n = len(s)
    pk = lambda vs: np.concatenate([words12(v) for v in vs]) if vs else np.zeros(1, np.uint32)
    E, Rr, S = pk(e), pk(r), pk(s)
    V = np.array(valid, np.uint8)
    u1, u2 = np.zeros(12 * n, np.uint32), np.zeros(12 * n, np.uint32)
    hs.hs384_inv(E.ctypes.data, Rr.ctypes.data, S.ctypes.data, V.ctypes.data, n, chunk,
                 u1.ctypes.data, u2.ctypes.data)
    return ([from_words(u1[12 * i:12 * i + 12]) for i in range(n)],
            [from_words(u2[12 * i:12 * i + 12]) for i in range(n)])


@pytest.mark.parametrize("chunk", [1, 7])
def test_scalar_inversion_chunked(hs, chunk):
    """Montgomery's trick per chunk; a rejected record (valid = 0) at every
    position of a chunk, and a chunk with no valid record at all."""
    rng = random.Random(70 + chunk)
    n = 23
    s = [1, 2, N - 1] + [rng.randrange(1, N) for _ in range(n - 3)]
    e = [0, 1, N - 1] + [rng.randrange(N) for _ in range(n - 3)]
    r = [rng.randrange(1, N) for _ in range(n)]
    masks = [[1] * n, [0] * n] + [[0 if i == j else 1 for i in range(n)] for j in range(n)]
    stride = (n + chunk - 1) // chunk
    masks.append([0 if i % stride == 1 % stride else 1 for i in range(n)])  # one whole lane invalid
    for valid in masks:
        u1, u2 = run_inv(hs, e, r, s, valid, chunk)
        for i in range(n):
            w = pow(s[i], -1, N) if valid[i] else 1
            assert u1[i] == e[i] * w % N and u2[i] == r[i] * w % N, (chunk, i, valid)


def test_gtab_entries(hs):
    """Spot entries of the fixed-base table: d 16^w G, affine."""
    for win, d in [(0, 1), (0, 15), (1, 1), (7, 9), (50, 3), (95, 15), (95, 1)]:
        xy = np.zeros(24, np.uint32)
        hs.hs384_gtab_entry(win, d, xy.ctypes.data)
        want = O.scalar_mult(P384, d << (4 * win), (P384.gx, P384.gy))
        assert (from_words(xy[:12]), from_words(xy[12:])) == want, (win, d)


def test_point_operations_exceptional_cases(hs):
    """j384_add / j384_madd / j384_dbl directly: A = aG and T = tG come from
    separate chains (different Z), so a == t is the A == T doubling branch,
    a == -t the infinity branch, 0 an operand at infinity."""
    rng = random.Random(9)
    G = (P384.gx, P384.gy)
    big = rng.randrange(1, N)
    pairs = [(1, 1), (5, 5), (big, big), (N - 1, N - 1), (1, N - 1), (big, N - big), (0, 7), (7, 0),
             (0, 0), (1, 2), (2, 1), (big, 1), (N - 3, N - 3), (3, N - 3), (big, rng.randrange(1, N))]
    for a, t in pairs:
        for mode in range(5):
            if mode in (2, 3) and t == 0:
                continue
            k = {0: a + t, 1: a - t, 2: a + t, 3: a - t, 4: 2 * a}[mode] % N
            want = O.scalar_mult(P384, k, G) if k else None
            xy = np.zeros(24, np.uint32)
            A, T = words12(a), words12(t)
            inf = hs.hs384_point_sum(A.ctypes.data, T.ctypes.data, mode, xy.ctypes.data)
            got = None if inf else (from_words(xy[:12]), from_words(xy[12:]))
            assert got == want, (a, t, mode)


def run_hs(hs, arrs, flags, chunk=7):
    pub, sig, so, sl, msg, mo, ml = arrs
    n = len(sl)
    out = np.full(max(n, 1), 255, np.uint8)
    hs.hs384_verify(pub.ctypes.data, sig.ctypes.data, so.ctypes.data, sl.ctypes.data,
                    msg.ctypes.data, mo.ctypes.data, ml.ctypes.data, n, flags, chunk,
                    out.ctypes.data)
    return out[:n]


def expect(recs, no_low_s):
    return [r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"] for r in recs]


@pytest.mark.parametrize("no_low_s", [False, True])
@pytest.mark.parametrize("chunk", [1, 7])
def test_golden_digest_mode(hs, golden384, chunk, no_low_s):
    out = run_hs(hs, U.pack384(golden384, False), _lib.BH_F_NO_LOW_S if no_low_s else 0, chunk)
    bad = [(r["tag"], int(o), w) for r, o, w in zip(golden384, out, expect(golden384, no_low_s))
           if o != w]
    assert not bad


@pytest.mark.parametrize("no_low_s", [False, True])
@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_golden_fused_mode(hs, golden384, family, no_low_s):
    recs = [r for r in golden384 if r.get("family") == family]
    assert len(recs) >= 11
    flags = (_lib.BH_F_HASH_SHA256 if family == "SHA2" else _lib.BH_F_HASH_SHA3_256) | \
        (_lib.BH_F_NO_LOW_S if no_low_s else 0)
    out = run_hs(hs, U.pack384(recs, True), flags)
    bad = [(r["tag"], int(o), w) for r, o, w in zip(recs, out, expect(recs, no_low_s)) if o != w]
    assert not bad
    # the other family's hash must reject every record that verified
    other = _lib.BH_F_HASH_SHA3_256 if family == "SHA2" else _lib.BH_F_HASH_SHA256
    out2 = run_hs(hs, U.pack384(recs, True), other)
    assert all(o != 0 for r, o in zip(recs, out2) if r["reason"] == 0)


def test_golden_fixture_matches_oracle(golden384):
    """The committed expectations are the oracle's (tests/golden/gen_golden_p384.py)."""
    assert 150 <= len(golden384) <= 210
    assert os.path.getsize(U.GOLDEN384) < 150 * 1024
    for r in golden384:
        got = O.csp_verify(P384, int(r["qx"], 16), int(r["qy"], 16), bytes.fromhex(r["sig"]),
                           bytes.fromhex(r["digest"]))[1]
        assert got == r["reason"], r["tag"]
    tags = {r["tag"] for r in golden384}
    for t in ("digest_len47", "digest_len49", "valid_msg_SHA3_len136", "s_eq_half_valid",
              "s_eq_half_plus1", "high_s", "r_eq_n", "r_n_plus1", "s_eq_n", "r_49byte", "s_49byte",
              "r_zero", "s_neg1", "p256_der_trailing_garbage_ok", "p256_ref_impl_test_der_0",
              "q_offcurve", "q_x_eq_p", "q_y_ge_p", "q_zero", "e_zero_digest", "digest_eq_n",
              "u2_eq_1", "u2_eq_2", "u2_eq_nm1", "q_eq_G", "q_eq_negG", "q_eq_2G",
              "u1G_eq_u2Q_accept", "sum_infinity", "xwrap_accept", "flip_r", "flip_s",
              "flip_digest", "flip_key_x", "u2_eq_nm6", "acc_eq_gentry_w0_d1_q1G",
              "acc_eq_gentry_w0_d1_q1G_wrong_r", "acc_eq_gentry_w3_d5_q1G",
              "acc_eq_gentry_w95_d15_q1G", "acc_eq_gentry_w95_d15_q1G_wrong_r"):
        assert t in tags, t


@pytest.fixture(scope="module")
def libcrypto():
    try:
        return U.LibCrypto()
    except OSError as e:  # the only reason this may skip
        pytest.skip(f"libcrypto cannot be loaded: {e}")


def test_oracle_vs_libcrypto(libcrypto):
    """The Python restatement against OpenSSL on 64 random valid and corrupted
    records at digest lengths 1..64 (no low-S rule, strict-DER inputs only)."""
    rng = random.Random(64)
    for i in range(64):
        d = rng.randrange(1, N)
        qx, qy = O.pubkey(P384, d)
        dg = bytes(rng.getrandbits(8) for _ in range(1 + i))
        k = libcrypto.key(d, qx, qy)
        r, s = libcrypto.sign(k, dg)
        mode = i % 4
        if mode == 1:
            r ^= 1 << rng.randrange(383)
        elif mode == 2:
            dg = bytes([dg[0] ^ 0x10]) + dg[1:]
        elif mode == 3 and i % 8 == 3:
            s = N - s
        sig = O.marshal_ecdsa_signature(r, s)
        want = O.go_ecdsa_verify(P384, qx, qy, dg, r, s) == O.R_OK
        assert libcrypto.verify(k, dg, sig) == want, (i, mode)
        if mode in (0, 3):
            assert want
        libcrypto.free_key(k)


@pytest.fixture(scope="module")
def libcrypto_required():
    return U.LibCrypto()  # a load failure is an error of this test, never a skip


def test_libcrypto_batch_through_harness(hs, libcrypto_required):
    """600 libcrypto-signed records, 24 keys, one in eight corrupted by
    construction: the harness gives the constructed reasons, and libcrypto's
    verdict on every record where low-S and DER do not enter."""
    libcrypto = libcrypto_required
    for family, flag in (("SHA2", _lib.BH_F_HASH_SHA256), ("SHA3", _lib.BH_F_HASH_SHA3_256)):
        recs, want = U.signed_batch(libcrypto, 600, 24, seed=600, family=family)
        assert 60 <= int((want != 0).sum()) <= 90
        out = run_hs(hs, U.pack384(recs, True), flag, chunk=16)
        assert (out == want).all(), np.nonzero(out != want)[0][:10]
        out_d = run_hs(hs, U.pack384(recs, False), 0, chunk=16)
        assert (out_d == want).all()
        for r, w in zip(recs, want):
            if w == O.R_HIGH_S:
                continue
            k = libcrypto.key(None, int(r["qx"], 16), int(r["qy"], 16))
            ok = k is not None and libcrypto.verify(k, bytes.fromhex(r["digest"]),
                                                    bytes.fromhex(r["sig"]))
            assert ok == (w == 0)
            if k is not None:
                libcrypto.free_key(k)


def test_der_8_word_instantiation_unchanged():
    """der.h became a template on the word count; bh_parse_der_sig (8 words)
    still matches the oracle on every signature of the P-256 fixture."""
    from bdls_amd.bccsp import parse_der_sig
    with open(GOLDEN) as f:
        recs = [json.loads(l) for l in f]
    for r in recs:
        sig = bytes.fromhex(r["sig"])
        if not sig:
            continue
        reason, rv, sv = O.unmarshal_ecdsa_signature(sig)
        got, gr, gs = parse_der_sig(sig)
        assert got == reason, r["tag"]
        if reason == O.R_OK:
            assert gr == (rv if rv < 2**256 else None) and gs == (sv if sv < 2**256 else None), r["tag"]


def test_der_12_word_instantiation(hs, golden384):
    for r in golden384:
        sig = bytes.fromhex(r["sig"])
        if not sig:
            continue
        reason, rv, sv = O.unmarshal_ecdsa_signature(sig)
        buf = np.frombuffer(sig, np.uint8)
        ro, so, big = np.zeros(12, np.uint32), np.zeros(12, np.uint32), np.zeros(2, np.uint32)
        got = hs.hs384_parse_der(buf.ctypes.data, len(sig), ro.ctypes.data, so.ctypes.data,
                                 big.ctypes.data)
        assert got == reason, r["tag"]
        if reason == O.R_OK:
            assert bool(big[0]) == (rv >= 2**384) and bool(big[1]) == (sv >= 2**384), r["tag"]
            if not big[0]:
                assert from_words(ro) == rv
            if not big[1]:
                assert from_words(so) == sv


def test_curve_key_bytes():
    L = _lib.lib()
    assert _lib.BH_CURVE_P384 == 2
    assert [L.bh_curve_key_bytes(c) for c in (0, 1, 2)] == [64, 64, 96]
    assert L.bh_curve_key_bytes(3) < 0 and L.bh_curve_key_bytes(-1) < 0


def test_unsupported_entry_points_name_the_curve():
    """Everything but bh_verify / bh_verify_dev answers BH_E_INVALID for
    BH_CURVE_P384, naming the curve, before it looks for a device."""
    L = _lib.lib()
    C = _lib.BH_CURVE_P384
    n = 1
    pub = np.zeros(96, np.uint8)
    sig = np.zeros(8, np.uint8)
    off = np.zeros(1, np.uint64)
    ln = np.array([8], np.uint32)
    bm, rs = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    p = lambda a: a.ctypes.data
    b = _lib.BhBatch(p(pub), p(sig), p(off), p(ln), p(sig), p(off), p(ln))
    cb = _lib.BhCBatch(p(pub), None, 1, p(sig), p(ln), p(sig), p(ln), 0)
    ptrs = np.array([p(pub)], np.uint64)
    pb = _lib.BhPBatch(p(ptrs), p(ptrs), p(ln), p(ptrs), p(ln))
    job = ctypes.c_void_p()
    bd = _lib.BhBdlsBatch(*([p(pub)] * 11))
    cnt = ctypes.c_size_t()
    calls = {
        "bh_verify_2seg": lambda: L.bh_verify_2seg(C, ctypes.byref(b), p(off), p(ln), n, 1, p(bm), p(rs)),
        "bh_verify_submit": lambda: L.bh_verify_submit(C, ctypes.byref(b), n, 0, p(bm), p(rs),
                                                       ctypes.byref(job)),
        "bh_verify_compact": lambda: L.bh_verify_compact(C, ctypes.byref(cb), n, 0, p(bm), p(rs)),
        "bh_verify_compact_submit": lambda: L.bh_verify_compact_submit(
            C, ctypes.byref(cb), n, 0, p(bm), p(rs), ctypes.byref(job)),
        "bh_batch_verify": lambda: L.bh_batch_verify(C, ctypes.byref(b), n, 0, p(bm), p(rs)),
        "bh_batch_verify_submit": lambda: L.bh_batch_verify_submit(
            C, ctypes.byref(b), n, 0, p(bm), p(rs), ctypes.byref(job)),
        "bh_batch_verify_ptrs": lambda: L.bh_batch_verify_ptrs(C, ctypes.byref(pb), n, 0, p(bm), p(rs)),
        "bh_batch_verify_ptrs_submit": lambda: L.bh_batch_verify_ptrs_submit(
            C, ctypes.byref(pb), n, 0, p(bm), p(rs), ctypes.byref(job)),
        "bh_keys_reserve": lambda: L.bh_keys_reserve(-1, C, 16),
        "bh_keys_register": lambda: L.bh_keys_register(-1, C, p(pub), 1, None),
        "bh_keys_clear": lambda: L.bh_keys_clear(-1, C),
        "bh_keys_count": lambda: L.bh_keys_count(-1, C, ctypes.byref(cnt)),
        "bh_verify_bdls": lambda: L.bh_verify_bdls(C, ctypes.byref(bd), n, p(bm), p(rs)),
        "bh_verify_bdls_dev": lambda: L.bh_verify_bdls_dev(0, C, ctypes.byref(bd), n, p(bm), p(rs),
                                                           None, 1, None),
        "bh_bdls_preverify": lambda: L.bh_bdls_preverify(C, p(sig), p(off), p(ln), n, p(pub), 1, 0,
                                                         p(bm), None, 0, ctypes.byref(cnt)),
    }
    for name, call in calls.items():
        assert call() == -1, name                      # BH_E_INVALID
        assert "P-384" in _lib.last_error(), (name, _lib.last_error())
    # an unknown curve is still refused, by these and by bh_verify itself
    assert L.bh_verify(7, ctypes.byref(b), n, 0, p(bm), p(rs)) == -1
    assert L.bh_verify_dev(0, 7, ctypes.byref(b), n, 0, p(bm), p(rs), None, 1, None) == -1
    # the two entry points that take the curve get as far as the device check
    if L.bh_device_count() == 0:  # (no bh_init in this process)
        assert L.bh_verify(C, ctypes.byref(b), n, 0, p(bm), p(rs)) == -2   # BH_E_NOT_INIT
        assert L.bh_verify_dev(0, C, ctypes.byref(b), n, 0, p(bm), p(rs), None, 1, None) == -2


def test_python_key_forms():
    from bdls_amd.bccsp import BCCSPError, ECDSAPublicKey, batch_curve, pack_records
    k384 = ECDSAPublicKey(P384.gx, P384.gy, curve="P-384")
    k256 = ECDSAPublicKey(O.P256.gx, O.P256.gy)
    assert len(k384.raw()) == 96 and k384.raw() == bytes.fromhex(U.h48(P384.gx) + U.h48(P384.gy))
    assert len(k256.raw()) == 64 and k256.raw64() == k256.raw()
    assert ECDSAPublicKey(2**384, 1, curve="P-384").raw() == b"\0" * 96
    assert batch_curve([k384, k384]) == _lib.BH_CURVE_P384 and batch_curve([k256]) == 0
    with pytest.raises(BCCSPError):
        pack_records([k256, k384], [b"", b""], [b"", b""])
