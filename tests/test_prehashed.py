"""BDLS records whose SignedProto.Hash() the caller supplies
(bh_verify_bdls_prehashed_dev): the crafted list of tests/prehashed_cases.py
through the host build of the device's stage functions, every route the
harness restates, against the oracle; the digest -> e rule on its own; and the
list's expectations against a second, independent reference (OpenSSL)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ecdsa_ref as O
from tests import prehashed_cases as PC

CURVES = ["secp256k1", "P-256"]


@pytest.fixture(scope="module")
def hs():
    if not os.path.exists(PC.HOSTSIM):
        pytest.skip("hostsim not built")
    L = ctypes.CDLL(PC.HOSTSIM)
    vp = ctypes.c_void_p
    L.hs_verify_bdls_prehashed.argtypes = [ctypes.c_int] + [vp] * 11 + [ctypes.c_uint32] * 2 + [vp]
    L.hs_bdls_given_e.argtypes = [ctypes.c_int, vp, ctypes.c_uint32, vp]
    L.hs_bdls_given_e.restype = None
    return L


@pytest.fixture(scope="module")
def crafted(hs):
    """{curve: (records, packed arrays)}, built once."""
    out = {}
    for curve in CURVES:
        recs = PC.build(curve)
        out[curve] = (recs, PC.pack(recs))
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_crafted_expectations_vs_openssl(crafted, curve):
    """go_ecdsa_verify's reasons against oracle/orc.c (OpenSSL) on every record
    whose r and s its 32-byte interface can carry."""
    from oracle import orc
    for tag, x, y, rb, sb, dg, reason in crafted[curve][0]:
        r, s = int.from_bytes(rb, "big"), int.from_bytes(sb, "big")
        if r >= 2**256 or s >= 2**256:  # past any order: a range or, on P-256, a key reject
            assert reason in (O.R_R_RANGE, O.R_S_RANGE, O.R_BAD_KEY), tag
            continue
        assert orc.go_verify(x + y, dg, r, s, curve=PC.CURVE_ID[curve]) == reason, tag


@pytest.mark.parametrize("curve", CURVES)
def test_crafted_list_is_stable(crafted, curve):
    """The list is a function of the generators' seeds alone (GPU cases and
    CPU cases see the same records), and small enough for the wide routes."""
    recs = crafted[curve][0]
    assert PC.build(curve) == recs
    assert 200 <= len(recs) <= 2048
    print(curve, dict(sorted(PC.class_counts(recs).items())))


# (wide, ll, reg) as the harness's run_seq tells them apart: comb tables
# (ll) exist for the one-lane route only, and a registry slot (reg) is built
# the same way whatever ll says
ROUTES = [(1, 0, 0), (1, 1, 0), (1, 0, 1), (4, 0, 0), (4, 0, 1), (16, 0, 0), (16, 0, 1)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("min_uses", [1, 1000])
@pytest.mark.parametrize("wide,ll,reg", ROUTES)
def test_crafted_hostsim(hs, crafted, curve, min_uses, wide, ll, reg):
    """min_uses 1: every key gets a table (windowed, comb or registry slot);
    1000: every record takes the ladder (secp256k1 at wide > 1: the two-lane
    GLV ladder)."""
    recs, arrs = crafted[curve]
    out = np.full(len(recs), 255, np.uint8)
    hs.hs_set_wide(wide)
    hs.hs_set_ll(ll)
    hs.hs_set_reg(reg)
    try:
        hs.hs_verify_bdls_prehashed(PC.CURVE_ID[curve], *[a.ctypes.data for a in arrs], len(recs),
                                    min_uses, out.ctypes.data)
    finally:
        hs.hs_set_wide(1)
        hs.hs_set_ll(0)
        hs.hs_set_reg(0)
    bad = [(t[0], int(o), t[6]) for t, o in zip(recs, out) if o != t[6]]
    assert not bad


@pytest.mark.parametrize("curve", CURVES)
def test_digest_to_e(hs, curve):
    """stage_bdls_given: e = the left-most min(len, 32) bytes, big-endian, minus
    n once when >= n; the digest at every byte alignment."""
    n = PC.CURVES[curve].n
    assert 2**255 < n < 2**256  # one subtraction reduces any 256-bit value
    tail = bytes(range(0xA0, 0xC0))
    buf = np.zeros(128, np.uint8)
    base = (-buf.ctypes.data) % 4  # buf[base] is 4-byte aligned
    e = np.zeros(8, np.uint32)
    for v in (0, n - 1, n, n + 1, 2**256 - 1, 0x0102030405060708090A0B0C0D0E0F10 << 128 | 0xF1):
        for ln in (0, 1, 31, 32, 33, 64):
            dg = (v.to_bytes(32, "big") + tail)[:ln]
            want = int.from_bytes(dg[:32], "big")
            if want >= n:
                want -= n
            for al in range(4):
                buf[:] = 0xEE
                buf[base + al:base + al + ln] = np.frombuffer(dg, np.uint8)
                e[:] = 0xFFFFFFFF
                hs.hs_bdls_given_e(PC.CURVE_ID[curve], buf.ctypes.data + base + al, ln,
                                   e.ctypes.data)
                got = sum(int(x) << (32 * k) for k, x in enumerate(e))
                assert got == want, (hex(v), ln, al, hex(got), hex(want))


def test_prehashed_parity_with_hashing_hostsim(hs):
    """The committed digests of the BDLS golden set through the prehashed
    harness entry give the reasons the hashing path's golden file records."""
    import json
    with open(os.path.join(PC.ROOT, "tests", "golden", "bdls_vectors.jsonl")) as f:
        gold = [json.loads(l) for l in f]
    from tests.bdls_util import pack_bdls
    for curve in CURVES:
        recs = [dict(r, msg=r["digest"]) for r in gold if r["curve"] == curve]
        out = np.full(len(recs), 255, np.uint8)
        arrs = pack_bdls(recs)
        hs.hs_verify_bdls_prehashed(PC.CURVE_ID[curve], *[a.ctypes.data for a in arrs],
                                    len(recs), 1, out.ctypes.data)
        assert [int(o) for o in out] == [r["reason"] for r in recs]


def test_p384_refused_by_name():
    """BH_CURVE_P384 is refused by name, before any device is looked for, like
    the other BDLS entry points (tests/test_p384_cpu.py
    test_unsupported_entry_points_name_the_curve holds their table)."""
    from bdls_amd import _lib
    L = _lib.lib()
    buf = np.zeros(96, np.uint8)
    p = buf.ctypes.data
    bd = _lib.BhBdlsBatch(*([p] * 11))
    assert L.bh_verify_bdls_prehashed_dev(0, _lib.BH_CURVE_P384, ctypes.byref(bd), 1, p, p, None,
                                          1, None) == -1  # BH_E_INVALID
    assert "P-384" in _lib.last_error(), _lib.last_error()
    # an unknown curve and an unknown public flag are still refused
    assert L.bh_verify_bdls_prehashed_dev(0, 7, ctypes.byref(bd), 1, p, p, None, 1, None) == -1
    b = _lib.BhBatch(*([p] * 7))
    assert L.bh_verify(0, ctypes.byref(b), 1, 0x100, p, p) == -1
    assert "flag" in _lib.last_error()
