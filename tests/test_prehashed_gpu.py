"""GPU: crafted curve edge cases through the kernels production BDLS batches
run, by way of bh_verify_bdls_prehashed_dev (the caller supplies
SignedProto.Hash(), so e, u1 and u2 are the test's to choose).

The records are tests/prehashed_cases.py's (x wrap, u1 G + u2 Q = infinity,
u1 G == u2 Q, GLV split edges, comb / window / G-comb edge scalars, Q = +-G and
2 G, digest and r / s encodings, bad keys), the expected reasons the oracle's
(oracle.ecdsa_ref.go_ecdsa_verify; cross-checked against OpenSSL in
tests/test_prehashed.py). Batches are that list repeated, at the smallest
sizes that select each kernel set:

  a  the list once (< 8,192)   k_ladder2_q/_g (secp256k1), k_ladder1_q (P-256)
  b  the same, keys registered k_reg_win slots through k_keycomb_wide_q/_g<16>
  c  8,192                     per-batch windowed tables, 16 lanes
  d  8,256                     k_keycomb_wide_q/_g<4>; BH_ROUTE=ladder: the split
                               ladder with the two-slot Q tables
  e  32,832                    one lane: comb (BH_LL=1) / windowed (BH_LL=0)
                               tables, k_ktab_ladder's ladder (BH_ROUTE=ladder)
  f  32,832, keys registered   one lane over registry combs
  g  the golden BDLS set: committed digests through this entry point against
     the hashing entry point in the same process

Every case asserts the reasons record by record, the bitmap, and the route
taken (bh_timing: wide, n_ladder, n_keycomb, n_keytables)."""
import ctypes
import json
import os

import numpy as np
import pytest

from bdls_amd import _lib
from tests import prehashed_cases as PC
from tests.bdls_util import pack_bdls

pytestmark = pytest.mark.gpu
CURVES = ["secp256k1", "P-256"]


@pytest.fixture
def L():
    """The library with an empty key registry before and after."""
    _lib.ensure_init()
    lib = _lib.lib()
    for c in (0, 1):
        _lib.check(lib.bh_keys_clear(-1, c))
    yield lib
    for c in (0, 1):
        _lib.check(lib.bh_keys_clear(-1, c))


@pytest.fixture(scope="module")
def crafted():
    return {curve: PC.build(curve) for curve in CURVES}


def _batch(recs, n):
    """The list repeated and cut to n records: (records, arrays, expected reasons)."""
    reps = (recs * (-(-n // len(recs))))[:n]
    return reps, PC.pack(reps), np.array([r[6] for r in reps], np.uint8)


def _route_facts(curve, reps):
    """(records reaching the group equation, their distinct keys)."""
    math = [r for r in reps if PC.reaches_group_equation(curve, r)]
    return len(math), len({r[1] + r[2] for r in math})


def _run(L, curve, arrs, n, entry="bh_verify_bdls_prehashed_dev", env=None):
    DA = _lib.DeviceArray
    d = [DA.from_numpy(0, x) for x in arrs]
    words = DA(0, ((n + 63) // 64) * 8)
    reason = DA(0, n)
    tm = _lib.BhTiming()
    b = _lib.BhBdlsBatch(*[x.ptr for x in d])
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        _lib.check(getattr(L, entry)(0, PC.CURVE_ID[curve], ctypes.byref(b), n, words.ptr,
                                     reason.ptr, None, 1, ctypes.byref(tm)))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    bits = np.unpackbits(words.to_numpy(np.uint64, (n + 63) // 64).view(np.uint8),
                         bitorder="little")[:n].astype(bool)
    got = reason.to_numpy(np.uint8, n)
    for x in d + [words, reason]:
        x.free()
    print(f"{curve} n={n} env={env}: wide={tm.wide} n_ladder={tm.n_ladder} "
          f"n_keycomb={tm.n_keycomb} n_keytables={tm.n_keytables}")
    return got, bits, tm


def _check(reps, got, bits, want):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), reps[i][0], int(got[i]), int(want[i])) for i in bad[:12]]
    assert (bits == (want == 0)).all()


def _register(L, curve, recs):
    keys = sorted({r[1] + r[2] for r in recs})
    pubs = np.frombuffer(b"".join(keys), np.uint8)
    st = np.full(len(keys), 77, np.uint8)
    _lib.check(L.bh_keys_register(-1, PC.CURVE_ID[curve], pubs.ctypes.data, len(keys),
                                  st.ctypes.data))
    c = PC.CURVES[curve]
    for k, s in zip(keys, st):  # a key registers iff it is a curve point
        x, y = int.from_bytes(k[:32], "big"), int.from_bytes(k[32:], "big")
        assert (s == 0) == (x < c.p and y < c.p and PC.O.on_curve(c, x, y)), k.hex()


@pytest.mark.parametrize("curve", CURVES)
def test_a_split_ladders(L, crafted, curve):
    recs = crafted[curve]
    n = len(recs)
    assert n < 8192
    reps, arrs, want = _batch(recs, n)
    got, bits, tm = _run(L, curve, arrs, n)
    _check(reps, got, bits, want)
    math, _ = _route_facts(curve, reps)
    # below kKeyTableMinBatch: no tables, every record on the split ladder
    assert tm.wide == 16 and tm.n_keycomb == 0 and tm.n_keytables == 0
    assert tm.n_ladder == math


@pytest.mark.parametrize("curve", CURVES)
def test_b_registry_slots_16_lanes(L, crafted, curve):
    recs = crafted[curve]
    n = len(recs)
    assert n < 8192
    reps, arrs, want = _batch(recs, n)
    _register(L, curve, recs)
    got, bits, tm = _run(L, curve, arrs, n)
    _check(reps, got, bits, want)
    math, _ = _route_facts(curve, reps)
    assert tm.wide == 16 and tm.n_ladder == 0 and tm.n_keytables == 0
    assert tm.n_keycomb == math


@pytest.mark.parametrize("curve", CURVES)
def test_c_batch_tables_16_lanes(L, crafted, curve):
    n = 8192
    reps, arrs, want = _batch(crafted[curve], n)
    assert n // len(crafted[curve]) >= 4  # every key reaches kMinUses
    got, bits, tm = _run(L, curve, arrs, n)
    _check(reps, got, bits, want)
    math, keys = _route_facts(curve, reps)
    assert tm.wide == 16 and tm.n_keytables == keys and tm.n_keytables > 0
    assert tm.n_keycomb == math and tm.n_ladder == 0


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ["default", "ladder"])
def test_d_4_lanes(L, crafted, curve, route):
    n = 8256
    assert 8192 < n <= 32768
    reps, arrs, want = _batch(crafted[curve], n)
    got, bits, tm = _run(L, curve, arrs, n, env={"BH_ROUTE": "ladder"} if route == "ladder" else None)
    _check(reps, got, bits, want)
    math, keys = _route_facts(curve, reps)
    assert tm.wide == 4
    if route == "ladder":
        assert tm.n_ladder == math and tm.n_keycomb == 0 and tm.n_keytables == 0
    else:
        assert tm.n_keytables == keys and tm.n_keytables > 0
        assert tm.n_keycomb == math and tm.n_ladder == 0


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("env", [{"BH_LL": "1"}, {"BH_LL": "0"}, {"BH_ROUTE": "ladder"}],
                         ids=["ll1", "ll0", "ladder"])
def test_e_one_lane(L, crafted, curve, env):
    n = 32_832
    assert n > 32768
    reps, arrs, want = _batch(crafted[curve], n)
    got, bits, tm = _run(L, curve, arrs, n, env=env)
    _check(reps, got, bits, want)
    math, keys = _route_facts(curve, reps)
    assert tm.wide == 1
    if "BH_ROUTE" in env:
        assert tm.n_ladder == math and tm.n_keycomb == 0 and tm.n_keytables == 0
    else:
        assert tm.n_keytables == keys and tm.n_keytables > 0
        assert tm.n_keycomb == math and tm.n_ladder == 0


@pytest.mark.parametrize("curve", CURVES)
def test_f_one_lane_registry(L, crafted, curve):
    n = 32_832
    assert n > 32768
    reps, arrs, want = _batch(crafted[curve], n)
    _register(L, curve, crafted[curve])
    got, bits, tm = _run(L, curve, arrs, n)
    _check(reps, got, bits, want)
    math, _ = _route_facts(curve, reps)
    assert tm.wide == 1 and tm.n_ladder == 0 and tm.n_keytables == 0
    assert tm.n_keycomb == math


@pytest.mark.parametrize("curve", CURVES)
def test_g_parity_with_hashing_entry(L, curve):
    with open(os.path.join(PC.ROOT, "tests", "golden", "bdls_vectors.jsonl")) as f:
        gold = [r for r in map(json.loads, f) if r["curve"] == curve]
    n = len(gold)
    hashed, hbits, _ = _run(L, curve, pack_bdls(gold), n, entry="bh_verify_bdls_dev")
    pre, pbits, _ = _run(L, curve, pack_bdls([dict(r, msg=r["digest"]) for r in gold]), n)
    assert (pre == hashed).all() and (pbits == hbits).all()
    assert [int(x) for x in hashed] == [r["reason"] for r in gold]
