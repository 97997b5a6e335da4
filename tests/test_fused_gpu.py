"""GPU: the fused point formulas (ec30.h: one reduction for the additions' Y3,
the composite 2 A + T through the co-Z addition without the partner update) on
the three routes that run them, bit for bit against construction and the C oracle:

  * the one-lane folded comb (k_ktab_ladder + k_keycomb, verify.h q_llcomb_g) at
    40,960 records, the smallest batch the fixtures send there: every key used
    >= 4 times, the crafted comb scalars and the folded Horner's degenerate
    branches (tests/comb_cases.py) among generator records with 1/16 corrupted,
    through bh_verify_dev on the caller's stream and with BH_F_ANY_LANE;
  * the one-lane ladder with its folded G additions (q_ladder_odd_g) on a
    distinct-key batch of the same size with the crafted last-window events;
  * the small-batch route (k_small and the wide kernels) at 2,000 records.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from bdls_amd import _lib, workload
from oracle import ecdsa_ref as O
from oracle import orc
from tests.comb_cases import (distinct_key_classes, fold_crafted, ladder_crafted,
                              records_for_fold, records_for_u2, signed_comb_u2)

pytestmark = pytest.mark.gpu

N = 40_960


@pytest.fixture(scope="module")
def L():
    _lib.ensure_init()
    return _lib.lib()


def _pack(recs):
    """[(pub64, sig, digest)] -> bh_batch arrays (digest mode)."""
    pub = np.frombuffer(b"".join(r[0] for r in recs), np.uint8)
    sl = np.array([len(r[1]) for r in recs], np.uint32)
    dl = np.array([len(r[2]) for r in recs], np.uint32)
    so = np.zeros(len(recs), np.uint64)
    do = np.zeros(len(recs), np.uint64)
    so[1:] = np.cumsum(sl[:-1])
    do[1:] = np.cumsum(dl[:-1])
    sig = np.frombuffer(b"".join(r[1] for r in recs) + b"\0", np.uint8)
    dg = np.frombuffer(b"".join(r[2] for r in recs) + b"\0", np.uint8)
    return pub, sig, so, sl, dg, do, dl


def _dev_verify(L, arrs, n, flags=0):
    """One bh_verify_dev pass; with BH_F_ANY_LANE on the library's streams
    (no timing record, bh_sync before the outputs are read)."""
    DA = _lib.DeviceArray
    d = [DA.from_numpy(0, x) for x in arrs]
    words = DA(0, ((n + 63) // 64) * 8)
    reason = DA(0, n)
    b = _lib.BhBatch(*[x.ptr for x in d])
    tm = None
    if flags & _lib.BH_F_ANY_LANE:
        _lib.check(L.bh_verify_dev(0, 0, ctypes.byref(b), n, flags, words.ptr, reason.ptr, None,
                                   0, None))
        _lib.check(L.bh_sync(0))
    else:
        tm = _lib.BhTiming()
        _lib.check(L.bh_verify_dev(0, 0, ctypes.byref(b), n, flags, words.ptr, reason.ptr, None,
                                   1, ctypes.byref(tm)))
    bits = np.unpackbits(words.to_numpy(np.uint64, (n + 63) // 64).view(np.uint8),
                         bitorder="little")[:n].astype(bool)
    out = bits, reason.to_numpy(np.uint8, n), tm
    for x in d + [words, reason]:
        x.free()
    return out


def _filler(recs, want, fill, nkeys, seed):
    """generator records in digest mode (1/16 corrupted) appended to recs / want"""
    w = workload.generate(fill, nkeys, 64, 16, seed=seed)
    for i in range(w.n):
        m = bytes(w.msg[w.msg_off[i]:w.msg_off[i] + w.msg_len[i]])
        recs.append((bytes(w.pub[64 * i:64 * i + 64]),
                     bytes(w.sig[w.sig_off[i]:w.sig_off[i] + w.sig_len[i]]),
                     hashlib.sha256(m).digest()))
    want += [int(x) for x in w.reason]
    return w.n


def _orc_sample(recs, want, lo, n, seed):
    for i in np.random.default_rng(seed).choice(n, 100, replace=False):
        q, s, dg = recs[lo + i]
        assert orc.csp_verify(q, s, dg) == want[lo + i], int(lo + i)


@pytest.fixture(scope="module")
def comb_batch():
    """(arrays, expected reasons): crafted comb scalars and folded-Horner events,
    each key 4 times, scattered into generator records on keys used ~64 times."""
    c = O.P256
    crafted, cwant = [], []
    for k, (qx, qy, sig, dg) in enumerate(records_for_u2(c, signed_comb_u2(c.n, 7, 37), seed=71,
                                                         low_s=True)):
        crafted.append((qx.to_bytes(32, "big") + qy.to_bytes(32, "big"), sig, dg))
        cwant.append(0 if k % 2 == 0 else 9)  # a valid signature, then its flipped-digest twin
    kgf = int(os.environ.get("BH_GFOLD", 3))  # the library's G group size (verify.h kGF)
    fold = records_for_fold(c, fold_crafted(c, 7, 37, seed=35, low_s=True, kgf=kgf), low_s=True)
    assert len(fold) >= 13
    for qx, qy, sig, dg, exp in fold:
        crafted.append((qx.to_bytes(32, "big") + qy.to_bytes(32, "big"), sig, dg))
        cwant.append(exp)
    assert all(orc.csp_verify(*r) == w for r, w in zip(crafted, cwant))
    recs, want = [], []
    fill = N - 4 * len(crafted)
    _filler(recs, want, fill, fill // 64, seed=53)
    _orc_sample(recs, want, 0, fill, 7)
    # the crafted records, 4 uses of each key, mixed into the random ones
    pos = sorted(np.random.default_rng(9).choice(fill, 4 * len(crafted), replace=False))
    for j, at in enumerate(pos):
        recs.insert(int(at) + j, crafted[j // 4])
        want.insert(int(at) + j, cwant[j // 4])
    assert len(recs) == N
    return _pack(recs), np.array(want, np.uint8)


@pytest.mark.parametrize("any_lane", [0, 1])
def test_folded_comb_40960(L, comb_batch, any_lane):
    arrs, want = comb_batch
    bits, reason, tm = _dev_verify(L, arrs, N, _lib.BH_F_ANY_LANE if any_lane else 0)
    bad = np.nonzero(reason != want)[0]
    assert not len(bad), [(int(i), int(reason[i]), int(want[i])) for i in bad[:10]]
    assert (bits == (want == 0)).all()
    if tm is not None:  # one lane per record, every group equation through the key tables
        assert tm.wide == 1 and tm.n_ladder == 0
        assert tm.n_keycomb == int(((want == 0) | (want == 9)).sum())


def test_ladder_distinct_keys_40960(L):
    c = O.P256
    kgf = int(os.environ.get("BH_GFOLD", 3))
    recs, want = [], []
    for seed in (46, 47):
        for qx, qy, sig, dg, exp in records_for_fold(c, ladder_crafted(c, seed=seed, low_s=True,
                                                                       kgf=kgf), low_s=True):
            recs.append((qx.to_bytes(32, "big") + qy.to_bytes(32, "big"), sig, dg))
            want.append(exp)
    for qx, qy, sig, dg, exp, _tag in distinct_key_classes(c, seed=62, reps=2):
        recs.append((qx.to_bytes(32, "big") + qy.to_bytes(32, "big"), sig, dg))
        want.append(exp)
    assert all(orc.csp_verify(*r) == w for r, w in zip(recs, want))
    base = len(recs)
    fill = N - base
    _filler(recs, want, fill, fill, seed=54)  # a distinct key each
    _orc_sample(recs, want, base, fill, 8)
    want = np.array(want, np.uint8)
    bits, reason, tm = _dev_verify(L, _pack(recs), N)
    bad = np.nonzero(reason != want)[0]
    assert not len(bad), [(int(i), int(reason[i]), int(want[i])) for i in bad[:10]]
    assert (bits == (want == 0)).all()
    assert tm.wide == 1 and tm.n_keycomb == 0 and tm.n_keytables == 0
    assert tm.n_ladder == int(((want == 0) | (want == 9)).sum())


def test_small_batch_2000(L):
    n = 2000
    w = workload.generate(n, 40, 64, 16, seed=55)
    bits, reason, tm = _dev_verify(L, w.arrays(), n, _lib.BH_F_HASH_SHA256)
    assert (reason == w.reason).all() and (bits == w.expected_valid).all()
    for i in np.random.default_rng(6).choice(n, 100, replace=False):
        q = bytes(w.pub[64 * i:64 * i + 64])
        s = bytes(w.sig[w.sig_off[i]:w.sig_off[i] + w.sig_len[i]])
        dg = hashlib.sha256(bytes(w.msg[w.msg_off[i]:w.msg_off[i] + w.msg_len[i]])).digest()
        assert orc.csp_verify(q, s, dg) == w.reason[i], int(i)
