"""CPU: index-keyed P-384 passes (In384::key_idx: keys384_prep, stage384_prep's
gather, the grouping by key index) and pack.h at key width 96, compiled for
the host by the TEST-ONLY harness tests/native_p384idx/hostsim384_idx.cpp; and
the argument checks of bh_verify384_compact / bh_batch_verify384_ptrs, which
need no device. A missing harness FAILS these tests: `make` builds it."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from oracle import ecdsa_ref as O
from tests import p384_batch_util as B
from tests import p384_util as U
from tests.conftest import ROOT

HOSTSIM384I = os.path.join(ROOT, "tests", "native", "build", "libhostsim384i.so")
SELFTEST = os.path.join(ROOT, "tests", "native", "build", "idx384_selftest")
BH_E_INVALID, BH_E_NOT_INIT = -1, -2
OFF_CURVE = bytes(95) + b"\x01"
X_GE_P = b"\xff" * 48 + bytes(48)
CRAFT_KEY = bytes(47) + b"\x02" + bytes(47) + b"\x03"   # off the curve, used by the crafted records
NLS, BK = _lib.BH_F_NO_LOW_S, _lib.BH_F_BATCH_KEYS


@pytest.fixture(scope="module")
def hi():
    assert os.path.exists(HOSTSIM384I), "tests/native/build/libhostsim384i.so is not built (make)"
    L = ctypes.CDLL(HOSTSIM384I)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.hs384i_prep_words.restype = u32
    L.hs384i_prep.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
    L.hs384i_prep.restype = None
    L.hs384i_comb_pass.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp,
                                   vp]
    L.hs384i_comb_pass.restype = u32
    L.hs384i_pack.argtypes = [vp, vp, vp, vp, vp, u32, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.hs384i_pack.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def signed():
    return U.signed_batch(U.LibCrypto(), 600, 24, seed=600, family="SHA2")


def crafted(signed):
    """The precedence cases: under an off-curve key a high S, an empty signature
    and r >= n; and the same key with an acceptable signature."""
    recs, _ = signed
    base = recs[0]
    _, r, s = O.unmarshal_ecdsa_signature(bytes.fromhex(base["sig"]))
    bad = {"qx": CRAFT_KEY[:48].hex(), "qy": CRAFT_KEY[48:].hex()}
    mk = lambda sig: dict(base, sig=sig.hex(), **bad)
    return ([mk(O.marshal_ecdsa_signature(r, U.N - s)), mk(b""),
             mk(O.marshal_ecdsa_signature(U.N + 5, s)), mk(bytes.fromhex(base["sig"]))],
            [(O.R_HIGH_S, O.R_BAD_KEY), (O.R_EMPTY_SIG, O.R_EMPTY_SIG),
             (O.R_BAD_KEY, O.R_BAD_KEY), (O.R_BAD_KEY, O.R_BAD_KEY)])


def prep(hi, keys, nk, idx, sigs, msgs, flags):
    sig, so, sl = U.pack_bytes(sigs)
    msg, mo, ml = U.pack_bytes(msgs)
    n, pw = len(sigs), hi.hs384i_prep_words()
    st, words = np.full(n, 0xEE, np.uint8), np.full(n * pw, 0xEEEEEEEE, np.uint32)
    kst = np.full(max(nk, 1), 0xEE, np.uint8)
    kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8)
    hi.hs384i_prep(kb.ctypes.data, nk, None if idx is None else idx.ctypes.data, sig.ctypes.data,
                   so.ctypes.data, sl.ctypes.data, msg.ctypes.data, mo.ctypes.data, ml.ctypes.data,
                   n, flags, st.ctypes.data, words.ctypes.data, kst.ctypes.data)
    return st, words.reshape(n, pw), kst


@pytest.mark.parametrize("flags", [0, NLS])
def test_indexed_prep_equals_expanded(hi, signed, flags):
    """keys_prep + stage384_prep over a shuffled key table with duplicate and
    unused entries against stage384_prep alone on the expanded layout: every
    status byte and every e, r, sm, qx, qy, rm, r2m word."""
    recs, want = signed
    cr, cw = crafted(signed)
    recs = U.load_golden384() + recs + cr
    want = np.concatenate([[r.get("reason_no_low_s", r["reason"]) if flags else r["reason"]
                            for r in U.load_golden384()],
                           np.where(want == O.R_HIGH_S, O.R_OK, want) if flags else want,
                           [w[1 if flags else 0] for w in cw]]).astype(np.uint8)
    first = B.key_bytes(recs[300])
    table, idx = B.key_table(recs, seed=3845, extra=(first, first, OFF_CURVE, X_GE_P))
    # half of one key's records name its duplicate entry
    dup = max(j for j, k in enumerate(table) if k == first)
    orig = min(j for j, k in enumerate(table) if k == first)
    users = np.nonzero(idx == orig)[0]
    if not len(users):   # (the shuffle put a spare entry first)
        users = np.nonzero(np.isin(idx, [j for j, k in enumerate(table) if k == first]))[0]
    idx[users[::2]] = dup
    used = set(idx.tolist())
    assert table.index(OFF_CURVE) not in used and table.index(X_GE_P) not in used
    sigs, msgs = B.fields(recs, False)
    st_i, w_i, kst = prep(hi, table, len(table), idx, sigs, msgs, flags)
    st_e, w_e, _ = prep(hi, [B.key_bytes(r) for r in recs], len(recs), None, sigs, msgs, flags)
    assert (st_i == st_e).all(), np.nonzero(st_i != st_e)[0][:8]
    assert (w_i == w_e).all(), np.nonzero((w_i != w_e).any(axis=1))[0][:8]
    # prep's own verdicts: what the record was built to get, up to the curve arithmetic
    pre = st_i & 0x7f
    passed = np.isin(want, (O.R_OK, O.R_MATH))
    assert (pre[~passed] == want[~passed]).all() and (pre[passed] == O.R_OK).all()
    assert kst[table.index(OFF_CURVE)] == O.R_BAD_KEY and kst[table.index(X_GE_P)] == O.R_BAD_KEY
    assert kst[dup] == O.R_OK and kst[orig] == O.R_OK
    n = len(recs)
    assert [int(x) for x in pre[n - 4:]] == [w[1 if flags else 0] for w in cw]


def test_index_grouping(hi, signed):
    """130 records over keys used 1, 3, 4, 5 and 117 times, some rejected in
    prep: the counts per key index and the routes against a recount, the comb
    route's verdicts against the ladder's."""
    recs, want = signed
    by_key = {}
    for r, w in zip(recs, want):
        if w in (O.R_OK, O.R_MATH, O.R_HIGH_S):
            by_key.setdefault(B.key_bytes(r), []).append((r, int(w)))
    pools = sorted(by_key.values(), key=len, reverse=True)
    uses = [1, 3, 4, 5]
    picked = [(r, w, k) for k, u in enumerate(uses) for r, w in pools[k][:u]]
    # 117 records of one key: its own (25, some of them high-S: rejected in prep), repeated
    big = max(pools[4:], key=lambda pool: sum(w == O.R_HIGH_S for _, w in pool))
    picked += [(big[i % len(big)][0], big[i % len(big)][1], 4) for i in range(117)]
    order = np.random.default_rng(130).permutation(130)
    picked = [picked[i] for i in order]
    table = [B.key_bytes(next(r for r, _, k in picked if k == j)) for j in range(5)]
    table += [table[4], X_GE_P]                      # a duplicate entry and an unused bad one
    idx = np.array([k for _, _, k in picked], np.uint32)
    idx[np.nonzero(idx == 4)[0][::3]] = 5            # a third of the big key's records use the duplicate
    w = np.array([x for _, x, _ in picked], np.uint8)
    assert (w == O.R_HIGH_S).sum() >= 3
    sigs, msgs = B.fields([r for r, _, _ in picked], False)
    sig, so, sl = U.pack_bytes(sigs)
    msg, mo, ml = U.pack_bytes(msgs)
    kb = np.frombuffer(b"".join(table) + b"\0", np.uint8)
    n, nk = 130, len(table)
    cnt, route = np.full(nk, 99, np.uint32), np.full(n, 99, np.uint8)
    reason, ladder = np.full(n, 99, np.uint8), np.full(n, 99, np.uint8)
    tables = hi.hs384i_comb_pass(kb.ctypes.data, nk, idx.ctypes.data, sig.ctypes.data,
                                 so.ctypes.data, sl.ctypes.data, msg.ctypes.data, mo.ctypes.data,
                                 ml.ctypes.data, n, 0, 4, cnt.ctypes.data, route.ctypes.data,
                                 reason.ctypes.data, ladder.ctypes.data)
    admitted = w != O.R_HIGH_S
    recount = np.bincount(idx[admitted], minlength=nk)
    assert (cnt == recount).all(), (cnt, recount)
    assert recount[6] == 0 and recount[0] == 1 and recount[1] == 3 and recount[2] == 4
    want_route = (admitted & (recount[idx] >= 4)).astype(np.uint8)
    assert (route == want_route).all()
    assert tables == int((recount >= 4).sum()) == 4   # keys 2, 3, 4 and 4's duplicate: two indices, two keys
    assert (reason == ladder).all() and (reason == w).all()
    # the inputs exercise both routes: the recount sends most records to a comb,
    # and the singles, the triple and every rejected record to the ladder
    assert want_route.sum() >= 50 and (want_route == 0).sum() >= 1 + 3 + 3


def pack96(hi, keys, sigs, msgs, threads=3):
    pb = B.Ptrs(keys, sigs, msgs)
    n = pb.n
    ok = np.zeros(n * 96 + 1, np.uint8)
    kidx, slen, mlen = (np.full(n, 0xEEEEEEEE, np.uint32) for _ in range(3))
    sb = sum(len(s) for s in sigs if s is not None)
    mb = sum(len(m) for m in msgs if m is not None)
    so, mo = np.zeros(sb + 1, np.uint8), np.zeros(mb + 1, np.uint8)
    nk = hi.hs384i_pack(pb.pub.ctypes.data, pb.sig.ctypes.data, pb.sig_len.ctypes.data,
                        pb.msg.ctypes.data, pb.msg_len.ctypes.data, n, threads, ok.ctypes.data,
                        kidx.ctypes.data, slen.ctypes.data, mlen.ctypes.data, so.ctypes.data,
                        mo.ctypes.data)
    return nk, ok, kidx, slen, mlen, so[:sb].tobytes(), mo[:mb].tobytes()


def test_packer_at_96_bytes(hi):
    """Keys that differ only in byte 95, 64 or 0 stay distinct; equal keys
    behind different pointers merge; a NULL key pointer is the all-zero point;
    NULL signature / message pointers are empty fields whatever their length says."""
    rng = np.random.default_rng(96)
    base = rng.integers(0, 256, 96, dtype=np.uint8).tobytes()

    def flip(k, at):
        b = bytearray(k)
        b[at] ^= 0x80
        return bytes(b)
    kinds = [base, flip(base, 95), flip(base, 64), flip(base, 0), None]
    keys = [kinds[i % 5] for i in range(200)]
    sigs = [None if i % 17 == 3 else bytes([i % 251]) * (60 + i % 13) for i in range(200)]
    msgs = [None if i % 19 == 4 else bytes([(3 * i) % 251]) * (i % 40) for i in range(200)]
    for threads in (1, 3):
        nk, ok, kidx, slen, mlen, sb, mb = pack96(hi, keys, sigs, msgs, threads)
        assert nk >= 5
        got = [ok[96 * j:96 * j + 96].tobytes() for j in kidx]
        assert got == [k if k is not None else bytes(96) for k in keys]
        named = {int(j) for j in kidx}
        assert len(named) == 5                       # five contents, five ids, no more
        assert all(ok[96 * j:96 * j + 96].tobytes() == bytes(96)
                   for j in range(nk) if j not in named)   # ids no record names: zero keys
        assert (slen == [len(s) if s is not None else 0 for s in sigs]).all()
        assert (mlen == [len(m) if m is not None else 0 for m in msgs]).all()
        assert sb == b"".join(s for s in sigs if s is not None)
        assert mb == b"".join(m for m in msgs if m is not None)


def _dummy(n=4):
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    idx = np.array([0, 1, 2, 1], np.uint32)
    ln = np.array([8, 8, 8, 8], np.uint32)
    ptr = np.full(n, p, np.uint64)
    cb = dict(keys=p, key_idx=idx.ctypes.data, nkeys=3, sig=p, sig_len=ln.ctypes.data, msg=p,
              msg_len=ln.ctypes.data, msg_stride=0)
    pb = dict(pub=ptr.ctypes.data, sig=ptr.ctypes.data, sig_len=ln.ctypes.data,
              msg=ptr.ctypes.data, msg_len=ln.ctypes.data)
    return (buf, idx, ln, ptr), p, cb, pb


def _calls(L, p, cb, pb, n=4, flags=0):
    """The four entry points on one set of arguments -> their return codes."""
    c, q, job = _lib.BhCBatch(**cb), _lib.BhPBatch(**pb), ctypes.c_void_p(1)
    out = [L.bh_verify384_compact(ctypes.byref(c), n, flags, p, p),
           L.bh_verify384_compact_submit(ctypes.byref(c), n, flags, p, p, ctypes.byref(job))]
    assert job.value is None
    job = ctypes.c_void_p(1)
    out += [L.bh_batch_verify384_ptrs(ctypes.byref(q), n, flags, p, p),
            L.bh_batch_verify384_ptrs_submit(ctypes.byref(q), n, flags, p, p, ctypes.byref(job))]
    assert job.value is None
    return out


def test_argument_checks_need_no_device():
    """Key index >= nkeys, null required fields, the refused hash flags (named
    in bh_last_error), a null job: BH_E_INVALID, before any device is asked for."""
    L = _lib.lib()
    keep, p, cb, pb = _dummy()
    c = _lib.BhCBatch(**dict(cb, nkeys=2))           # index 2 >= nkeys
    assert L.bh_verify384_compact(ctypes.byref(c), 4, 0, p, p) == BH_E_INVALID
    assert "key index" in _lib.last_error()
    job = ctypes.c_void_p()
    assert L.bh_verify384_compact_submit(ctypes.byref(c), 4, 0, p, p,
                                         ctypes.byref(job)) == BH_E_INVALID
    for f in ("keys", "sig_len", "sig", "msg"):
        c = _lib.BhCBatch(**dict(cb, **{f: None}))
        assert L.bh_verify384_compact(ctypes.byref(c), 4, 0, p, p) == BH_E_INVALID, f
        assert "null" in _lib.last_error()
    for f in ("pub", "sig", "sig_len", "msg", "msg_len"):
        q = _lib.BhPBatch(**dict(pb, **{f: None}))
        assert L.bh_batch_verify384_ptrs(ctypes.byref(q), 4, 0, p, p) == BH_E_INVALID, f
        assert "null" in _lib.last_error()
    c, q = _lib.BhCBatch(**cb), _lib.BhPBatch(**pb)
    for bm, rs in ((None, p), (p, None)):
        assert L.bh_verify384_compact(ctypes.byref(c), 4, 0, bm, rs) == BH_E_INVALID
        assert L.bh_batch_verify384_ptrs(ctypes.byref(q), 4, 0, bm, rs) == BH_E_INVALID
    assert L.bh_verify384_compact(None, 4, 0, p, p) == BH_E_INVALID
    assert L.bh_batch_verify384_ptrs(None, 4, 0, p, p) == BH_E_INVALID
    assert L.bh_verify384_compact_submit(ctypes.byref(c), 4, 0, p, p, None) == BH_E_INVALID
    assert L.bh_batch_verify384_ptrs_submit(ctypes.byref(q), 4, 0, p, p, None) == BH_E_INVALID
    for flag, name in ((_lib.BH_F_HASH_SHA384, "BH_F_HASH_SHA384"),
                       (_lib.BH_F_HASH_SHA512, "BH_F_HASH_SHA512")):
        for k in range(4):
            assert _calls(L, p, cb, pb, flags=flag)[k] == BH_E_INVALID
            e = _lib.last_error()
            assert name in e and "bh_verify" in e and "384" in e.replace(name, "")
    assert _calls(L, p, cb, pb, flags=0x100) == [BH_E_INVALID] * 4
    assert _calls(L, p, cb, pb, flags=1 | 8) == [BH_E_INVALID] * 4
    assert _calls(L, p, cb, pb, n=1 << 32) == [BH_E_INVALID] * 4
    assert "too large" in _lib.last_error()
    del keep


def test_not_init_in_a_fresh_process():
    """Before bh_init every accepted flag combination answers BH_E_NOT_INIT
    (argument checks come first: a bad index is still BH_E_INVALID), n = 0 too."""
    code = (
        "import ctypes, json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "from tests.test_p384_batch_cpu import _dummy, _calls\n"
        "L = _lib.lib()\n"
        "keep, p, cb, pb = _dummy()\n"
        "out = [_calls(L, p, cb, pb, flags=f) for f in (0, 1, 8, 2 | 128, 4 | 16 | 1)]\n"
        "out.append(_calls(L, p, cb, pb, n=0))\n"
        "out.append(_calls(L, p, dict(cb, nkeys=1), pb)[:2])\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == [[BH_E_NOT_INIT] * 4] * 6 + [[BH_E_INVALID] * 2]


def test_bindings_and_header():
    hdr = open(os.path.join(ROOT, "include", "bdls_hip.h")).read()
    for name in ("bh_verify384_compact", "bh_verify384_compact_submit", "bh_batch_verify384_ptrs",
                 "bh_batch_verify384_ptrs_submit"):
        assert f"int {name}(" in hdr and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).argtypes
    from bdls_amd.bccsp import verify_packed384
    assert callable(verify_packed384)


def test_sanitizer_selftest_program():
    """The stand-alone program (address + undefined-behaviour sanitizers, its
    own main) builds, runs the indexed prep and grouping on 130 records and exits 0."""
    b = subprocess.run(["make", "-C", ROOT, os.path.relpath(SELFTEST, ROOT)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([SELFTEST], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "130 records" in r.stdout and "ok" in r.stdout
