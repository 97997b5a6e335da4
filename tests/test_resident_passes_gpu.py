"""GPU: the host code that strings the kernels together for a device-resident
batch above one pass (bdls_hip.cpp run_dev384, run_dev_wide, run_dev's pass
loop) and the deferred stage timing bench.py relies on (bh_timing_begin /
bh_timing_end).

Expected values never come from the library: the fixture
tests/golden/p384_vectors.jsonl holds the oracle's, and the by-construction
batches (tests/resident_util.py) are put to oracle/ecdsa_ref.py on every
corrupted record and every 16th other one. Every bh_verify_dev call writes into
guarded outputs: one bitmap word and 64 reason bytes more than it may touch.

BH_P384_CHUNK is parsed once per process, so the P-384 and wide-hash passes of
64 run in two child processes (one per fixture below, each under its own
timeout); BH_MAX_CHUNK is read per call and is set around the call.
"""
import ctypes
import os

import pytest

from bdls_amd import _lib, workload
from tests import resident_util as R
from tests import sha2wide_util as W

pytestmark = pytest.mark.gpu
STAGES = _lib.BhTiming.STAGES


@pytest.fixture(scope="module")
def L():
    _lib.ensure_init()
    return _lib.lib()


@pytest.fixture(scope="module")
def p384_child(tmp_path_factory):
    """Section 1 in one child with BH_P384_CHUNK=64: (results, expectations)."""
    batches, ops, expect = R.plan_p384()
    return R.run_child(batches, ops, tmp_path_factory.mktemp("p384")), expect


@pytest.fixture(scope="module")
def wide_child(tmp_path_factory):
    """Section 2 in a second child with BH_P384_CHUNK=64."""
    batches, ops, expect = R.plan_wide()
    return R.run_child(batches, ops, tmp_path_factory.mktemp("wide")), expect


def check_ops(child, prefix):
    res, expect = child
    ids = [i for i in expect if i.startswith(prefix)]
    assert ids
    for op_id in ids:
        n, want, _ = expect[op_id]
        R.check_result(res[op_id], n, want, op_id)
        # one batch per call of the C ABI, however many passes it took
        assert res[op_id]["stats"] == [1, n], op_id
    return ids


# ---------------------------------------------------------------- 1. resident P-384
def test_p384_digest_mode_prefixes(p384_child):
    """The fixture in digest mode at n = 1, 64, 65, 128, 129 and whole (1 to 4
    passes of 64), with and without the low-S rule, with and without a
    bh_timing: reasons, bits [0, n) and both guards."""
    ids = check_ops(p384_child, "digest/")
    assert len(ids) == 24


def test_p384_fused_hash_passes(p384_child):
    """200 libcrypto-signed records hashed on the device (SHA-256, SHA3-256) in
    passes of 64, 64, 64 and 8: each pass reads its own slice of msg_off / msg_len."""
    assert len(check_ops(p384_child, "fused/")) == 4


def test_p384_timing_sums_over_passes(p384_child):
    """A call with a bh_timing gives the results of the call without one;
    n_ladder is the sum over the passes (n, not the last pass's count), nothing
    takes a key table, and the three stages P-384 fills are positive."""
    res, expect = p384_child
    timed = [i for i, (_, _, t) in expect.items() if t]
    assert len(timed) == 14
    for op_id in timed:
        n = expect[op_id][0]
        plain = res[op_id[:-1] + "0"]
        assert res[op_id]["reason"] == plain["reason"] and res[op_id]["words"] == plain["words"]
        assert plain["timing"] is None
        t = res[op_id]["timing"]
        assert t["n_ladder"] == n, (op_id, t)
        assert t["n_keycomb"] == 0 and t["n_keytables"] == 0 and t["wide"] == 0, (op_id, t)
        assert t["prep_ms"] > 0 and t["inv_ms"] > 0 and t["build_ladder_ms"] > 0, (op_id, t)
        assert t["plan_ms"] == 0 and t["publish_ms"] == 0 and t["keycomb_ms"] == 0, (op_id, t)


def test_p384_two_calls_in_flight(p384_child):
    """Two calls with sync = 0 and no timing, the fixture and the fixture
    reversed, each with its own outputs, then one bh_sync: the second call
    re-carves the one P-384 workspace behind the first, and both are right."""
    assert len(check_ops(p384_child, "async/")) == 2


# ---------------------------------------------------------------- 2. wide hashes, passes of 64
def test_wide_hash_p384_resident_passes(wide_child):
    """P-384 with SHA-384 and with SHA-512, 200 records: four digest passes
    rewrite the one digest buffer, each followed by its curve pass; with the
    low-S rule and with BH_F_NO_LOW_S | BH_F_KEEP_KEYS | BH_F_ANY_LANE (the last
    two ignored), with and without a bh_timing."""
    res, expect = wide_child
    ids = check_ops(wide_child, "wide/")
    assert len(ids) == 8
    for op_id in ids:
        n, _, timed = expect[op_id]
        t = res[op_id]["timing"]
        if not timed:
            assert t is None
            continue
        assert t["n_ladder"] == n and t["n_keycomb"] == 0 and t["n_keytables"] == 0, (op_id, t)
        assert t["prep_ms"] > 0 and t["inv_ms"] > 0 and t["build_ladder_ms"] > 0, (op_id, t)
        plain = res[op_id[:-1] + "0"]
        assert res[op_id]["reason"] == plain["reason"] and res[op_id]["words"] == plain["words"]


def test_wide_hash_p256_host_chunks(wide_child):
    """bh_verify of 200 P-256 + SHA-512 records in four uploads of 64, each
    with its own digest pass and key tables: reasons, bitmap, one batch."""
    assert check_ops(wide_child, "host/") == ["host/P256/SHA512"]


# ---------------------------------------------------------------- 3. P-256 and a wide hash, forced
@pytest.fixture
def chunk_env():
    """Sets BH_MAX_CHUNK (read per call) and always restores it."""
    old = os.environ.get("BH_MAX_CHUNK")

    def set_chunk(v):
        if v is None:
            os.environ.pop("BH_MAX_CHUNK", None)
        else:
            os.environ["BH_MAX_CHUNK"] = str(v)
    yield set_chunk
    set_chunk(old)


@pytest.mark.parametrize("h", ["SHA384", "SHA512"])
def test_p256_wide_hash_forced_passes(L, chunk_env, h):
    """257 P-256 records with a wide hash and BH_MAX_CHUNK=128: one digest pass,
    then three curve passes (128, 128, 1) slicing the library's own digest
    offsets and lengths. The counts of a bh_timing are sums over the passes."""
    n = 257
    recs, want, nls = R.wide_batch("P-256", h, n)
    flag = W.HASHES[h][1]
    res = R.Resident(R.pack(recs, "msg"))
    try:
        chunk_env(128)
        plain = R.dev_call(res, W.BH_CURVE_P256, n, flag)
        timed = R.dev_call(res, W.BH_CURVE_P256, n, flag, timing=True)
        no_rule = R.dev_call(res, W.BH_CURVE_P256, n, flag | _lib.BH_F_NO_LOW_S)
        chunk_env(None)
        whole = R.dev_call(res, W.BH_CURVE_P256, n, flag, timing=True)
    finally:
        chunk_env(None)
        res.free()
    for name, got, exp in (("plain", plain, want), ("timed", timed, want),
                           ("no_low_s", no_rule, nls), ("one pass", whole, want)):
        R.check_result(got, n, exp, (h, name))
        assert got["stats"] == [1, n], name
    assert whole["reason"] == plain["reason"] and whole["words"] == plain["words"]
    for name, got in (("timed", timed), ("one pass", whole)):
        t = got["timing"]
        assert t["n_keycomb"] + t["n_ladder"] == R.count_math(want), (name, t)
        assert t["prep_ms"] > 0 and t["inv_ms"] > 0, (name, t)
        assert all(t[s] >= 0 for s in STAGES), (name, t)


# ---------------------------------------------------------------- 4. deferred stage timing
@pytest.fixture(scope="module")
def w3000(L):
    """3000 P-256 records over 50 keys, 200-byte messages, one in eight
    corrupted; resident on device 0. Expected reasons: the generator's."""
    w = workload.generate(3000, 50, 200, 8, seed=77)
    res = R.Resident(w.arrays())
    yield w, res
    res.free()


def timing_end(L):
    t = _lib.BhTiming(prep_ms=7.0, keycomb_ms=3.0, n_keycomb=5, n_ladder=9, n_keytables=2, wide=3)
    rc = L.bh_timing_end(0, ctypes.byref(t))
    return rc, R.timing_dict(t)


ZERO = {f: 0 for f in R.TIMING_FIELDS}
FLAGS = _lib.BH_F_HASH_SHA256


def test_deferred_timing_three_calls(L, w3000):
    """bh_timing_begin, three calls with sync = 0 and no bh_timing, bh_timing_end:
    every call's results are right, the times are those of recorded events
    (non-negative, the stages every pass runs positive), the counts are the
    last call's and `wide` is what a call with its own bh_timing reports."""
    w, res = w3000
    own = R.dev_call(res, 0, w.n, FLAGS, timing=True)
    R.check_result(own, w.n, w.reason, "own timing")
    outs = [R.Outputs(w.n) for _ in range(3)]  # on the device before the first call
    _lib.check(L.bh_timing_begin(0))
    calls = [R.dev_call(res, 0, w.n, FLAGS, sync=0, out=o) for o in outs]
    rc, t = timing_end(L)
    assert rc == _lib.BH_OK
    _lib.check(L.bh_sync(0))
    for k, (got, o) in enumerate(zip(calls, outs)):
        assert got["stats"] == [1, w.n] and got["timing"] is None
        R.check_result(o.read(), w.n, w.reason, f"deferred call {k}")
    assert all(t[s] >= 0 for s in STAGES), t
    assert t["prep_ms"] > 0 and t["inv_ms"] > 0 and t["build_ladder_ms"] + t["keycomb_ms"] > 0, t
    assert t["n_keycomb"] + t["n_ladder"] == R.count_math(w.reason), t
    assert t["n_keycomb"] + t["n_ladder"] == own["timing"]["n_keycomb"] + own["timing"]["n_ladder"]
    assert t["wide"] == own["timing"]["wide"], (t, own["timing"])


def test_deferred_timing_forced_passes(L, w3000, chunk_env):
    """One untimed call in passes of 1024, 1024 and 952 between begin and end:
    three event sets from the pool; the times are positive and the counts are
    those of the last pass's 952 records (include/bdls_hip.h)."""
    w, res = w3000
    out = R.Outputs(w.n)
    _lib.check(L.bh_timing_begin(0))
    chunk_env(1024)
    try:
        got = R.dev_call(res, 0, w.n, FLAGS, sync=0, out=out)
    finally:
        chunk_env(None)
    rc, t = timing_end(L)
    assert rc == _lib.BH_OK and got["stats"] == [1, w.n]
    _lib.check(L.bh_sync(0))
    R.check_result(out.read(), w.n, w.reason, "forced passes")
    assert all(t[s] >= 0 for s in STAGES), t
    assert t["prep_ms"] > 0 and t["inv_ms"] > 0 and t["build_ladder_ms"] + t["keycomb_ms"] > 0, t
    assert w.n - 2048 == 952
    assert t["n_keycomb"] + t["n_ladder"] == R.count_math(w.reason[2048:]), t


def test_deferred_timing_reset_and_end(L, w3000):
    """begin resets what an earlier begin collected; end with nothing deferred,
    and end without a begin, fill an all-zero bh_timing and return BH_OK; after
    end nothing is deferred, and a call with its own bh_timing still fills it."""
    w, res = w3000
    _lib.check(L.bh_timing_begin(0))
    assert timing_end(L) == (_lib.BH_OK, ZERO)  # begin, end
    assert timing_end(L) == (_lib.BH_OK, ZERO)  # end alone
    _lib.check(L.bh_timing_begin(0))
    got = R.dev_call(res, 0, w.n, FLAGS)  # one pass deferred ...
    R.check_result(got, w.n, w.reason, "before the second begin")
    _lib.check(L.bh_timing_begin(0))  # ... and dropped by the second begin
    assert timing_end(L) == (_lib.BH_OK, ZERO)
    # after end: an untimed call defers nothing, a timed one fills its own bh_timing
    got = R.dev_call(res, 0, w.n, FLAGS)
    R.check_result(got, w.n, w.reason, "after end")
    assert timing_end(L) == (_lib.BH_OK, ZERO)
    own = R.dev_call(res, 0, w.n, FLAGS, timing=True)
    R.check_result(own, w.n, w.reason, "own timing after end")
    t = own["timing"]
    assert t["prep_ms"] > 0 and t["inv_ms"] > 0 and t["build_ladder_ms"] + t["keycomb_ms"] > 0, t
    assert t["n_keycomb"] + t["n_ladder"] == R.count_math(w.reason), t
    # a timed call between begin and end keeps its own events: nothing deferred by it
    _lib.check(L.bh_timing_begin(0))
    own2 = R.dev_call(res, 0, w.n, FLAGS, timing=True)
    assert own2["timing"]["n_keycomb"] + own2["timing"]["n_ladder"] == R.count_math(w.reason)
    assert timing_end(L) == (_lib.BH_OK, ZERO)


def test_deferred_timing_errors(L):
    BH_E_INVALID, BH_E_NOT_INIT = -1, -2
    assert L.bh_timing_end(0, None) == BH_E_INVALID
    assert L.bh_timing_begin(63) == BH_E_NOT_INIT
    t = _lib.BhTiming()
    assert L.bh_timing_end(63, ctypes.byref(t)) == BH_E_NOT_INIT
    # neither left device 0 deferring
    assert timing_end(L) == (_lib.BH_OK, ZERO)
