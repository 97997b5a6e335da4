"""GPU: the P-384 key registry (bh_keys384_*) and the table route of the P-384
pass (k384_plan, k384_keywin), against the golden fixture, the crafted fixture
tests/golden/p384_keywin_vectors.jsonl, a libcrypto-signed batch, and the same
calls with the registry empty: results never depend on the registry. Every
test leaves the registry empty (the other P-384 tests assert n_keycomb == 0)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib
from bdls_amd.bccsp import ECDSAPublicKey, HipCSP, verify_packed
from oracle import ecdsa_ref as O
from tests import p384_util as U
from tests.conftest import ROOT, pack
from tests.p384_util import N, P, P384

pytestmark = pytest.mark.gpu
C384 = _lib.BH_CURVE_P384
KEYWIN = os.path.join(ROOT, "tests", "golden", "p384_keywin_vectors.jsonl")


@pytest.fixture(scope="module")
def csp():
    return HipCSP()


@pytest.fixture
def reg(csp, request):
    """The library, with the P-384 registry back at its default size and empty afterwards."""
    L = _lib.lib()
    request.addfinalizer(lambda: _lib.check(L.bh_keys384_reserve(-1, 256)))
    _lib.check(L.bh_keys384_clear(-1))
    return L


@pytest.fixture(scope="module")
def batch600():
    return U.signed_batch(U.LibCrypto(), 600, 24, seed=600, family="SHA2")


def load(path):
    with open(path) as f:
        return [json.loads(l) for l in f]


def expect(recs, no_low_s):
    return np.array([r.get("reason_no_low_s", r["reason"]) if no_low_s else r["reason"]
                     for r in recs], np.uint8)


def key_bytes(r):
    return bytes.fromhex(r["qx"] + r["qy"])


def is_point(kb):
    x, y = int.from_bytes(kb[:48], "big"), int.from_bytes(kb[48:], "big")
    return x < P and y < P and O.on_curve(P384, x, y)


def distinct_keys(recs):
    return list(dict.fromkeys(key_bytes(r) for r in recs))


def register(L, keys, device=0):
    st = np.full(len(keys), 99, np.uint8)
    _lib.check(L.bh_keys384_register(device, b"".join(keys), len(keys), st.ctypes.data))
    return st


def count(L, device=0):
    c = ctypes.c_size_t(99)
    _lib.check(L.bh_keys384_count(device, ctypes.byref(c)))
    return c.value


def run_dev(L, arrs, n, flags):
    """bh_verify_dev with stage timing: (reasons, validity bits, timing)."""
    dev = [_lib.DeviceArray.from_numpy(0, a) for a in arrs]
    bm = _lib.DeviceArray(0, 8 * ((n + 63) // 64))
    rs = _lib.DeviceArray(0, n)
    b = _lib.BhBatch(*[d.ptr for d in dev])
    t = _lib.BhTiming()
    _lib.check(L.bh_verify_dev(0, C384, ctypes.byref(b), n, flags, bm.ptr, rs.ptr, None, 1,
                               ctypes.byref(t)))
    reason = rs.to_numpy(np.uint8, n)
    words = bm.to_numpy(np.uint64, (n + 63) // 64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    for d in dev + [bm, rs]:
        d.free()
    return reason, bits, t


def on_table(recs, want, registered):
    """Records that pass prep (reason OK or MATH) with a registered key."""
    return int(sum(1 for r, w in zip(recs, want) if w in (O.R_OK, O.R_MATH) and key_bytes(r) in registered))


def check_routed(L, recs, fused, flags, want, registered):
    reason, bits, t = run_dev(L, U.pack384(recs, fused), len(recs), flags)
    bad = [(r.get("tag"), int(g), int(w)) for r, g, w in zip(recs, reason, want) if g != w]
    assert not bad, bad[:8]
    assert (bits == (want == 0)).all()
    assert t.n_keycomb == on_table(recs, want, registered)
    assert t.n_keycomb + t.n_ladder == len(recs)
    assert t.n_keytables == 0 and t.wide == 0
    if t.n_keycomb:
        assert t.keycomb_ms > 0 and t.plan_ms > 0
    return t


@pytest.mark.parametrize("fixture", ["golden", "keywin"])
def test_fixture_resident_with_keys_registered(reg, fixture):
    recs = U.load_golden384() if fixture == "golden" else load(KEYWIN)
    keys = [k for k in distinct_keys(recs) if is_point(k)]
    assert (register(reg, keys) == 0).all() and count(reg) == len(keys)
    for no_low_s in (False, True):
        t = check_routed(reg, recs, False, _lib.BH_F_NO_LOW_S if no_low_s else 0,
                         expect(recs, no_low_s), set(keys))
        assert t.n_keycomb > 0 and t.keycomb_ms > 0
    fused = [r for r in recs if r.get("family") == "SHA2"]
    if fused:
        t = check_routed(reg, fused, True, _lib.BH_F_HASH_SHA256, expect(fused, False), set(keys))
        assert t.n_keycomb > 0 and t.keycomb_ms > 0


def test_mixed_routes(reg, batch600):
    """Every other key registered: each wave of the plan holds both routes."""
    recs, want = batch600
    assert (want == O.R_MATH).sum() > 20 and (want == O.R_BAD_KEY).sum() > 5
    good = [k for k in distinct_keys(recs) if is_point(k)]
    assert len(good) == 24
    arrs = U.pack384(recs, True)
    r0, b0, t0 = run_dev(reg, arrs, len(recs), _lib.BH_F_HASH_SHA256)
    assert (t0.n_keycomb, t0.n_ladder, t0.keycomb_ms, t0.plan_ms) == (0, len(recs), 0.0, 0.0)
    half = set(good[::2])
    assert (register(reg, sorted(half)) == 0).all() and count(reg) == 12
    r1, b1, t1 = run_dev(reg, arrs, len(recs), _lib.BH_F_HASH_SHA256)
    assert (r1 == r0).all() and (b1 == b0).all() and (r1 == want).all()
    assert t1.n_keycomb == on_table(recs, want, half) and 200 < t1.n_keycomb < 320
    assert t1.n_keycomb + t1.n_ladder == len(recs)
    assert t1.keycomb_ms > 0 and t1.build_ladder_ms > 0
    _lib.check(reg.bh_keys384_clear(0))
    r2, b2, t2 = run_dev(reg, arrs, len(recs), _lib.BH_F_HASH_SHA256)
    assert (r2 == r0).all() and (b2 == b0).all() and t2.n_keycomb == 0 and t2.n_ladder == len(recs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_list_edges(reg, batch600, n):
    """All keys registered, none, and the key of exactly one record (the last,
    given a key of its own: a valid signature under it becomes BH_R_MATH)."""
    recs, want = [dict(r) for r in batch600[0][:n]], batch600[1][:n].copy()
    own = O.pubkey(P384, 7777 + n)
    recs[n - 1].update(qx=U.h48(own[0]), qy=U.h48(own[1]))
    if want[n - 1] != O.R_HIGH_S:  # (the low-S rule comes before the key)
        want[n - 1] = O.R_MATH
    arrs = U.pack384(recs, True)
    every = [k for k in distinct_keys(recs) if is_point(k)]
    for registered in (every, [], [key_bytes(recs[n - 1])]):
        _lib.check(reg.bh_keys384_clear(0))
        if registered:
            assert (register(reg, registered) == 0).all()
        reason, bits, t = run_dev(reg, arrs, n, _lib.BH_F_HASH_SHA256)
        assert (reason == want).all() and (bits == (want == 0)).all()
        assert t.n_keycomb == on_table(recs, want, set(registered)) and t.n_keycomb + t.n_ladder == n
        if len(registered) == 1:
            assert t.n_keycomb == (1 if want[n - 1] == O.R_MATH else 0)
        elif registered:
            assert t.n_ladder == int(np.isin(want, (O.R_HIGH_S, O.R_BAD_KEY)).sum())


def test_three_chunks_child_process(batch600, tmp_path):
    """BH_P384_CHUNK=64 in a fresh child: 130 records are three chunks, each
    planning its own two lists; the bitmap words concatenate."""
    recs, want = batch600[0][:130], batch600[1][:130]
    path = tmp_path / "recs.json"
    path.write_text(json.dumps(recs))
    code = (
        "import ctypes, json, sys\n"
        "sys.path.insert(0, '.')\n"
        "import numpy as np\n"
        "from bdls_amd import _lib\n"
        "from bdls_amd.bccsp import HipCSP\n"
        "from tests import p384_util as U\n"
        "from tests.test_p384_keys_gpu import distinct_keys, register, run_dev\n"
        f"recs = json.load(open({str(path)!r}))\n"
        "HipCSP()\n"
        "L = _lib.lib()\n"
        "keys = distinct_keys(recs)[::2]\n"
        "st = register(L, keys)\n"
        "reason, bits, t = run_dev(L, U.pack384(recs, True), len(recs), _lib.BH_F_HASH_SHA256)\n"
        "print(json.dumps({'reason': reason.tolist(), 'bits': bits.tolist(), 'st': st.tolist(),\n"
        "                  'kc': t.n_keycomb, 'lad': t.n_ladder, 'keys': [k.hex() for k in keys]}))\n")
    env = dict(os.environ, BH_P384_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["reason"] == want.tolist() and res["bits"] == (want == 0).tolist()
    registered = {bytes.fromhex(k) for k, s in zip(res["keys"], res["st"]) if s == 0}
    assert res["kc"] == on_table(recs, want, registered) and res["kc"] > 30
    assert res["kc"] + res["lad"] == 130


def test_registry_semantics(reg, batch600):
    recs, want = batch600
    good = [k for k in distinct_keys(recs) if is_point(k)]
    bad = next(k for k in distinct_keys(recs) if not is_point(k))
    assert count(reg) == 0
    assert list(register(reg, good[:3])) == [0, 0, 0] and count(reg) == 3
    assert list(register(reg, [good[1], good[3], good[1]])) == [0, 0, 0] and count(reg) == 4
    assert list(register(reg, [bad, good[0]])) == [7, 0] and count(reg) == 4
    assert count(reg, -1) == 4
    # capacity 2: the third key reports 255 and its records verify on the ladder
    _lib.check(reg.bh_keys384_reserve(0, 2))
    assert count(reg) == 0
    assert list(register(reg, good[:3])) == [0, 0, 255] and count(reg) == 2
    arrs = U.pack384(recs, True)
    r1, b1, t1 = run_dev(reg, arrs, len(recs), _lib.BH_F_HASH_SHA256)
    assert (r1 == want).all() and (b1 == (want == 0)).all()
    assert t1.n_keycomb == on_table(recs, want, set(good[:2])) > 0
    assert (r1[[i for i, r in enumerate(recs) if key_bytes(r) == good[2]]] ==
            want[[i for i, r in enumerate(recs) if key_bytes(r) == good[2]]]).all()
    _lib.check(reg.bh_keys384_clear(0))
    assert count(reg) == 0
    r2, b2, t2 = run_dev(reg, arrs, len(recs), _lib.BH_F_HASH_SHA256)
    assert t2.n_keycomb == 0 and t2.n_ladder == len(recs) and (r2 == r1).all() and (b2 == b1).all()
    # the slots are free again
    assert list(register(reg, good[2:4])) == [0, 0] and count(reg) == 2


def test_host_verify_sha384_and_p256_untouched(reg, csp, batch600, golden):
    recs, want = batch600
    L = reg
    c256 = ctypes.c_size_t()
    _lib.check(L.bh_keys_count(0, 0, ctypes.byref(c256)))
    v256, r256 = verify_packed(*pack(golden, False))
    keys = [ECDSAPublicKey(int(r["qx"], 16), int(r["qy"], 16), curve="P-384") for r in recs[:24]]
    st = csp.register_keys_p384(keys, device=0)
    assert sorted(set(st.tolist())) in ([0], [0, 7]) and count(L) == int((st == 0).sum()) >= 20
    registered = {k.raw() for k, s in zip(keys, st) if s == 0}
    # host bh_verify: same reasons, one batch per call
    b0 = _lib.device_stats()
    valid, reason = verify_packed(*U.pack384(recs, True), curve=C384, flags=_lib.BH_F_HASH_SHA256)
    assert (reason == want).all() and (valid == (want == 0)).all()
    assert _lib.device_stats() == (b0[0] + 1, b0[1] + len(recs))
    # SHA-384 messages: the digest pass, then the routed curve pass
    lc = U.LibCrypto()
    import hashlib
    rng = np.random.default_rng(384)
    recs384, want384 = [], []
    for i in range(96):
        d = 1000 + i % 5
        qx, qy = O.pubkey(P384, d)
        msg = rng.integers(0, 256, 50 + i, dtype=np.uint8).tobytes()
        k = lc.key(d, qx, qy)
        r_, s_ = lc.sign(k, hashlib.sha384(msg).digest())
        lc.free_key(k)
        s_ = min(s_, N - s_)
        if i % 6 == 1:
            msg = msg[:-1] + bytes([msg[-1] ^ 1])
        recs384.append({"qx": U.h48(qx), "qy": U.h48(qy), "msg": msg.hex(),
                        "sig": O.marshal_ecdsa_signature(r_, s_).hex()})
        want384.append(O.R_MATH if i % 6 == 1 else O.R_OK)
    want384 = np.array(want384, np.uint8)
    arrs = U.pack384(recs384, True)
    ra, ba, ta = run_dev(L, arrs, 96, _lib.BH_F_HASH_SHA384)
    assert (ra == want384).all() and ta.n_keycomb == 0
    keys384 = distinct_keys(recs384)
    assert (register(L, keys384[:3]) == 0).all()
    rb, bb, tb = run_dev(L, arrs, 96, _lib.BH_F_HASH_SHA384)
    assert (rb == ra).all() and (bb == ba).all()
    assert tb.n_keycomb == on_table(recs384, want384, set(keys384[:3])) > 0
    assert tb.n_keycomb + tb.n_ladder == 96
    vh, rh = verify_packed(*arrs, curve=C384, flags=_lib.BH_F_HASH_SHA384)
    assert (rh == ra).all()
    # the P-256 registry and a P-256 pass are as they were
    c2 = ctypes.c_size_t()
    _lib.check(L.bh_keys_count(0, 0, ctypes.byref(c2)))
    assert c2.value == c256.value
    v2, r2 = verify_packed(*pack(golden, False))
    assert (v2 == v256).all() and (r2 == r256).all()
    assert registered
