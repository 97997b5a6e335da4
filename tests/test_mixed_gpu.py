"""GPU: bh_verify_mixed against bh_verify and the fixtures, and the Fabric
callers over inputs that mix P-256 and P-384 identities, against the
generator's by-construction expectations and the oracle with its key
extraction restated for both curves (tests/mixed_util.py). Every test leaves
the P-384 key registry empty (the other P-384 tests assert n_keycomb == 0)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bdls_amd import _lib, fabric
from bdls_amd.bccsp import HipCSP, verify_mixed, verify_packed, x509_check_signatures
from bdls_amd.workload import fabric as F
from oracle import ecdsa_ref as O
from oracle import fabric_ref as R
from tests import mixed_util as M
from tests import p384_util as U
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
C256, C384 = _lib.BH_CURVE_P256, _lib.BH_CURVE_P384
FLAG = {"SHA2": _lib.BH_F_HASH_SHA256, "SHA3": _lib.BH_F_HASH_SHA3_256}
SIZES = (1, 63, 64, 65, 129, 600)
PATTERNS = ("alternating", "p256", "p384", "runs70")


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


def count384(L):
    c = ctypes.c_size_t(99)
    _lib.check(L.bh_keys384_count(0, ctypes.byref(c)))
    return c.value


@pytest.fixture(scope="module")
def pools():
    return {f: M.pool(f) for f in ("SHA2", "SHA3")}


def per_curve(recs, flags, fused=True):
    """bh_verify over the records of each curve, in record order: reasons, validity."""
    reason = np.zeros(len(recs), np.uint8)
    valid = np.zeros(len(recs), bool)
    for c in (C256, C384):
        ix = [i for i, r in enumerate(recs) if r["curve"] == c]
        if not ix:
            continue
        sub = [recs[i] for i in ix]
        _, pub, _, sig, so, sl, msg, mo, ml, _, _ = M.build_mixed(sub, False, fused)
        v, rs = verify_packed(pub, sig, so, sl, msg, mo, ml, flags=flags, curve=c)
        reason[ix], valid[ix] = rs, v
    return reason, valid


def check_mixed(recs, arrs, flags, want, ref):
    valid, reason = verify_mixed(*arrs, flags=flags)
    bad = [(i, r.get("tag"), int(g), int(w)) for i, (r, g, w) in enumerate(zip(recs, reason, want))
           if g != w]
    assert not bad, bad[:8]
    assert (reason == ref[0]).all() and (valid == ref[1]).all()
    assert (valid == (np.asarray(want) == 0)).all()


@pytest.mark.parametrize("two_span", [False, True])
@pytest.mark.parametrize("family", ["SHA2", "SHA3"])
def test_mixed_against_bh_verify(csp, pools, family, two_span):
    p256, p384 = pools[family]
    for no_low_s in (False, True):
        flags = FLAG[family] | (_lib.BH_F_NO_LOW_S if no_low_s else 0)
        for n in SIZES:
            for pat in PATTERNS:
                recs = M.pick(M.pattern(pat, n), p256, p384)
                want = [M.expect(r, no_low_s) for r in recs]
                ref = per_curve(recs, flags) if (pat == "alternating" or n == 129) else \
                    (np.array(want, np.uint8), np.array(want) == 0)
                check_mixed(recs, M.build_mixed(recs, two_span), flags, want, ref)


def test_mixed_digest_mode(csp, golden):
    g384 = [dict(r, curve=C384) for r in U.load_golden384()]
    g256 = []
    for r in golden:
        r = dict(r, curve=C256)
        if r["reason"] == O.R_HIGH_S:
            rc, rr, ss = O.unmarshal_ecdsa_signature(bytes.fromhex(r["sig"]))
            r["reason_no_low_s"] = O.go_ecdsa_verify(O.P256, int(r["qx"], 16), int(r["qy"], 16),
                                                     bytes.fromhex(r["digest"]), rr, ss)
        g256.append(r)
    for no_low_s in (False, True):
        flags = _lib.BH_F_NO_LOW_S if no_low_s else 0
        for n in SIZES:
            for pat in PATTERNS:
                recs = M.pick(M.pattern(pat, n), g256, g384)
                want = [M.expect(r, no_low_s) for r in recs]
                ref = per_curve(recs, flags, fused=False) if pat == "alternating" else \
                    (np.array(want, np.uint8), np.array(want) == 0)
                check_mixed(recs, M.build_mixed(recs, False, fused=False), flags, want, ref)


def test_mixed_bitmap_padding_and_stats(csp, pools):
    """Every bit of the ceil(n / 8) bytes is written, padding zero, whatever the
    caller left there; one batch is counted per non-empty curve group."""
    p256, p384 = pools["SHA2"]
    L = _lib.lib()
    for pat, batches in (("alternating", 2), ("p256", 1), ("p384", 1)):
        n = 13
        recs = M.pick(M.pattern(pat, n), p256, p384)
        arrs = M.build_mixed(recs, True)
        b = _lib.BhMBatch(*[None if a is None else a.ctypes.data for a in arrs])
        bm = np.full(2, 0xFF, np.uint8)
        rs = np.full(n, 0xEE, np.uint8)
        s0 = _lib.device_stats()
        _lib.check(L.bh_verify_mixed(ctypes.byref(b), n, FLAG["SHA2"], bm.ctypes.data, rs.ctypes.data))
        s1 = _lib.device_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (batches, n)
        want = np.array([r["reason"] for r in recs], np.uint8)
        assert (rs == want).all()
        bits = np.unpackbits(bm, bitorder="little")
        assert (bits[:n] == (want == 0)).all() and not bits[n:].any()


def test_mixed_several_p384_chunks(csp, pools, tmp_path):
    """BH_P384_CHUNK is read once per process: a fresh child with chunks of 64
    runs the P-384 group of 600 alternating two-span records in five chunks,
    the P-256 records sitting between them in the caller's buffers."""
    p256, p384 = pools["SHA2"]
    recs = M.pick(M.pattern("alternating", 600), p256, p384)
    want = [r["reason"] for r in recs]
    path = tmp_path / "recs.json"
    path.write_text(json.dumps(recs))
    code = (
        "import json, sys\n"
        "sys.path.insert(0, '.')\n"
        "from bdls_amd import _lib\n"
        "from bdls_amd.bccsp import verify_mixed\n"
        "from tests import mixed_util as M\n"
        f"recs = json.load(open({str(path)!r}))\n"
        "valid, reason = verify_mixed(*M.build_mixed(recs, True), flags=_lib.BH_F_HASH_SHA256)\n"
        "print(json.dumps({'reason': [int(x) for x in reason], 'valid': [bool(x) for x in valid]}))\n")
    env = dict(os.environ, BH_P384_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["reason"] == want and res["valid"] == [w == 0 for w in want]


def test_mixed_results_do_not_depend_on_the_registry(reg, pools):
    p256, p384 = pools["SHA2"]
    recs = M.pick(M.pattern("alternating", 129), p256, p384)
    keys = list(dict.fromkeys(bytes.fromhex(r["qx"] + r["qy"]) for r in recs if r["curve"] == C384))
    flags = FLAG["SHA2"]
    runs = []
    for step in ("empty", "registered", "cleared"):
        if step == "registered":
            st = np.full(len(keys), 99, np.uint8)
            _lib.check(reg.bh_keys384_register(0, b"".join(keys), len(keys), st.ctypes.data))
            assert count384(reg) > 0
        elif step == "cleared":
            _lib.check(reg.bh_keys384_clear(-1))
            assert count384(reg) == 0
        for two in (False, True):
            v, rs = verify_mixed(*M.build_mixed(recs, two), flags=flags)
            runs.append((v.tolist(), rs.tolist()))
    assert all(x == runs[0] for x in runs)
    assert runs[0][1] == [r["reason"] for r in recs]


# ---------------------------------------------------------------- the Fabric callers
def _got(t):
    return (t.status, t.creator, t.endorse, t.valid_endorsers)


def _want(fb, i):
    return (fb.tx_status[i], fb.tx_creator[i], fb.tx_endorse[i], fb.tx_valid_identities[i])


@pytest.fixture(scope="module")
def mixed_classes_block():
    return F.generate_fabric_block(ntx=2 * len(F.CORRUPTIONS), classes=F.CORRUPTIONS,
                                   p384_orgs=2, norgs=4)


@pytest.fixture(scope="module")
def p384_block():
    return F.generate_fabric_block(ntx=40, p384_orgs=4, norgs=4, nclients=8)


@pytest.mark.parametrize("which", ["classes", "all_p384"])
def test_block_preverify_mixed(csp, mixed_classes_block, p384_block, which, monkeypatch):
    fb = mixed_classes_block if which == "classes" else p384_block
    M.patch_oracle(monkeypatch)
    want = [_want(fb, i) for i in range(fb.ntx)]
    oracle = [_got(o) for o in R.validate_block(fb.block, M.make_verify(fb.p384_keys))]
    assert oracle == want
    if which == "classes":
        assert {"creator_high_s", "endorse_high_s", "endorse_dup", "endorse_dup_after_invalid"} \
            <= set(fb.tx_class)
    else:
        assert len(fb.p384_keys) == len(fb.identities)
    got = fabric.block_preverify(fb.block)
    assert [_got(t) for t in got] == want
    got2, creators, ends = fabric.block_preverify_refs(fb.block)
    assert [_got(t) for t in got2] == want
    assert [c.reason for c in creators if c is not None] == \
        [w[1] for w, c in zip(want, creators) if c is not None]
    flat = [r for w in want for r in w[2]]
    assert len(ends) == len(flat)
    assert all(e is None or e.reason == r for e, r in zip(ends, flat))


def test_twin_certificates_mixed(csp, mixed_classes_block, monkeypatch):
    """The twin (r, n - s) of a P-384 CA's certificate signature is the same
    identity: its endorsement after the original's is a duplicate."""
    fb = mixed_classes_block
    M.patch_oracle(monkeypatch)
    peer = next(i for i in fb.identities if i.curve == F.P384)
    der = R.pem_decode(peer.cert_pem)
    x, y, tbs_raw, sig = M.cert_key(der)
    rc, r, s = O.unmarshal_ecdsa_signature(sig)
    assert rc == O.R_OK
    twin = F.serialized_identity(peer.mspid, F.pem(F.x509_cert(
        tbs_raw, O.marshal_ecdsa_signature(r, U.N - s), F.OID_ECDSA_SHA384)))
    assert twin != peer.serialized
    L = F._gen()
    data = b"twin data"
    sg = F.sign(L, peer.priv, data, 99)
    sets = [[(peer.serialized, data, sg), (twin, data, sg)],
            [(twin, data, sg[:-1] + bytes([sg[-1] ^ 1])), (peer.serialized, data, sg)]]
    verify = M.make_verify(fb.p384_keys)
    want = [R.signature_set_to_valid_identities(s, verify) for s in sets]
    assert want == [([0, 253], 1), ([9, 0], 1)]
    assert fabric.signature_sets_verify(sets) == want


def test_p256_only_blocks_issue_the_same_device_calls(csp):
    """Without a P-384 identity the callers make the calls they always made:
    one device batch for a clean block, two for the classes block (its
    follow-up round)."""
    for fb, batches in ((F.generate_fabric_block(ntx=60, seed=3, corrupt_den=0), 1),
                        (F.generate_fabric_block(ntx=2 * len(F.CORRUPTIONS), corrupt_den=0,
                                                 classes=F.CORRUPTIONS, seed=7), 2)):
        s0 = _lib.device_stats()
        got = fabric.block_preverify(fb.block)
        s1 = _lib.device_stats()
        assert [_got(t) for t in got] == [_want(fb, i) for i in range(fb.ntx)]
        assert s1[0] - s0[0] == batches and s1[1] - s0[1] >= fb.n_signatures


def _envelopes(block):
    return R.unmarshal(block, R.BLOCK_SPEC)["data"]["data"]


def test_signature_sets_and_envelopes_mixed(csp, mixed_classes_block, monkeypatch):
    fb = mixed_classes_block
    M.patch_oracle(monkeypatch)
    verify = M.make_verify(fb.p384_keys)
    envs = _envelopes(fb.block)
    assert fabric.envelopes_preverify(envs) == [R.sigfilter(e, verify) for e in envs]
    sets = []
    for env in envs:
        try:
            e = R.unmarshal(env, R.ENVELOPE_SPEC)
            pl = R.unmarshal(e["payload"], R.PAYLOAD_SPEC)
            tx = R.unmarshal(pl["data"], R.TRANSACTION_SPEC)
            cap = R.unmarshal(tx["actions"][0]["payload"], R.CC_ACTION_PAYLOAD_SPEC)
        except (R.DecodeError, IndexError, TypeError):
            continue
        prp = cap["action"]["proposal_response_payload"]
        sets.append([(x["endorser"], prp + x["endorser"], x["signature"])
                     for x in cap["action"]["endorsements"]])
    sets.append([])
    assert len(sets) > 15
    want = [R.signature_set_to_valid_identities(s, verify) for s in sets]
    assert any(253 in w[0] for w in want) and any(9 in w[0] for w in want)
    assert fabric.signature_sets_verify(sets) == want


def test_block_signatures_mixed(csp, monkeypatch):
    M.patch_oracle(monkeypatch)
    _, orderers, _ = F.make_identities(F._gen(), 21, 4, 0, 2)
    verify = M.make_verify(M.p384_keys_of(orderers))
    blocks, exp = F.generate_signed_blocks(nblocks=len(F.BLOCKSIG_CORRUPTIONS),
                                           classes=F.BLOCKSIG_CORRUPTIONS, p384_orgs=2)
    assert [R.block_signatures(b, verify) for b in blocks] == exp
    assert [tuple(g) for g in fabric.block_signatures_preverify(blocks)] == exp
    # BFT: consenters 1 and 2 hold P-384 keys
    _, orderers, _ = F.make_identities(F._gen(), 31, 4, 0, 2)
    verify = M.make_verify(M.p384_keys_of(orderers))
    blocks, cons, exp = F.generate_bft_signed_blocks(nblocks=len(F.BFT_BLOCKSIG_CORRUPTIONS),
                                                     classes=F.BFT_BLOCKSIG_CORRUPTIONS,
                                                     p384_orgs=2)
    assert [R.block_signatures(b, verify, bft=True, consenters=cons) for b in blocks] == exp
    got = fabric.block_signatures_preverify(blocks, bft=True, consenters=cons)
    assert [tuple(g) for g in got] == exp


def _sent_keys(fb):
    """The key of every record the block sends to the device, in any order."""
    want = [_want(fb, i) for i in range(fb.ntx)]
    _, creators, ends = fabric.block_preverify_refs(fb.block, decode_only=True)
    by_ser = {i.serialized: i.pub for i in fb.identities}
    sent = [by_ser[c.identity] for c, w in zip(creators, want) if c is not None and w[1] != 255]
    flat = [r for w in want for r in w[2]]
    return sent + [by_ser[e.identity] for e, r in zip(ends, flat) if e is not None and r <= 10]


def test_keep_keys_fills_the_p384_registry(reg, p384_block):
    """BH_FAB_F_KEEP_KEYS: the P-384 keys at their second sighting (a record
    sent to the device under the key; two within one call count) are
    registered before the call's device work, each once; a cleared registry
    fills again; results never change."""
    fb = p384_block
    want = [_want(fb, i) for i in range(fb.ntx)]
    sent = _sent_keys(fb)
    twice = {k for k in sent if sent.count(k) >= 2}
    assert len(twice) == len(set(sent)) == 12  # 4 peers and 8 clients, each signing often
    assert count384(reg) == 0
    assert [_got(t) for t in fabric.block_preverify(fb.block)] == want
    assert count384(reg) == 0  # without the flag nothing is registered
    assert [_got(t) for t in fabric.block_preverify(fb.block, keep_keys=True)] == want
    assert count384(reg) == len(twice)
    assert [_got(t) for t in fabric.block_preverify(fb.block, keep_keys=True)] == want
    assert count384(reg) == len(twice)
    _lib.check(reg.bh_keys384_clear(-1))
    assert count384(reg) == 0
    assert [_got(t) for t in fabric.block_preverify(fb.block, keep_keys=True)] == want
    assert count384(reg) == len(twice)
    # a block of other identities where some clients sign once: those keys
    # wait for their second sighting, which the next call brings
    fb2 = F.generate_fabric_block(ntx=40, p384_orgs=4, norgs=4, seed=5)
    want2 = [_want(fb2, i) for i in range(fb2.ntx)]
    sent2 = _sent_keys(fb2)
    twice2 = {k for k in sent2 if sent2.count(k) >= 2}
    assert 4 <= len(twice2) < len(set(sent2)) and not set(sent2) & set(sent)
    assert [_got(t) for t in fabric.block_preverify(fb2.block, keep_keys=True)] == want2
    assert count384(reg) == len(twice) + len(twice2)
    assert [_got(t) for t in fabric.block_preverify(fb2.block, keep_keys=True)] == want2
    assert count384(reg) == len(twice) + len(set(sent2))


def test_generated_p384_certificates_verify_under_their_cas(csp, mixed_classes_block):
    """bh_verify_x509_ex: every generated certificate under its org's CA key,
    ecdsa-with-SHA384 for the P-384 orgs."""
    from bdls_amd.bccsp import ECDSAPublicKey
    fb = mixed_classes_block
    certs, issuers = [], []
    for ident in fb.identities:
        o = int(ident.mspid[3:-3]) - 1
        pub = fb.cas[o][1]
        w = len(pub) // 2
        certs.append(R.pem_decode(ident.cert_pem))
        issuers.append(ECDSAPublicKey(int.from_bytes(pub[:w], "big"), int.from_bytes(pub[w:], "big"),
                                      "P-384" if w == 48 else "P-256"))
    assert {k.curve for k in issuers} == {"P-256", "P-384"}
    valid, reason = x509_check_signatures(certs, issuers)
    assert all(valid) and not any(reason)
    # and not under another org's CA of the same curve
    swapped = [issuers[(i + 1) % len(issuers)] if issuers[(i + 1) % len(issuers)].curve == k.curve
               and issuers[(i + 1) % len(issuers)] != k else None for i, k in enumerate(issuers)]
    pairs = [(c, s) for c, s in zip(certs, swapped) if s is not None]
    assert pairs
    valid, _ = x509_check_signatures([c for c, _ in pairs], [s for _, s in pairs])
    assert not any(valid)
