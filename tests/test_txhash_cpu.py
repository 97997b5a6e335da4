"""bh_hash and bh_fabric_block_prevalidate without a GPU: hashspan.h's loaders
and compare step through the host harness (tests/native_hash) against hashlib,
the C ABI's argument checks, and the block path's decode against the
restatement of the two Go checks in tests/txhash_util.py."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from bdls_amd import _lib, fabric
from bdls_amd.workload import fabric as F
from tests import hash_cases as C
from tests import txhash_util as U
from tests.conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "build", "libhostsimhash.so")


@pytest.fixture(scope="module")
def hs():
    L = ctypes.CDLL(HARNESS)  # missing: an error, not a skip
    vp = ctypes.c_void_p
    for f in (L.hs_hash256_record, L.hs_hash3_record):
        f.argtypes = [vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, ctypes.c_uint64,
                      ctypes.c_uint32, ctypes.c_int, vp]
        f.restype = ctypes.c_int
    return L


def _run(hs, alg, p: C.Packed, r: int, want: bool):
    fn = hs.hs_hash256_record if alg == C.SHA256 else hs.hs_hash3_record
    dig = np.full(32, 0xEE, np.uint8)
    off = p.off[r * p.nspan:(r + 1) * p.nspan].copy()
    ln = p.len[r * p.nspan:(r + 1) * p.nspan].copy()
    res = fn(p.data.ctypes.data, p.data_len, off.ctypes.data, ln.ctypes.data, p.nspan,
             int(p.want_off[r]), int(p.want_len[r]), int(p.want_kind[r]) if want else -1,
             dig.ctypes.data)
    return res, dig.tobytes()


@pytest.mark.parametrize("alg", [C.SHA256, C.SHA3_256])
@pytest.mark.parametrize("nspan", [1, 2, 3])
def test_harness_sweep(hs, alg, nspan):
    """Every length x seam of the sweep, spans at rotating alignments: digest
    against hashlib, and the digest compared with itself (RAW)."""
    cases = C.sweep(nspan)
    h = C.hashfn(alg)
    for align in range(4) if nspan == 1 else [0, 2]:
        recs = [(parts, h(m).digest(), C.RAW) for parts, m in cases]
        p = C.Packed(recs, nspan, align)
        for r, (parts, m) in enumerate(cases):
            res, dig = _run(hs, alg, p, r, True)
            assert dig == h(m).digest(), (alg, nspan, align, [len(x) for x in parts])
            assert res == C.MATCH


@pytest.mark.parametrize("alg", [C.SHA256, C.SHA3_256])
def test_harness_pointer_alignment(hs, alg):
    """The dword path at every pointer alignment of each span (0..3), at
    lengths with whole blocks inside every span."""
    h = C.hashfn(alg)
    for length in (64, 136, 200, 300, 513, 4097):
        m = C.message(length, 1)
        for a in range(4):
            for cut in ((length,), (length // 2, length - length // 2),
                        (length // 3, length // 3, length - 2 * (length // 3))):
                parts, at = [], 0
                for c in cut:
                    parts.append(m[at:at + c])
                    at += c
                p = C.Packed([(parts, None, 0)], len(cut), a, with_want=False)
                res, dig = _run(hs, alg, p, 0, False)
                assert (res, dig) == (C.MATCH, h(m).digest())


@pytest.mark.parametrize("alg", [C.SHA256, C.SHA3_256])
def test_harness_compare(hs, alg):
    """RAW and HEX comparisons: upper-case hex, want_len 63 / 65 / 31 / 33, one
    flipped bit, the wrong kind for the bytes, an unknown kind."""
    for salt in range(8):
        m = C.message(100 + salt, salt)
        cases = C.compare_cases(alg, m)
        assert any(k == C.HEX and w != w.lower() for w, k, _ in cases) or salt
        p = C.Packed([([m[:40], m[40:]], w, k) for w, k, _ in cases], 2, salt)
        for r, (w, k, expect) in enumerate(cases):
            res, dig = _run(hs, alg, p, r, True)
            assert dig == C.hashfn(alg)(m).digest()
            assert res == expect, (alg, k, len(w))


@pytest.mark.parametrize("alg", [C.SHA256, C.SHA3_256])
def test_harness_range_guard(hs, alg):
    m = C.message(50)
    d = C.hashfn(alg)(m).digest()
    p = C.Packed([([m[:20], m[20:], b""], d, C.RAW)], 3)
    n = p.data_len
    res, dig = _run(hs, alg, p, 0, True)
    assert (res, dig) == (C.MATCH, d)

    def with_span(k, off, ln, want=None):
        q = C.Packed([([m[:20], m[20:], b""], d, C.RAW)], 3)
        if want is None:
            q.off[k], q.len[k] = off, ln
        else:
            q.want_off[0], q.want_len[0] = want
        return _run(hs, alg, q, 0, True)
    for k in range(3):
        for off, ln in ((n - 1, 2), (n, 1), (n + 1, 0), (2**64 - 1, 2), (2**64 - 1, 0),
                        (0, n + 1), (1, 0xFFFFFFFF)):
            assert with_span(k, off, ln) == (C.RANGE, b"\0" * 32), (k, off, ln)
    for want in ((n - 31, 32), (2**64 - 16, 32), (n + 1, 0)):
        assert with_span(0, 0, 0, want) == (C.RANGE, b"\0" * 32)
    # the last byte of the buffer, and an empty span at its end, are in range
    q = C.Packed([([m[:20], m[20:], b""], d, C.RAW)], 3)
    q.off[2], q.len[2] = n, 0
    assert _run(hs, alg, q, 0, True) == (C.MATCH, d)


def test_golden_txid_vector(hs):
    """protoutil/txutils_test.go:543-571: ComputeTxID("nonce", "creator")."""
    with open(os.path.join(ROOT, "tests", "golden", "txid_vectors.json")) as f:
        vecs = json.load(f)["vectors"]
    assert vecs
    for v in vecs:
        nonce, creator, txid = v["nonce"].encode(), v["creator"].encode(), v["txid"].encode()
        assert hashlib.sha256(nonce + creator).hexdigest().encode() == txid
        for want, expect in ((txid, C.MATCH), (txid.upper(), C.MISMATCH), (txid[:63], C.MISMATCH)):
            p = C.Packed([([nonce, creator, b""], want, C.HEX)], 3)
            res, dig = _run(hs, C.SHA256, p, 0, True)
            assert (res, dig) == (expect, bytes.fromhex(txid.decode()))


# ---------------------------------------------------------------- the C ABI's checks
def _hbatch(p: C.Packed, **kw):
    f = dict(data=p.data.ctypes.data, data_len=p.data_len, off=p.off.ctypes.data,
             len=p.len.ctypes.data, nspan=p.nspan, want_off=p.want_off.ctypes.data,
             want_len=p.want_len.ctypes.data, want_kind=p.want_kind.ctypes.data)
    f.update(kw)
    return _lib.BhHBatch(f["data"], f["data_len"], f["off"], f["len"], f["nspan"], f["want_off"],
                         f["want_len"], f["want_kind"])


def test_bh_hash_argument_checks():
    """Every check of the header's list: BH_E_INVALID with a text, before any
    device work (none of this needs a device)."""
    L = _lib.lib()
    m = C.message(80)
    p = C.Packed([([m[:10], m[10:]], hashlib.sha256(m).digest(), C.RAW)] * 3, 2)
    dig, res = np.zeros(96, np.uint8), np.zeros(3, np.uint8)
    D, R_ = dig.ctypes.data, res.ctypes.data
    before = _lib.device_stats()
    none3 = dict(want_off=None, want_len=None, want_kind=None)
    far = C.Packed([([m[:10], m[10:]], None, 0)] * 3, 2)
    far.off[3], far.len[3] = p.data_len - 1, 2
    wrap = C.Packed([([m[:10], m[10:]], None, 0)] * 3, 2)
    wrap.off[5], wrap.len[5] = 2**64 - 1, 2
    wfar = C.Packed([([m[:10], m[10:]], None, 0)] * 3, 2)
    wfar.want_off[2], wfar.want_len[2] = 2**64 - 8, 32
    bad = [
        ("alg 0", 0, _hbatch(p), D, R_), ("alg 3", 3, _hbatch(p), D, R_),
        ("nspan 0", 1, _hbatch(p, nspan=0), D, R_), ("nspan 4", 1, _hbatch(p, nspan=4), D, R_),
        ("batch", 1, None, D, R_),
        ("data", 1, _hbatch(p, data=None), D, R_), ("off", 1, _hbatch(p, off=None), D, R_),
        ("len", 1, _hbatch(p, len=None), D, R_),
        ("no output", 1, _hbatch(p), None, None),
        ("want_off only missing", 1, _hbatch(p, want_off=None), D, R_),
        ("want_len only missing", 1, _hbatch(p, want_len=None), D, R_),
        ("want_kind only missing", 1, _hbatch(p, want_kind=None), D, R_),
        ("only want_kind", 1, _hbatch(p, want_off=None, want_len=None), D, None),
        ("result without want", 1, _hbatch(p, **none3), D, R_),
        ("span beyond", 1, _hbatch(far), D, R_), ("span wraps", 1, _hbatch(wrap), D, R_),
        ("want beyond", 1, _hbatch(wfar), D, R_),
    ]
    for name, alg, b, d, r in bad:
        ref = ctypes.byref(b) if b is not None else None
        for call in ("bh_hash", "bh_hash_submit"):
            job = ctypes.c_void_p()
            rc = (L.bh_hash(alg, ref, 3, d, r) if call == "bh_hash"
                  else L.bh_hash_submit(alg, ref, 3, d, r, ctypes.byref(job)))
            assert rc == _lib.BH_E_INVALID, (call, name, rc)
            assert _lib.last_error(), (call, name)
            assert not job.value
    # bh_hash_dev checks what it can see (not the arrays)
    for name, alg, b, d, r in bad[:14]:
        ref = ctypes.byref(b) if b is not None else None
        assert L.bh_hash_dev(0, alg, ref, 3, d, r, None, 1) == _lib.BH_E_INVALID, name
        assert _lib.last_error()
    assert L.bh_hash_submit(1, ctypes.byref(_hbatch(p)), 3, D, R_, None) == _lib.BH_E_INVALID
    assert _lib.device_stats() == before


# ---------------------------------------------------------------- the block path's decode
CLASSES = F.HASH_CLASSES + ["none", "creator_sig_flip", "two_actions", "epoch", "payload_garbage"]


@pytest.fixture(scope="module")
def hash_block():
    return F.generate_fabric_block(ntx=len(CLASSES), corrupt_den=0, classes=CLASSES, seed=7)


def _orc_verify(x, y, msg, sig):
    from oracle import orc
    return orc.csp_verify(x.to_bytes(32, "big") + y.to_bytes(32, "big"), sig,
                          hashlib.sha256(msg).digest())


def _tx(t):
    return (t.status, t.type, t.creator, t.endorse, t.valid_endorsers)


def _real_blocks():
    with open(os.path.join(ROOT, "tests", "golden", "real_blocks.json")) as f:
        return {k: bytes.fromhex(v["hex"]) for k, v in json.load(f)["blocks"].items()}


def _check_decode_only(block):
    want_txs, want_cr, want_en = fabric.block_preverify_refs(block, decode_only=True)
    txs, cr, en, hashes = fabric.block_prevalidate(block, decode_only=True)
    assert [_tx(t) for t in txs] == [_tx(t) for t in want_txs]
    assert cr == want_cr and en == want_en
    go = U.go_checks(block)
    assert len(go) == len(hashes)
    for g, h in zip(go, hashes):
        assert h.spans == g.spans
        assert (h.txid, h.proposal_hash) == (U.NOT_CHECKED, U.NOT_CHECKED)
    return go


def test_prevalidate_decode_only_classes(hash_block):
    go = _check_decode_only(hash_block.block)
    # the spans are the inputs: hashing them gives the construction's verdicts
    assert sum(1 for g in go if g.spans["ccpp"][1]) >= 10


def test_prevalidate_decode_only_real_blocks():
    blocks = _real_blocks()
    assert len(blocks) >= 5
    for block in blocks.values():
        _check_decode_only(block)


def test_oracle_matches_construction(hash_block):
    """tests/txhash_util.py's restatement of the Go checks against what the
    generator built: oracle against construction, no library involved."""
    fb = hash_block
    go = U.go_checks(fb.block, _orc_verify)
    assert [g.status for g in go] == fb.tx_status
    assert [g.status_full for g in go] == fb.tx_status_full
    assert [(g.txid, g.proposal_hash) for g in go] == fb.tx_hash
    by = dict(zip(fb.tx_class, fb.tx_status_full))
    assert by["txid_and_phash_wrong"] == U.FAB_TXID and by["txid_wrong_two_actions"] == U.FAB_TXID
    assert by["ccpp_empty"] == by["ccpp_absent"] == F.FAB_TX
    assert by["phash_absent"] == by["phash_long"] == U.FAB_PROPOSAL_HASH
    assert by["txid_upper"] == U.FAB_TXID and by["none"] == F.FAB_OK


def test_default_block_unchanged():
    """HASH_CLASSES are reachable only through classes=: the default block
    (the benchmark's) is byte-identical to what it was before they existed."""
    fb = F.generate_fabric_block()
    assert hashlib.sha256(fb.block).hexdigest() == \
        "2f3925b6415a16b927c210ecf09242f30de9db939727a73eeb0222cdad0d6c97"
    assert not set(fb.tx_class) & set(F.HASH_CLASSES)
    assert fb.tx_status_full == fb.tx_status  # nothing of it fails a hash check
