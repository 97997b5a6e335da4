"""bh_hash / bh_hash_dev / bh_hash_submit, CSP.batch_hash and
bh_fabric_block_prevalidate on the device, against hashlib and the restatement
of the two Go checks (tests/txhash_util.py)."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

from bdls_amd import _lib, fabric
from bdls_amd.workload import fabric as F
from tests import hash_cases as C
from tests import txhash_util as U
from tests.conftest import pack

pytestmark = pytest.mark.gpu

ALGS = [C.SHA256, C.SHA3_256]


def _hbatch(p: C.Packed, ptr=lambda a: a.ctypes.data, want=True):
    return _lib.BhHBatch(ptr(p.data), p.data_len, ptr(p.off), ptr(p.len), p.nspan,
                         ptr(p.want_off) if want else None, ptr(p.want_len) if want else None,
                         ptr(p.want_kind) if want else None)


def host_hash(alg, p: C.Packed, digest=True, result=True, submit=False):
    """bh_hash (or bh_hash_submit + a wait function) over p."""
    _lib.ensure_init()
    L = _lib.lib()
    dig = np.full(max(1, p.n) * 32, 0xEE, np.uint8) if digest else None
    res = np.full(max(1, p.n), 0xEE, np.uint8) if result else None
    b = _hbatch(p, want=p.with_want)
    args = (alg, ctypes.byref(b), p.n, dig.ctypes.data if digest else None,
            res.ctypes.data if result else None)

    def out():
        return (dig[:p.n * 32].reshape(p.n, 32) if digest else None,
                res[:p.n] if result else None)
    if not submit:
        _lib.check(L.bh_hash(*args))
        return out()
    job = ctypes.c_void_p()
    _lib.check(L.bh_hash_submit(*args, ctypes.byref(job)))

    def wait(keep=(b, p)):
        _lib.check(L.bh_verify_wait(job))
        return out()
    return wait


def dev_hash(alg, p: C.Packed, digest=True, result=True):
    """bh_hash_dev over p made resident."""
    _lib.ensure_init()
    arrs = {}

    def up(a):
        d = _lib.DeviceArray.from_numpy(0, a)
        arrs[id(a)] = d
        return d.ptr
    b = _hbatch(p, ptr=up, want=p.with_want)
    dig = _lib.DeviceArray(0, max(1, p.n) * 32) if digest else None
    res = _lib.DeviceArray(0, max(1, p.n)) if result else None
    _lib.check(_lib.lib().bh_hash_dev(0, alg, ctypes.byref(b), p.n, dig.ptr if digest else None,
                                      res.ptr if result else None, None, 1))
    return (dig.to_numpy(np.uint8, p.n * 32).reshape(p.n, 32) if digest else None,
            res.to_numpy(np.uint8, p.n) if result else None)


def _want_digests(alg, recs):
    h = C.hashfn(alg)
    return np.frombuffer(b"".join(h(b"".join(parts)).digest() for parts, _, _ in recs),
                         np.uint8).reshape(len(recs), 32)


def _sweep_records(alg, nspan):
    """The CPU sweep's records; the expected span cycles through the compare
    cases of each record's digest."""
    recs, expect = [], []
    for r, (parts, m) in enumerate(C.sweep(nspan)):
        cases = C.compare_cases(alg, m)
        w, k, e = cases[r % len(cases)]
        recs.append((parts, w, k))
        expect.append(e)
    return recs, np.array(expect, np.uint8)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("nspan", [1, 2, 3])
def test_length_set(alg, nspan):
    """The CPU sweep's length x seam set as one batch, through bh_hash and
    bh_hash_dev; a hash job counts as one device batch."""
    recs, expect = _sweep_records(alg, nspan)
    p = C.Packed(recs, nspan, align=nspan)
    want = _want_digests(alg, recs)
    _lib.ensure_init()
    b0 = _lib.device_stats()
    dig, res = host_hash(alg, p)
    b1 = _lib.device_stats()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (1, p.n)
    assert (dig == want).all()
    assert (res == expect).all()
    assert set(expect) == {C.MATCH, C.MISMATCH}
    dig, res = dev_hash(alg, p)
    assert (dig == want).all()
    assert (res == expect).all()


@pytest.mark.parametrize("alg", ALGS)
def test_group_and_block_edges(alg):
    """n = 1, 3, 4, 5, 9, 33, 130: a partial lane group, a partial wave and a
    partial workgroup of both kernels; neighbours of very different lengths."""
    lens = [0, 55, 56, 64, 119, 120, 1, 300, 135, 136, 137, 1024, 7, 4097, 63, 271, 272]
    for n in (1, 3, 4, 5, 9, 33, 130):
        recs = []
        for r in range(n):
            m = C.message(lens[(r + n) % len(lens)], r)
            a, b = len(m) // 3, len(m) // 2
            d = C.hashfn(alg)(m).digest()
            recs.append(([m[:a], m[a:b], m[b:]], d.hex().encode() if r % 2 else d,
                         C.HEX if r % 2 else C.RAW))
        p = C.Packed(recs, 3, align=n)
        want = _want_digests(alg, recs)
        for fn in (host_hash, dev_hash):
            dig, res = fn(alg, p)
            assert (dig == want).all(), (n, fn.__name__)
            assert (res == C.MATCH).all(), (n, fn.__name__)


@pytest.mark.parametrize("alg", ALGS)
def test_long_record(alg):
    """One record of 40 SHA-256 blocks (more than two rounds of the lane
    group), alone and between short neighbours; 41 blocks beside it."""
    long40, long41 = C.message(40 * 64 - 9, 40), C.message(40 * 64 - 8, 41)
    for msgs in ([long40], [b"abc", long40, b"", long41, b"xyz"]):
        recs = [([m[:100], m[100:]], C.hashfn(alg)(m).digest(), C.RAW) for m in msgs]
        p = C.Packed(recs, 2)
        for fn in (host_hash, dev_hash):
            dig, res = fn(alg, p)
            assert (dig == _want_digests(alg, recs)).all()
            assert (res == C.MATCH).all()


@pytest.mark.parametrize("alg", ALGS)
def test_output_combinations(alg):
    recs, expect = _sweep_records(alg, 2)
    recs, expect = recs[::37], expect[::37]
    p = C.Packed(recs, 2)
    want = _want_digests(alg, recs)
    for fn in (host_hash, dev_hash):
        dig, res = fn(alg, p, digest=True, result=False)
        assert res is None and (dig == want).all()
        dig, res = fn(alg, p, digest=False, result=True)
        assert dig is None and (res == expect).all()
        dig, res = fn(alg, p)
        assert (dig == want).all() and (res == expect).all()
    # digests alone need no expected spans at all
    q = C.Packed(recs, 2, with_want=False)
    for fn in (host_hash, dev_hash):
        dig, _ = fn(alg, q, result=False)
        assert (dig == want).all()


@pytest.mark.parametrize("alg", ALGS)
def test_range_guard_dev(alg):
    """bh_hash_dev cannot see the arrays: a span or an expected span beyond
    data_len is BH_HASH_RANGE with a zero digest, its neighbours unaffected.
    (The bad records read nothing: the kernel tests the range before it forms
    an address.)"""
    msgs = [C.message(70 + i, i) for i in range(7)]
    recs = [([m[:30], m[30:], b""], C.hashfn(alg)(m).digest(), C.RAW) for m in msgs]
    p = C.Packed(recs, 3)
    n = p.data_len
    p.off[1 * 3 + 1], p.len[1 * 3 + 1] = n - 1, 2         # ends one byte beyond
    p.off[3 * 3 + 0], p.len[3 * 3 + 0] = 2**64 - 1, 2     # the sum would wrap
    p.want_off[5], p.want_len[5] = n - 31, 32             # the expected span
    dig, res = dev_hash(alg, p)
    want = _want_digests(alg, recs)
    for r in range(7):
        if r in (1, 3, 5):
            assert res[r] == C.RANGE and not dig[r].any()
        else:
            assert res[r] == C.MATCH and (dig[r] == want[r]).all()
    # the host form refuses the same batch before any device work
    b0 = _lib.device_stats()
    with pytest.raises(_lib.EngineError):
        host_hash(alg, p)
    assert _lib.device_stats() == b0


def test_submit_overlaps_verify(golden):
    """A hash job submitted before a bh_verify of 256 records runs on its own
    stream and is collected afterwards; both results are what they are alone."""
    from bdls_amd.bccsp import verify_packed
    recs = [golden[i % len(golden)] for i in range(256)]
    packed = pack(recs, False)
    valid0, reason0 = verify_packed(*packed)
    hrecs, expect = _sweep_records(C.SHA256, 3)
    p = C.Packed(hrecs, 3)
    wait = host_hash(C.SHA256, p, submit=True)
    wait2 = host_hash(C.SHA3_256, C.Packed(hrecs[:50], 3), digest=True, result=False, submit=True)
    valid, reason = verify_packed(*packed)
    assert (valid == valid0).all() and (reason == reason0).all()
    dig, res = wait()
    assert (dig == _want_digests(C.SHA256, hrecs)).all() and (res == expect).all()
    dig2, _ = wait2()
    assert (dig2 == _want_digests(C.SHA3_256, hrecs[:50])).all()
    # three jobs in flight on two slots: the third collects the first's slot
    waits = [host_hash(C.SHA256, C.Packed(hrecs[k::500], 3), submit=True) for k in range(3)]
    for k, w in reversed(list(enumerate(waits))):
        dig, res = w()
        assert (dig == _want_digests(C.SHA256, hrecs[k::500])).all()
        assert (res == expect[k::500]).all()


def test_csp_batch_hash():
    from bdls_amd.bccsp import HipCSP, SHA3_256Opts
    csp = HipCSP()
    msgs = [C.message(n, 3) for n in (0, 1, 55, 56, 64, 135, 136, 137, 1000, 4097)]
    assert csp.batch_hash(msgs) == [hashlib.sha256(m).digest() for m in msgs]
    assert csp.batch_hash(msgs, SHA3_256Opts()) == [hashlib.sha3_256(m).digest() for m in msgs]
    assert csp.batch_hash([]) == []
    assert csp.batch_hash(msgs[:1]) == [csp.hash(msgs[0])]


# ---------------------------------------------------------------- the block path
CLASSES = F.HASH_CLASSES + ["none", "creator_sig_flip", "two_actions", "epoch", "payload_garbage"]


@pytest.fixture(scope="module")
def hash_block():
    return F.generate_fabric_block(ntx=len(CLASSES), corrupt_den=0, classes=CLASSES, seed=7)


@pytest.fixture(scope="module")
def hash_block_p384():
    return F.generate_fabric_block(ntx=len(CLASSES), corrupt_den=0, classes=CLASSES, seed=7,
                                   p384_orgs=1)


def _tx(t):
    return (t.type, t.creator, t.endorse, t.valid_endorsers)


def _check_block(fb, **kw):
    """block_prevalidate against construction and against the old call."""
    old_txs, old_cr, old_en = fabric.block_preverify_refs(fb.block, **kw)
    txs, cr, en, hashes = fabric.block_prevalidate(fb.block, **kw)
    assert [_tx(t) for t in txs] == [_tx(t) for t in old_txs]
    assert cr == old_cr and en == old_en
    assert [(h.txid, h.proposal_hash) for h in hashes] == fb.tx_hash
    go = U.go_checks(fb.block)
    assert [h.spans for h in hashes] == [g.spans for g in go]
    assert [(g.txid, g.proposal_hash) for g in go] == fb.tx_hash
    return txs, old_txs


def test_prevalidate_classes(hash_block):
    txs, old = _check_block(hash_block)
    assert [t.status for t in old] == hash_block.tx_status
    assert [t.status for t in txs] == hash_block.tx_status_full
    assert {U.FAB_TXID, U.FAB_PROPOSAL_HASH, F.FAB_TX, F.FAB_OK} <= {t.status for t in txs}


def test_prevalidate_classes_sha3(hash_block):
    """BH_FAB_F_SHA3 changes the signatures' family only: ComputeTxID and
    GetProposalHash2 are hard-wired to crypto/sha256, so hashes[] does not
    move. The block's signatures were made over SHA-256 digests, so under the
    SHA3 family every creator signature fails, and that check comes first in
    Go's order: the statuses are the old call's."""
    txs, old = _check_block(hash_block, sha3=True)
    assert [t.status for t in txs] == [t.status for t in old]
    assert all(t.status in (F.FAB_CREATOR_SIGNATURE, F.FAB_HEADER, F.FAB_PAYLOAD) for t in txs)


def test_prevalidate_classes_mixed_route(hash_block_p384):
    fb = hash_block_p384
    assert fb.p384_keys
    txs, old = _check_block(fb)
    assert [t.status for t in old] == fb.tx_status
    assert [t.status for t in txs] == fb.tx_status_full


@pytest.fixture(scope="module")
def block64():
    return F.generate_fabric_block(ntx=64)


def test_prevalidate_block64(block64):
    fb = block64
    txs, _ = _check_block(fb)
    assert [t.status for t in txs] == fb.tx_status_full
    hashes = fabric.block_prevalidate(fb.block)[3]
    n = 0
    for cls, h in zip(fb.tx_class, hashes):
        if cls == "none":
            assert (h.txid, h.proposal_hash) == (U.MATCH, U.MATCH)
            n += 1
    assert n >= 32


def test_prevalidate_concurrent(hash_block, hash_block_p384, block64):
    """Four threads, five calls each, on different block buffers: what the
    serial calls give."""
    blocks = [hash_block, hash_block_p384, block64, hash_block]

    def run(fb):
        txs, cr, en, hashes = fabric.block_prevalidate(fb.block)
        return ([(t.status,) + _tx(t) for t in txs], cr, en,
                [(h.txid, h.proposal_hash, h.spans) for h in hashes])
    serial = [run(fb) for fb in blocks]
    got = [[None] * 5 for _ in blocks]
    errs = []

    def worker(k):
        try:
            for j in range(5):
                got[k][j] = run(blocks[k])
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for k in range(4):
        for j in range(5):
            assert got[k][j] == serial[k]
