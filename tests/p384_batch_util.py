"""Shared by tests/test_p384_batch_cpu.py and tests/test_p384_batch_gpu.py: the
layouts of the P-384 BatchVerify entry points (bh_verify384_compact: bh_cbatch
with 96-byte keys; bh_batch_verify384_ptrs: bh_pbatch) built from fixture
records, and thin callers."""
from __future__ import annotations

import ctypes
import random

import numpy as np

from bdls_amd import _lib
from tests import p384_util as U


def key_bytes(r) -> bytes:
    return bytes.fromhex(r["qx"] + r["qy"])


def fields(recs, fused):
    sigs = [bytes.fromhex(r["sig"]) for r in recs]
    msgs = [bytes.fromhex(r["msg"] if fused else r["digest"]) for r in recs]
    return sigs, msgs


def key_table(recs, seed=None, extra=()):
    """(table: list of 96-byte keys, idx: uint32 per record). The distinct keys
    in first-use order, then `extra` entries; seed: the table shuffled, the
    indices following."""
    table, where, idx = [], {}, []
    for r in recs:
        k = key_bytes(r)
        if k not in where:
            where[k] = len(table)
            table.append(k)
        idx.append(where[k])
    table += list(extra)
    if seed is not None:
        perm = list(range(len(table)))
        random.Random(seed).shuffle(perm)      # entry j moves to perm[j]
        moved = [None] * len(table)
        for j, p in enumerate(perm):
            moved[p] = table[j]
        table, idx = moved, [perm[j] for j in idx]
    return table, np.array(idx, np.uint32)


class Compact:
    """A bh_cbatch over numpy arrays it keeps alive."""

    def __init__(self, table, idx, sigs, msgs, stride=None):
        self.keys = np.frombuffer(b"".join(table) + b"\0", np.uint8).copy()
        self.idx = None if idx is None else np.ascontiguousarray(idx, np.uint32)
        self.sig, _, self.sig_len = U.pack_bytes(sigs)
        self.msg, _, self.msg_len = U.pack_bytes(msgs)
        if stride is not None:
            assert all(len(m) == stride for m in msgs)
            self.msg_len = None
        self.n = len(sigs)
        self.c = _lib.BhCBatch(
            self.keys.ctypes.data, None if self.idx is None else self.idx.ctypes.data, len(table),
            self.sig.ctypes.data, self.sig_len.ctypes.data, self.msg.ctypes.data,
            None if self.msg_len is None else self.msg_len.ctypes.data, stride or 0)


def compact(recs, fused, indexed=True, seed=None, extra=(), stride=None):
    sigs, msgs = fields(recs, fused)
    if indexed:
        table, idx = key_table(recs, seed, extra)
    else:
        table, idx = [key_bytes(r) for r in recs], None
    return Compact(table, idx, sigs, msgs, stride)


class Ptrs:
    """A bh_pbatch over per-record buffers it keeps alive (None: a NULL pointer)."""

    def __init__(self, keys, sigs, msgs):
        n = self.n = len(sigs)
        self.bufs = []

        def col(items, share=False):
            out, seen = np.zeros(max(n, 1), np.uint64), {}
            for i, b in enumerate(items):
                if b is None:
                    continue
                if share and b in seen:          # equal keys behind one pointer, sometimes
                    out[i] = seen[b]
                    continue
                a = np.frombuffer(bytes(b) + b"\0", np.uint8).copy()
                self.bufs.append(a)
                out[i] = a.ctypes.data
                if share and i % 2 == 0:
                    seen[b] = out[i]
            return out
        self.pub, self.sig, self.msg = col(keys, True), col(sigs), col(msgs)
        self.sig_len = np.array([len(s) if s is not None else 77 for s in sigs] or [0], np.uint32)
        self.msg_len = np.array([len(m) if m is not None else 77 for m in msgs] or [0], np.uint32)
        self.p = _lib.BhPBatch(self.pub.ctypes.data, self.sig.ctypes.data,
                               self.sig_len.ctypes.data, self.msg.ctypes.data,
                               self.msg_len.ctypes.data)

    def scribble(self):
        """Overwrite every caller-owned buffer (after a submit call has returned)."""
        for a in self.bufs:
            a[:] = 0xA5
        self.sig_len[:] = 3
        self.msg_len[:] = 5
        self.pub[:] = 0
        self.sig[:] = 0
        self.msg[:] = 0


def ptrs(recs, fused):
    sigs, msgs = fields(recs, fused)
    return Ptrs([key_bytes(r) for r in recs], sigs, msgs)


def outputs(n):
    return np.full((n + 7) // 8 + 1, 0xEE, np.uint8), np.full(n + 1, 0xEE, np.uint8)


def bits(bm, n):
    return np.unpackbits(bm[:(n + 7) // 8], bitorder="little")[:n].astype(bool)


def check_out(bm, rs, n):
    """Reasons and bits of a finished call; padding bits zero, nothing past the end."""
    nb = (n + 7) // 8
    assert bm[nb] == 0xEE and rs[n] == 0xEE
    if n % 8:
        assert bm[nb - 1] >> (n % 8) == 0
    return rs[:n].copy(), bits(bm, n)


def run_compact(L, cb, flags):
    bm, rs = outputs(cb.n)
    _lib.check(L.bh_verify384_compact(ctypes.byref(cb.c), cb.n, flags, bm.ctypes.data,
                                      rs.ctypes.data))
    return check_out(bm, rs, cb.n)


def run_ptrs(L, pb, flags):
    bm, rs = outputs(pb.n)
    _lib.check(L.bh_batch_verify384_ptrs(ctypes.byref(pb.p), pb.n, flags, bm.ctypes.data,
                                         rs.ctypes.data))
    return check_out(bm, rs, pb.n)


def run_expanded(L, recs, fused, flags):
    """bh_verify(BH_CURVE_P384) on the expanded batch: the reference of every parity test."""
    pub, sig, so, sl, msg, mo, ml = U.pack384(recs, fused)
    n = len(recs)
    b = _lib.BhBatch(pub.ctypes.data, sig.ctypes.data, so.ctypes.data, sl.ctypes.data,
                     msg.ctypes.data, mo.ctypes.data, ml.ctypes.data)
    bm, rs = outputs(n)
    _lib.check(L.bh_verify(_lib.BH_CURVE_P384, ctypes.byref(b), n, flags, bm.ctypes.data,
                           rs.ctypes.data))
    if n == 0:
        return rs[:0].copy(), bits(bm, 0)
    return check_out(bm, rs, n)
