"""Span records for the tests of bh_hash: the length / seam / alignment sweep
shared by the host-harness test (one record per call) and the GPU tests (the
same records as batches), and the packer that lays records out in one data
buffer the way a caller would index a block."""
from __future__ import annotations

import hashlib

import numpy as np

SHA256, SHA3_256 = 1, 2
RAW, HEX = 0, 1
MATCH, MISMATCH, RANGE = 0, 1, 2

# total message lengths: every padding case of both block sizes (64 and 136),
# the boundaries of 8 and 16 blocks (one and two rounds of the lane group)
LENGTHS = list(range(301)) + [511, 512, 513, 1015, 1016, 1023, 1024, 1025, 4096, 4097]


def hashfn(alg):
    return hashlib.sha256 if alg == SHA256 else hashlib.sha3_256


def message(length: int, salt: int = 0) -> bytes:
    return hashlib.shake_128(b"bh_hash %d %d" % (length, salt)).digest(length)


def splits(length: int, nspan: int) -> list[tuple]:
    """Span lengths of a message of `length` bytes cut into nspan spans: seams
    at 0, 1, 63, 64, 65 and the end; with three spans also two seams inside
    one block, both at one point, and a whole block between them."""
    if nspan == 1:
        return [(length,)]
    if nspan == 2:
        seams = sorted({s for s in (0, 1, 63, 64, 65, length) if s <= length})
        return [(s, length - s) for s in seams]
    pairs = [(0, 0), (0, 1), (0, length), (length, length), (1, 2), (3, 60), (63, 65), (64, 64),
             (64, 128), (65, 70), (1, length)]
    pairs = sorted({p for p in pairs if p[0] <= p[1] <= length})
    return [(a, b - a, length - b) for a, b in pairs]


def sweep(nspan: int):
    """[(parts, message)] over LENGTHS x splits."""
    out = []
    for length in LENGTHS:
        m = message(length)
        for cut in splits(length, nspan):
            parts, at = [], 0
            for c in cut:
                parts.append(m[at:at + c])
                at += c
            out.append((parts, m))
    return out


class Packed:
    """Records [(parts, want bytes or None, kind)] laid out in one buffer:
    spans out of message order, filler between them, and span k of record r at
    an address whose alignment is (align + r + k) % 4."""

    def __init__(self, records, nspan: int, align: int = 0, with_want: bool = True):
        buf = bytearray(b"\xA5" * 8)
        n = len(records)
        self.n, self.nspan = n, nspan
        self.off = np.zeros(n * nspan, np.uint64)
        self.len = np.zeros(n * nspan, np.uint32)
        self.want_off = np.zeros(max(1, n), np.uint64)
        self.want_len = np.zeros(max(1, n), np.uint32)
        self.want_kind = np.zeros(max(1, n), np.uint8)
        self.with_want = with_want

        def place(b: bytes, a: int) -> int:
            while len(buf) % 4 != a % 4:
                buf.append(0xA5)
            at = len(buf)
            buf.extend(b)
            buf.append(0x5A)
            return at
        for r, (parts, want, kind) in enumerate(records):
            assert len(parts) == nspan
            for k in reversed(range(nspan)):
                self.off[r * nspan + k] = place(parts[k], align + r + k)
                self.len[r * nspan + k] = len(parts[k])
            if with_want:
                self.want_off[r] = place(want or b"", align + r + 3)
                self.want_len[r] = len(want or b"")
                self.want_kind[r] = kind
        self.data_len = len(buf)
        # the buffer itself at a 4-byte aligned address (numpy allocations are)
        self.data = np.frombuffer(bytes(buf) + b"\0" * 8, np.uint8).copy()
        assert self.data.ctypes.data % 4 == 0


def compare_cases(alg: int, msg: bytes):
    """[(want, kind, expected result)] for the digest of msg."""
    d = hashfn(alg)(msg).digest()
    hx = d.hex().encode()
    flip = bytes([d[0] ^ 1]) + d[1:]
    bad_hex = (b"1" if hx[:1] == b"0" else b"0") + hx[1:]
    out = [(d, RAW, MATCH), (hx, HEX, MATCH), (flip, RAW, MISMATCH), (bad_hex, HEX, MISMATCH),
           (d[:31], RAW, MISMATCH), (d + b"\0", RAW, MISMATCH), (hx[:63], HEX, MISMATCH),
           (hx + b"0", HEX, MISMATCH), (b"", RAW, MISMATCH), (b"", HEX, MISMATCH),
           (d, HEX, MISMATCH), (hx, RAW, MISMATCH), (d, 7, MISMATCH),
           (d[:-1] + bytes([d[-1] ^ 0x80]), RAW, MISMATCH)]
    if hx.upper() != hx:
        out.append((hx.upper(), HEX, MISMATCH))
    return out
