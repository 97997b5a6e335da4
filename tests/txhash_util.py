"""The two SHA-256 checks ValidateTransaction makes of an endorser transaction,
restated from the Go code for the tests of bh_hash / bh_fabric_block_prevalidate.
Decodes with oracle.fabric_ref and hashes with hashlib; never calls the library.

  protoutil.CheckTxID (core/common/validation/msgvalidation.go:288-296,
  protoutil/proputils.go:351-370):
      hex.EncodeToString(sha256(nonce || creator)) == ChannelHeader.tx_id
  the proposal hash (msgvalidation.go:228-241, protoutil/txutils.go:449-466):
      GetProposalHash2 -> "nil arguments" if chaincode_proposal_payload is nil
      (absent, or present with length 0: protobuf-go's proto3 bytes decoder
      stores append([]byte(nil), v...)), else
      sha256(channel_header || actions[0].header || chaincode_proposal_payload)
      must equal ProposalResponsePayload.proposal_hash (bytes.Equal).
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field

from oracle import fabric_ref as R

MATCH, MISMATCH, NOT_CHECKED = 0, 1, 0xFF
FAB_TXID, FAB_PROPOSAL_HASH = 8, 9
SPANS = ("nonce", "creator", "txid", "chdr", "ashdr", "ccpp", "phash")


def _bytes_fields(b: bytes, base: int):
    """(num, offset in the block, length) of every length-delimited field of
    message b, which starts at block offset `base` (b decodes: the caller
    decoded it with fabric_ref first)."""
    i = 0
    while i < len(b):
        tag, i = R.consume_varint(b, i)
        num, typ = tag >> 3, tag & 7
        if typ == 0:
            _, i = R.consume_varint(b, i)
        elif typ == 2:
            ln, j = R.consume_varint(b, i)
            yield num, base + j, ln
            i = j + ln
        else:
            i = R.consume_field_value(num, typ, b, i)


def _last(b: bytes, base: int, num: int):
    """The last occurrence of bytes field `num` (proto3: the last one wins):
    (offset, length), or None when absent."""
    out = None
    for n, off, ln in _bytes_fields(b, base):
        if n == num:
            out = (off, ln)
    return out


def _merged(b: bytes, base: int, num: int, sub: tuple):
    """Singular message field `num` of b, occurrences merged: for each bytes
    field of `sub`, its last occurrence over all occurrences of the message."""
    out = {s: None for s in sub}
    for n, off, ln in _bytes_fields(b, base):
        if n != num:
            continue
        for m, o2, l2 in _bytes_fields(b[off - base:off - base + ln], off):
            if m in out:
                out[m] = (o2, l2)
    return out


@dataclass
class GoTx:
    status: int            # the old call's status (fabric_ref.validate_block)
    status_full: int       # with BH_FAB_TXID / BH_FAB_PROPOSAL_HASH in Go's order
    txid: int = NOT_CHECKED
    proposal_hash: int = NOT_CHECKED
    spans: dict = field(default_factory=lambda: {s: (0, 0) for s in SPANS})


def go_checks(block: bytes, verify=None) -> list[GoTx]:
    """Per transaction of a serialized common.Block: the old call's status, the
    two checks, the new call's status and where the checks' inputs lie.
    verify as fabric_ref.validate_block takes it; None = decode only (the
    creator signatures count as valid)."""
    block = bytes(block)
    old = R.validate_block(block, verify, decode_only=verify is None)
    envs = []
    for n, off, ln in _bytes_fields(block, 0):
        if n == 2:
            envs += [(o, l) for m, o, l in _bytes_fields(block[off:off + ln], off) if m == 1]
    assert len(envs) == len(old)
    out = []
    for (eo, el), o in zip(envs, old):
        g = GoTx(o.status, o.status)
        out.append(g)
        if o.status in (R.ENVELOPE, R.PAYLOAD, R.HEADER):
            continue
        sp = lambda s: block[s[0]:s[0] + s[1]] if s else b""  # noqa: E731
        payload = _last(block[eo:eo + el], eo, 1)
        hdr = _merged(sp(payload), payload[0], 1, (1, 2))
        chdr, shdr = hdr[1], hdr[2]
        txid = _last(sp(chdr), chdr[0], 5)
        creator, nonce = _last(sp(shdr), shdr[0], 1), _last(sp(shdr), shdr[0], 2)
        put = lambda name, s: g.spans.__setitem__(name, s if s and s[1] else (0, 0))  # noqa: E731
        put("nonce", nonce)
        put("creator", creator)
        put("txid", txid)
        put("chdr", chdr)
        if o.type != 3:
            continue
        # CheckTxID
        want = hashlib.sha256(sp(nonce) + sp(creator)).hexdigest()
        g.txid = MATCH if sp(txid) == want.encode() else MISMATCH  # a string compare
        structure_ok = True
        ccpp = phash = ashdr = None
        try:
            pl = R.unmarshal(sp(payload), R.PAYLOAD_SPEC)
            tx = R.unmarshal(pl["data"] or b"", R.TRANSACTION_SPEC)
            if len(tx["actions"]) != 1:
                raise R.DecodeError("actions")
            act = tx["actions"][0]
            ash = R.unmarshal(act["header"] or b"", R.SIGNATURE_HEADER_SPEC)
            if not ash["nonce"] or not ash["creator"]:
                raise R.DecodeError("action header")
            cap = R.unmarshal(act["payload"] or b"", R.CC_ACTION_PAYLOAD_SPEC)
            if cap["action"] is None:
                raise R.DecodeError("nil action")
            R.unmarshal(cap["action"]["proposal_response_payload"] or b"", R.PRP_SPEC)
        except R.DecodeError:
            structure_ok = False
        if structure_ok:
            data = _last(sp(payload), payload[0], 2)
            action = [(a, b) for m, a, b in _bytes_fields(sp(data), data[0]) if m == 1][0]
            ashdr = _last(sp(action), action[0], 1)
            apl = _last(sp(action), action[0], 2)
            ccpp = _last(sp(apl), apl[0], 1)
            cea = _merged(sp(apl), apl[0], 2, (1,))
            prp = cea[1]
            phash = _last(sp(prp), prp[0], 1) if prp else None
            put("ashdr", ashdr)
            put("ccpp", ccpp)
            put("phash", phash)
            if sp(ccpp):  # a nil payload: GetProposalHash2 "nil arguments"
                h = hashlib.sha256(sp(chdr) + sp(ashdr) + sp(ccpp)).digest()
                g.proposal_hash = MATCH if h == sp(phash) else MISMATCH
        # the first failing check in Go's order, once the creator check passed
        if o.status in (R.OK, R.TX):
            if g.txid == MISMATCH:
                g.status_full = FAB_TXID
            elif o.status == R.OK and not sp(ccpp):
                g.status_full = R.TX
            elif o.status == R.OK and g.proposal_hash == MISMATCH:
                g.status_full = FAB_PROPOSAL_HASH
    return out
