"""CPU: the batches, expectations and plans of tests/test_resident_passes_gpu.py
(tests/resident_util.py) are built and put to the oracle here, so a slip in a
helper does not wait for a GPU run. No device code runs."""
import json

import numpy as np

from oracle import ecdsa_ref as O
from tests import resident_util as R


def test_batches_and_spot_checks():
    """Every batch the GPU module runs: sizes, one record in eight corrupted,
    and (inside the builders) the oracle on every corrupted record and every
    16th other one, with and without the low-S rule where both are used."""
    recs, want, nls = R.golden384()
    assert len(recs) == len(want) == len(nls) and (want != nls).any()
    for fam in ("SHA2", "SHA3"):
        frecs, fwant = R.p384_fused(fam)
        assert len(frecs) == len(fwant) == 200 and set(fwant.tolist()) == {0, 6, 7, 9}
    for curve, h, n in (("P-384", "SHA384", 200), ("P-384", "SHA512", 200),
                        ("P-256", "SHA512", 200), ("P-256", "SHA384", 257),
                        ("P-256", "SHA512", 257)):
        wrecs, wwant, wnls = R.wide_batch(curve, h, n)
        assert len(wrecs) == n and set(wwant.tolist()) == {0, 6, 7, 9}
        # a high-S record is a valid signature without the rule, nothing else differs
        assert ((wwant != wnls) == (wwant == O.R_HIGH_S)).all() and (wnls[wwant == 6] == 0).all()
        lens = {len(r["msg"]) // 2 for r in wrecs[:64]}
        assert lens == set(R.W.EDGE_LENS)  # every pass of 64 hashes every padding edge
        assert R.count_math(wwant) == n - int(np.isin(wwant, (6, 7)).sum())


def test_plans_are_complete_and_serialisable():
    """Each call of a plan has its expectation, the prefixes cross the pass
    boundaries, and a plan survives the JSON file the child reads."""
    n = len(R.golden384()[0])
    batches, ops, expect = R.plan_p384()
    ids = [op["id"] for op in ops if op["op"] == "dev"]
    assert len(ids) == len(set(ids)) == 2 * 6 * 2 + 4
    assert {op["n"] for op in ops if op["op"] == "dev" and op["mode"] == "digest"} == \
        {1, 64, 65, 128, 129, n}
    assert set(expect) == set(ids) | {"async/0", "async/1"}
    assert (expect["async/1"][1] == expect["async/0"][1][::-1]).all()
    assert batches["golden_rev"][0] == batches["golden"][-1]
    wb, wops, wexpect = R.plan_wide()
    assert set(wexpect) == {op["id"] for op in wops} and len(wops) == 2 * 2 * 2 + 1
    for b, o in ((batches, ops), (wb, wops)):
        back = json.loads(json.dumps({"batches": b, "ops": o}))
        used = {op["batch"] for op in o if "batch" in op} | \
            {x for op in o for x in op.get("batches", [])}
        assert back["ops"] == o and set(back["batches"]) == used
    for arrs in (R.pack(batches["golden"], "digest"), R.pack(wb["P256"], "msg")):
        pub, sig, so, sl, msg, mo, ml = arrs
        assert so.dtype == mo.dtype == np.uint64 and sl.dtype == ml.dtype == np.uint32
        assert int(so[-1] + sl[-1]) == len(sig) - 1 and int(mo[-1] + ml[-1]) == len(msg) - 1


def test_result_check_catches_each_kind_of_damage():
    """check_result on made-up results: a wrong reason, a wrong bit, a touched
    guard word and a touched guard byte each fail it; the clean result passes."""
    want = np.array([0, 9, 0, 6] * 17, np.uint8)[:65]
    words = [int(np.packbits(want[:64] == 0, bitorder="little").view(np.uint64)[0]), 1]
    good = {"reason": want.tolist(), "words": words, "guard_word": R.GUARD_WORD,
            "guard_bytes": [R.GUARD]}
    R.check_result(good, 65, want)
    assert (R.bits_of(words, 65) == (want == 0)).all()
    for damage in ({"reason": [9] + want.tolist()[1:]}, {"words": [words[0] ^ 2, 1]},
                   {"words": [words[0], 0]}, {"guard_word": 0}, {"guard_bytes": [0, R.GUARD]},
                   {"words": words[:1]}):
        try:
            R.check_result(dict(good, **damage), 65, want)
        except AssertionError:
            continue
        raise AssertionError(f"not caught: {damage}")
