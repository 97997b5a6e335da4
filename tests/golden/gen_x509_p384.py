"""Generate tests/golden/x509_p384_vectors.json: (certificate DER, issuer curve,
issuer public key, expected BH_R_* of CheckSignatureFrom) for bh_verify_x509_ex.

The reference holds no certificate signed with ecdsa-with-SHA384 / -SHA512 or
by a P-384 key, so the certificates are made here with the `openssl` command
line:
  * the chain an MSP with hardened CAs has: a P-384 root (-sha384), a P-384
    intermediate it signs, a P-256 leaf the intermediate signs (Go's
    x509.CreateCertificate, and fabric-ca with it, picks ecdsa-with-SHA384 for
    a P-384 signer), and further leaves of both curves under the intermediate;
  * one self-signed CA per remaining (issuer curve, hash) pairing, each with
    leaves of both curves, so all six pairings of {P-256, P-384} x {SHA-256,
    SHA-384, SHA-512} occur;
  * the mutations tests/golden/gen_x509.py applies, on one verifying link per
    pairing, plus ecdsa-with-SHA1 / -SHA224 algorithms, a key of the other
    curve offered for the link, and (P-384) an r of 49 significant bytes.
Expected results come from tests/sha2wide_util.py check_signature_from_ex
(Go 1.21 x509 + VerifyASN1 restated). Run from the repo root:
python tests/golden/gen_x509_p384.py
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ecdsa_ref as O  # noqa: E402
from oracle import x509_ref as X  # noqa: E402
from tests import sha2wide_util as W  # noqa: E402
from tests.golden.gen_x509 import pem_certs, rebuild, tlv  # noqa: E402

OUT = W.X509_P384
OSSL_CURVE = {"P-256": "prime256v1", "P-384": "secp384r1"}
OID_CURVE = {bytes.fromhex("2a8648ce3d030107"): "P-256", bytes.fromhex("2b81040022"): "P-384"}
OID_ALG = {"SHA256": "2a8648ce3d040302", "SHA384": "2a8648ce3d040303", "SHA512": "2a8648ce3d040304",
           "SHA1": "2a8648ce3d0401", "SHA224": "2a8648ce3d040301"}


def sh(*args):
    subprocess.run(args, check=True, capture_output=True)


class Pki:
    def __init__(self, d):
        self.d = d
        self.serial = 1
        with open(os.path.join(d, "ca.ext"), "w") as f:
            f.write("basicConstraints=critical,CA:TRUE\nkeyUsage=critical,keyCertSign,cRLSign\n")
        with open(os.path.join(d, "leaf.ext"), "w") as f:
            f.write("basicConstraints=critical,CA:FALSE\nkeyUsage=critical,digitalSignature\n")

    def path(self, name, ext):
        return os.path.join(self.d, f"{name}.{ext}")

    def key(self, name, curve):
        sh("openssl", "ecparam", "-name", OSSL_CURVE[curve], "-genkey", "-noout", "-out",
           self.path(name, "key"))

    def cert(self, name, curve, hash_name, issuer=None, ca=False):
        """A certificate for a fresh key on `curve`, signed with `hash_name` by
        `issuer` (None: self-signed). Returns its DER."""
        self.key(name, curve)
        sh("openssl", "req", "-new", "-key", self.path(name, "key"), "-subj",
           f"/O=sha2wide/CN={name}", "-out", self.path(name, "csr"))
        self.serial += 1
        cmd = ["openssl", "x509", "-req", "-in", self.path(name, "csr"), "-days", "3650",
               "-" + hash_name.lower(), "-set_serial", str(self.serial), "-extfile",
               os.path.join(self.d, "ca.ext" if ca else "leaf.ext"), "-out", self.path(name, "pem")]
        if issuer is None:
            cmd += ["-signkey", self.path(name, "key")]
        else:
            cmd += ["-CA", self.path(issuer, "pem"), "-CAkey", self.path(issuer, "key")]
        sh(*cmd)
        return next(pem_certs(self.path(name, "pem")))


def cert_key(der):
    """(curve name, x, y) of a certificate's subject public key."""
    c = tlv(der, 0)
    tbs = tlv(c[1], 0)
    t = tlv(tbs[1], 0)
    if t[0] == 0xA0:
        t = tlv(tbs[1], t[3])
    f = t
    for _ in range(5):  # signature, issuer, validity, subject, subjectPublicKeyInfo
        f = tlv(tbs[1], f[3])
    algid = tlv(f[1], 0)
    bits = tlv(f[1], algid[3])
    params = tlv(algid[1], tlv(algid[1], 0)[3])
    curve = OID_CURVE[params[1]]
    cb = 32 if curve == "P-256" else 48
    assert bits[1][:2] == b"\x00\x04" and len(bits[1]) == 2 + 2 * cb
    return curve, int.from_bytes(bits[1][2:2 + cb], "big"), int.from_bytes(bits[1][2 + cb:], "big")


def vec(tag, der, key):
    curve, qx, qy = key
    cb = 32 if curve == "P-256" else 48
    return {"tag": tag, "cert": der.hex(), "curve": curve, "qx": qx.to_bytes(cb, "big").hex(),
            "qy": qy.to_bytes(cb, "big").hex(),
            "reason": W.check_signature_from_ex(der, W.CURVES[curve][0], qx, qy)}


def mutations(tag, der, key, other_key):
    """The gen_x509.py mutations of one verifying link (der <- key)."""
    curve, qx, qy = key
    c = W.CURVES[curve][0]
    n = c.n
    _, _, _, sig = X.split_cert(der)
    r, s = X.parse_signature(sig)
    mine = W.cert_hash(der)
    other = "SHA256" if mine != "SHA256" else "SHA384"

    def m_int(v, nonmin=False, longlen=False):
        b = v.to_bytes(max(1, (v.bit_length() + 8) // 8), "big")
        if nonmin:
            b = b"\x00" + b
        return b"\x02" + (b"\x81" if longlen else b"") + bytes([len(b)]) + b

    def m_sig(rr, ss, tail=b"", extra=b"", rnm=False, rll=False):
        body = m_int(rr, rnm, rll) + m_int(ss) + extra
        assert len(body) < 128
        return b"\x30" + bytes([len(body)]) + body + tail

    flip = lambda t: t[:-3] + bytes([t[-3] ^ 1]) + t[-2:]  # noqa: E731
    oid = lambda name: bytes.fromhex(OID_ALG[name])  # noqa: E731
    cases = {
        "tbs_flip": rebuild(der, tbs_mut=flip),
        "high_s_twin": rebuild(der, m_sig(r, n - s)),
        "der_trailing": rebuild(der, m_sig(r, s, tail=b"\x00")),
        "der_extra_elem": rebuild(der, m_sig(r, s, extra=b"\x02\x01\x07")),
        "der_nonminimal_r": rebuild(der, m_sig(r, s, rnm=True)),
        "der_longform_short": rebuild(der, m_sig(r, s, rll=True)),
        "r_zero": rebuild(der, m_sig(0, s)),
        "s_zero": rebuild(der, m_sig(r, 0)),
        "r_plus_n": rebuild(der, m_sig(r + n, s)),
        "s_plus_n": rebuild(der, m_sig(r, s + n)),
        "negative_r": rebuild(der, b"\x30\x06\x02\x01\xff\x02\x01\x01"),
        "alg_mismatch": rebuild(der, alg_oid=oid(other)),
        "other_hash_alg": rebuild(der, alg_oid=oid(other), inner_oid=oid(other)),
        "sha1_alg": rebuild(der, alg_oid=oid("SHA1"), inner_oid=oid("SHA1")),
        "sha224_alg": rebuild(der, alg_oid=oid("SHA224"), inner_oid=oid("SHA224")),
        "not_a_cert": der[:40],
    }
    if curve == "P-384":  # one byte more than the order holds
        cases["r_49_bytes"] = rebuild(der, m_sig(r | 1 << 384, s))
    out = [vec(f"mut:{name}:{tag}", d, key) for name, d in cases.items()]
    out.append(vec(f"mut:wrong_key:{tag}", der, (curve,) + O.pubkey(c, 12345)))
    out.append(vec(f"mut:offcurve_key:{tag}", der, (curve, qx, qy ^ 1)))
    out.append(vec(f"mut:other_curve_key:{tag}", der, other_key))
    return out


def main():
    vecs, links = [], {}
    with tempfile.TemporaryDirectory() as d:
        pki = Pki(d)

        def link(tag, der, issuer_der, pairing):
            v = vec(tag, der, cert_key(issuer_der))
            vecs.append(v)
            if v["reason"] == 0:
                links.setdefault(pairing, (tag, der, cert_key(issuer_der)))

        # the hardened-CA chain: P-384 root -> P-384 intermediate -> P-256 leaf
        root = pki.cert("root384", "P-384", "SHA384", ca=True)
        inter = pki.cert("int384", "P-384", "SHA384", issuer="root384", ca=True)
        link("chain:root384<-root384", root, root, ("P-384", "SHA384"))
        link("chain:int384<-root384", inter, root, ("P-384", "SHA384"))
        for k, lc in enumerate(("P-256", "P-384", "P-256", "P-384", "P-256")):
            leaf = pki.cert(f"leaf{k}.int384", lc, "SHA384", issuer="int384")
            link(f"chain:leaf{k}({lc})<-int384", leaf, inter, ("P-384", "SHA384"))
            if k == 0:  # the leaf against the root: a link that is not one
                vecs.append(vec("chain:leaf0<-root384(not its issuer)", leaf, cert_key(root)))
        # one CA per remaining (issuer curve, hash) pairing
        for cc, hh in (("P-384", "SHA256"), ("P-384", "SHA512"), ("P-256", "SHA256"),
                       ("P-256", "SHA384"), ("P-256", "SHA512")):
            name = f"ca{cc[2:]}{hh[3:]}"
            ca = pki.cert(name, cc, hh, ca=True)
            link(f"ca:{name}<-{name}", ca, ca, (cc, hh))
            for k, lc in enumerate(("P-256", "P-384", "P-256", "P-384", "P-256")):
                leaf = pki.cert(f"leaf{k}.{name}", lc, hh, issuer=name)
                link(f"ca:leaf{k}({lc})<-{name}", leaf, ca, (cc, hh))
    for pairing in sorted(links):
        tag, der, key = links[pairing]
        # a key of the other curve: the first link of that curve's SHA-256 CA
        other = links[("P-256" if pairing[0] == "P-384" else "P-384", "SHA256")][2]
        vecs.extend(mutations(tag, der, key, other))
    ok = Counter((v["curve"], W.cert_hash(bytes.fromhex(v["cert"]))) for v in vecs if v["reason"] == 0)
    assert len(ok) == 6 and min(ok.values()) >= 6, ok
    assert {v["reason"] for v in vecs} >= {0, 3, 4, 5, 7, 8, 9, 10, 11}
    with open(OUT, "w") as f:
        json.dump(vecs, f, indent=0)
    assert os.path.getsize(OUT) <= 422223  # no larger than x509_vectors.json
    print(len(vecs), "vectors", sorted(Counter(v["reason"] for v in vecs).items()), dict(ok))


if __name__ == "__main__":
    main()
