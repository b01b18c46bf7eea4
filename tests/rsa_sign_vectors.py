"""Helpers of the RSA signing tests: the golden fixture's reader, CRT parameters of the test keys
and a restatement, in Python integers, of the scheme the signing kernels run."""
import json
import os
from typing import List, NamedTuple

import rsa_ref
import rsagen

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "rsa_sign_vectors.json")
LENGTHS = [0, 1, 32, 55, 56, 63, 64, 119, 120, 128, 256]
R = 1 << 1036  # the kernels' Montgomery radix: 37 limbs of 28 bits


class RsaSignVector(NamedTuple):
    key: int
    msg: bytes
    sig: bytes


def load_rsa_sign_vectors(path: str = PATH) -> List[RsaSignVector]:
    raw = json.load(open(path))["vectors"]
    return [RsaSignVector(int(v["key"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in raw]


def crt_params(key):
    """(p, q, dP, dQ, qInv, e) of a tests/rsagen.py key, the tuple Context.rsa_load_signers takes."""
    p, q, d = key["p"], key["q"], key["d"]
    return (p, q, d % (p - 1), d % (q - 1), pow(q, -1, p), key["e"])


def em_of(msg: bytes) -> int:
    return int.from_bytes(rsa_ref.emsa_pkcs1_v15_sha256(msg, 2048), "big")


def crt_sign_int(em: int, p: int, q: int, dP: int, dQ: int, qInv: int) -> int:
    """The kernels' scheme on integers.  Both halves start from EM = H R + Lo (no reduction of EM
    mod the prime beforehand), m_q enters the p side as m_q mod p, and the difference is taken as
    m_p + 2p - (a value in [0, 2p) congruent to m_q) so that it is never negative."""
    hi, lo = divmod(em, R)
    m_p = pow((hi * R + lo) % p, dP, p)
    m_q = pow((hi * R + lo) % q, dQ, q)
    for u in (m_q % p, m_q % p + p):  # the lazy product leaves either representative
        d = m_p + 2 * p - u
        assert 0 < d < 3 * p
        h = d * qInv % p
        s = m_q + h * q
        yield s


def crt_sign(em: int, p: int, q: int, dP: int, dQ: int, qInv: int) -> int:
    s = set(crt_sign_int(em, p, q, dP, dQ, qInv))
    assert len(s) == 1, "the two representatives of m_q mod p must give one signature"
    return s.pop()


def crt_edge_ems(p: int, q: int, dP: int, dQ: int, qInv: int):
    """Raw representatives that messages cannot reach, by name: the arithmetic edges of the CRT
    recombination for the key (p, q)."""
    n = p * q
    e = pow(dP, -1, p - 1)  # e d = 1 mod (p - 1): enough to place m_p; the q side uses its own
    eq = pow(dQ, -1, q - 1)

    def em_with(m_p: int, m_q: int) -> int:
        """The representative whose CRT halves are exactly m_p and m_q."""
        a, b = pow(m_p, e, p), pow(m_q, eq, q)
        return (b + q * ((a - b) * qInv % p)) % n

    out = {"zero": 0, "one": 1, "n_minus_1": n - 1, "multiple_of_p": 3 * p, "multiple_of_q": 5 * q,
           "mp_eq_mq": em_with(12345, 12345), "mp_lt_mq": em_with(5, 7)}
    if p < q:
        out["mq_ge_p"] = em_with(9, p + 1)
    return out
