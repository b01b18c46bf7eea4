"""Writes tests/golden/bls_sign_vectors.json: BLS BN-P254 share-signing vectors made with the
Python oracle (oracle/bn254_ref.py) alone.

Signers: the scalars whose GLV halves are degenerate or extreme (1, 2, 3, r - 1, r - 2, 2^127 +- 1,
2^128, both cube roots of unity mod r and their neighbours) and random ones.  Messages: every
length 0 .. 130 (SHA-256's 55 / 56 / 63 / 64 / 119 / 120 padding edges), 1,000 and 4,096 bytes,
messages whose hash needs 0 .. 12 and 16 increments to reach the curve, and random 32-byte
digests under every signer.

    python tests/golden/gen_bls_sign_vectors.py          (about 20 s)
"""
import hashlib
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import bn254_ref as B  # noqa: E402
from bls_sign_vectors import PATH, BlsSignVector, dump_fixture  # noqa: E402

# b"cbft-bls-sign-%d" % i needs this many increments (checked below against the oracle's loop)
LONG_TRIES = {254: 7, 1268: 8, 1660: 9, 4453: 10, 6658: 11, 2790: 12, 18153: 16}


def increments(msg: bytes) -> int:
    x = int.from_bytes(hashlib.sha256(msg).digest(), "big") % B.P
    k = 0
    while B.fp_sqrt((x * x * x + B.B1) % B.P) is None:
        x = (x + 1) % B.P
        k += 1
    return k


def cube_roots():
    g = 2
    while pow(g, (B.R - 1) // 3, B.R) == 1:
        g += 1
    w = pow(g, (B.R - 1) // 3, B.R)
    return sorted([w, w * w % B.R])


def main():
    rng = random.Random(0xB15)
    w1, w2 = cube_roots()
    scalars = [1, 2, 3, B.R - 1, B.R - 2, 2**127 - 1, 2**127 + 1, 2**128, w1, w2, w1 + 1, w1 - 1, w2 + 1, w2 - 1]
    scalars += [rng.randrange(1, B.R) for _ in range(10)]
    signers = [(sk, 1 + (37 * i) % 2048) for i, sk in enumerate(scalars)]
    signers[3] = (signers[3][0], 2048)
    ns = len(signers)

    tries = {}
    for i, k in LONG_TRIES.items():
        m = b"cbft-bls-sign-%d" % i
        assert increments(m) == k, (i, k)
        tries[k] = m
    i = 0
    while any(k not in tries for k in range(7)):
        m = b"cbft-bls-sign-%d" % i
        tries.setdefault(increments(m), m)
        i += 1

    items = []  # (signer, msg)
    for n in list(range(131)) + [1000, 4096]:
        items.append((n % ns, rng.randbytes(n)))
    for j, k in enumerate(sorted(tries)):
        for q in range(2):
            items.append(((5 * j + 11 * q) % ns, tries[k]))
    for s in range(ns):
        for _ in range(10):
            items.append((s, rng.randbytes(32)))

    vectors = []
    for s, m in items:
        sk, sid = signers[s]
        vectors.append(BlsSignVector(s, m, increments(m), B.sign_share(sk, sid, m)))
    dump_fixture(PATH, signers, vectors)
    print(f"{len(vectors)} vectors, {ns} signers -> {PATH} ({os.path.getsize(PATH)} bytes)")


if __name__ == "__main__":
    main()
