"""Writes tests/golden/bls_keygen_vectors.json: BLS BN-P254 key derivation vectors, vk = (sk mod r) * g2,
made with the Python oracle (oracle/bn254_ref.py) alone.

Scalars: 1, 2, 3, r - 1, r - 2, r - 3; values at and above r (r, r + 1, 2r - 1, 2^255, 2^256 - 1) and 0,
with 65 zero bytes and ok = 0 where the scalar is 0 mod r; an even / odd neighbour pair; scalars whose
recoded radix-16 digits (csrc/bls_keygen_batch.h: the nibbles of u = (k' + 2^256 - 1) / 2) are one value v
in positions 0..62 for every v = 0..15, or alternate 0 / 15, each as the odd scalar itself and, for some,
as the even scalar r - k' that takes the negation path; and random ones.

    python tests/golden/gen_bls_keygen_vectors.py          (about 5 s)
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import bn254_ref as B  # noqa: E402
from bls_keygen_vectors import PATH, R, ZERO65, BlsKeygenVector, dump_fixture, recoded_nibbles  # noqa: E402

assert R == B.R


def from_nibbles(low63) -> int:
    """The odd k' whose recoding has these digits in positions 0..62 and 8 on top (k' = 2 L + 1 < 2^253 < r)."""
    L = sum(v << (4 * j) for j, v in enumerate(low63))
    k = 2 * L + 1
    assert recoded_nibbles(k) == list(low63) + [8]
    return k


def main():
    rng = random.Random(0xB15C0DE)
    cases = [("small", 1), ("small", 2), ("small", 3), ("top", R - 1), ("top", R - 2), ("top", R - 3),
             ("zero", 0), ("zero", R), ("above_r", R + 1), ("above_r", 2 * R - 1), ("above_r", 2**255),
             ("above_r", 2**256 - 1), ("above_r", 6 * R), ("above_r", 4 * R + 5), ("above_r", 2 * R)]
    x = rng.randrange(2, R - 2) & ~1
    cases += [("pair", x), ("pair", x + 1)]
    for v in range(16):
        k = from_nibbles([v] * 63)
        cases.append((f"nibbles_{v}", k))
        if v in (0, 7, 8, 15):
            cases.append((f"nibbles_{v}_even", R - k))
    for name, pat in (("alt_0_15", [0, 15]), ("alt_15_0", [15, 0]), ("alt_7_8", [7, 8])):
        k = from_nibbles([pat[j & 1] for j in range(63)])
        cases += [(name, k), (name + "_even", R - k)]
    while len(cases) < 64:
        cases.append(("random", rng.randrange(1, 2**256)))
    vectors = []
    for cls, sk in cases:
        k = sk % R
        vk = B.g2_to_bytes(B.ec_mul(k, B.G2_GEN)) if k else ZERO65
        vectors.append(BlsKeygenVector(cls, sk, vk, 1 if k else 0))
    dump_fixture(PATH, vectors)
    print(f"{len(vectors)} vectors -> {PATH}")


if __name__ == "__main__":
    main()
