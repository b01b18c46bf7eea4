"""CPU tests of batched BLS share combination: the lane code of csrc/bls_combine_batch.h (the source
the GPU runs one share per lane) built for the host (tests/cpp/bls_combine_shim.cpp), against the Python
oracle.  No expected value comes from the code under test."""
import os
import random
import subprocess

import pytest

import bn254_ref as B
import bls_combine_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "cpp", "bls_combine_shim_san")
ROOTS = [w for w in (pow(g, (B.R - 1) // 3, B.R) for g in (2, 3, 5, 7)) if w != 1][:1]
ROOTS = ROOTS + [ROOTS[0] * ROOTS[0] % B.R]


@pytest.mark.parametrize("ids", [[1], [1, 2], [1, 2048], [2047, 2048], list(range(1, 22)),
                                 random.Random(1).sample(range(1, 2049), 683)],
                         ids=["1", "1-2", "1-2048", "2047-2048", "1..21", "683 random"])
def test_lagrange_coefficients(ids):
    got, state, dup = U.shim_lagrange(ids)
    want = B.lagrange_coeffs(ids)
    assert state == [1] * len(ids) and not any(dup)
    assert got == {j: want[i] for j, i in enumerate(ids)}
    if ids == [1, 2]:
        assert got == {0: 2, 1: B.R - 1}


def test_lagrange_repeated_id_and_range():
    """A repeated id is reported by both shares that carry it and by nobody else; ids 0 and 2049 are bad
    and stay out of the other shares' coefficients."""
    ids = [3, 9, 4, 9, 11]
    got, state, dup = U.shim_lagrange(ids)
    assert state == [1] * 5 and dup == [0, 1, 0, 1, 0]
    ids = [5, 0, 2049, 8, 2048]
    got, state, dup = U.shim_lagrange(ids)
    assert state == [1, 2, 2, 1, 1] and not any(dup)
    want = B.lagrange_coeffs([5, 8, 2048])
    assert got == {0: want[5], 3: want[8], 4: want[2048]}


def test_lagrange_use_mask():
    """Unused ids are not range-checked, not compared and not part of the set."""
    ids = [7, 0, 12, 7, 5000, 1, 2048, 12]
    use = [1, 0, 1, 0, 0, 1, 1, 0]
    got, state, dup = U.shim_lagrange(ids, use)
    assert state == use and not any(dup)
    want = B.lagrange_coeffs([7, 12, 1, 2048])
    assert got == {0: want[7], 2: want[12], 5: want[1], 6: want[2048]}


def test_scalar_multiplication():
    """0, 1, 2, r - 1, 2^127 +- 1, the cube roots of unity mod r +- 1 and themselves (the GLV split's edge
    cases) and 200 random scalars, on a hash point, against the oracle's ec_mul."""
    assert all(pow(w, 3, B.R) == 1 and w != 1 for w in ROOTS) and ROOTS[0] != ROOTS[1]
    rng = random.Random(0x24)
    ks = [0, 1, 2, 3, B.R - 1, B.R - 2, 2 ** 127 - 1, 2 ** 127, 2 ** 127 + 1, 2 ** 128]
    ks += [w + d for w in ROOTS for d in (-1, 0, 1)]
    ks += [rng.randrange(B.R) for _ in range(200)]
    H = B.g1_map(b"scalar multiplication")
    h33 = B.g1_to_bytes(H)
    bad = [k for k in ks if U.shim_mul(h33, k) != B.g1_to_bytes(B.ec_mul(k, H))]
    assert not bad, f"{len(bad)} of {len(ks)} products differ, first {bad[:4]}"
    assert U.shim_mul(bytes(33), 5) == bytes(33)  # infinity stays infinity


def _sh(i, pt):
    return i.to_bytes(4, "big") + B.g1_to_bytes(pt)


def test_certificate_sum_on_special_operands():
    """Multisig sums (no coefficients: the sum alone): equal points double, opposite points cancel, the sum
    goes on from infinity, infinite shares count for nothing, also across the 64-share boundary of a
    wave."""
    H = B.g1_map(b"sums")
    Q = B.ec_mul(77, H)
    nH = B.ec_neg(H)
    certs = [
        [_sh(1, H), _sh(2, H)],                                   # equal
        [_sh(1, H), _sh(2, nH)],                                  # opposite: infinity
        [_sh(1, H), _sh(2, nH), _sh(3, Q)],                       # on from infinity
        [_sh(1, None), _sh(2, Q)],                                # an infinite share first
        [_sh(1, Q), _sh(2, None), _sh(3, H)],                     # in the middle
        [_sh(1, None), _sh(2, None)],                             # nothing but infinity
        [_sh(1, H), _sh(2, H), _sh(3, H), _sh(4, H)],             # equal partial sums in the tree
        [_sh(i, H if i % 2 else nH) for i in range(1, 71)],       # cancels inside and across two waves
        [_sh(i, H) for i in range(1, 131)],                       # 130 H over three waves
    ]
    sigs, status = U.shim_batch(certs, multisig=True)
    assert status.tolist() == [1] * len(certs)
    assert sigs == [U.multisig_value(c) for c in certs]
    assert sigs[1] == bytes(33) and sigs[5] == bytes(33) and sigs[7] == bytes(33)
    assert sigs[8] == B.g1_to_bytes(B.ec_mul(130, H))


def test_threshold_batch_against_the_oracle_identity():
    """A ragged batch (k = 1, 2, 3, 7, 0, 65, 70) through every stage on the host: each certificate equals
    sk * g1_map(msg); with a use mask that leaves k of n shares, the same."""
    certs, want = [], []
    for c, k in enumerate([1, 2, 3, 7, 0, 65, 70]):
        if k == 0:
            certs.append([])
            want.append(bytes(33))
            continue
        msg = b"ragged %d" % c
        sk, sh = U.sharing(k, k, 0x300 + c, msg)
        certs.append(sh)
        want.append(U.threshold_value(sk, msg))
    sigs, status = U.shim_batch(certs)
    assert status.tolist() == [1, 1, 1, 1, 0, 1, 1]
    assert sigs == want
    msg = b"masked"
    sk, sh = U.sharing(7, 5, 0x310, msg)
    bad = [sh[0][:4] + b"\x05" + sh[0][5:], U.with_id(sh[3], 0)]
    cert = [bad[0], sh[1], sh[2], bad[1], sh[4], sh[5], sh[6]]
    sigs, status = U.shim_batch([cert, cert, cert], use=[1] * 7 + [0, 1, 1, 0, 1, 1, 1] + [0] * 7)
    assert status.tolist() == [0, 1, 0]
    assert sigs == [bytes(33), U.threshold_value(sk, msg), bytes(33)]


def test_crafted_certificates():
    """Refusals and the crafted good cases, threshold and multisig, against bn254_ref.combine_threshold /
    ec_add; a refused certificate leaves its neighbours exact."""
    msg = b"crafted"
    sk, sh = U.sharing(7, 5, 0x320, msg)
    good = sh[:5]
    x = U.off_curve_x()
    same = [sh[0], U.with_id(sh[0], 2), sh[2]]
    opposite = [sh[0], U.with_id(U.negated(sh[0]), 2)]
    infinite = [sh[0], (2).to_bytes(4, "big") + bytes(33), sh[2]]
    certs = [good,
             [sh[0][:4] + b"\x05" + sh[0][5:]] + sh[1:5],
             good,
             sh[:4] + [sh[4][:4] + b"\x02" + B.P.to_bytes(32, "big")],
             sh[:2] + [sh[2][:4] + b"\x02" + x.to_bytes(32, "big")] + sh[3:5],
             [U.with_id(sh[0], 0)] + sh[1:5],
             sh[:4] + [U.with_id(sh[4], 2049)],
             sh[:4] + [U.with_id(sh[4], 2)],
             same, opposite, infinite, [], good]
    ok = [1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1]
    for multisig in (False, True):
        sigs, status = U.shim_batch(certs, multisig=multisig)
        assert status.tolist() == ok
        for c, cert in enumerate(certs):
            want = U.crafted_value(cert, multisig) if ok[c] else bytes(33)
            assert sigs[c] == want, f"certificate {c}, multisig {multisig}"
    assert U.crafted_value(opposite, True) == bytes(33)
    assert U.crafted_value(good, False) == U.threshold_value(sk, msg)


def test_stand_alone_sanitizer_run():
    assert os.path.exists(SAN), "tests/cpp/bls_combine_shim_san not built (make bls_combine_shim)"
    p = subprocess.run([SAN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "as expected" in p.stdout
