"""GPU tests of batched BLS share combination (cbft_bls_combine_batch, cbft_bls_combine_fixed_device)
through the C ABI.  Expected values come from the Python oracle: any k shares of a degree-(k - 1)
sharing combine to sk * g1_map(msg) (one scalar multiplication), multisig sums are ec_add over the
decoded points, crafted shares go through bn254_ref.combine_threshold.  Byte equality with the lone
cbft_bls_combine on the same shares is asserted beside that, never instead of it."""
import ctypes

import numpy as np
import pytest

import bn254_ref as B
import bls_combine_util as U
import blsgen
import cbft_hipcrypto as cb
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
EINVAL, E2BIG = -22, -7
RAGGED = [1, 2, 3, 7, 64, 65, 200, 683, 2048]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    return U.Pool()


@pytest.fixture(scope="module")
def ragged():
    """[(shares, threshold value)] for k-of-k sharings, k in RAGGED"""
    out = []
    for c, k in enumerate(RAGGED):
        msg = b"ragged certificate %d" % k
        sk, sh = U.sharing(k, k, 0x2400 + c, msg)
        out.append((sh, U.threshold_value(sk, msg)))
    return out


@pytest.mark.parametrize("multisig", [False, True], ids=["threshold", "multisig"])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_certificate_counts(ctx, pool, m, multisig):
    """k = 5: certificates straddle wave boundaries (13 x 5 = 65 shares) and, from 13 certificates on, a
    launch has more than one block."""
    certs = [pool.cert(c) for c in range(m)]
    sigs, status = ctx.bls_combine_batch(certs, multisig=multisig)
    assert status.tolist() == [1] * m
    want = [U.multisig_value(c) for c in certs[:16]] if multisig else [pool.expected(c) for c in range(m)]
    bad = [c for c in range(len(want)) if sigs[c] != want[c]]
    assert not bad, f"{len(bad)} of {len(want)} certificates differ from the oracle, first {bad[:8]}"
    lone = [ctx.bls_combine(c, multisig=multisig) for c in certs]
    assert sigs == lone, "differs from the lone call"


@pytest.mark.parametrize("multisig", [False, True], ids=["threshold", "multisig"])
def test_ragged_batch(ctx, ragged, multisig):
    """k = 1 .. 2048 side by side, an empty certificate among them."""
    certs = [sh for sh, _ in ragged[:4]] + [[]] + [sh for sh, _ in ragged[4:]]
    sigs, status = ctx.bls_combine_batch(certs, multisig=multisig)
    assert status.tolist() == [1] * 4 + [0] + [1] * 5
    assert sigs[4] == bytes(33)
    got = sigs[:4] + sigs[5:]
    want = [U.multisig_value(sh) if multisig else v for sh, v in ragged]
    bad = [RAGGED[c] for c in range(len(RAGGED)) if got[c] != want[c]]
    assert not bad, f"k = {bad} differ from the oracle"
    assert got == [ctx.bls_combine(sh, multisig=multisig) for sh, _ in ragged], "differs from the lone call"


def _crafted(pool):
    sh = pool.shares[0]
    x = U.off_curve_x()
    good = sh[:5]
    certs = [good,
             [sh[0][:4] + b"\x05" + sh[0][5:]] + sh[1:5],                          # bad prefix
             pool.cert(1),
             sh[:4] + [sh[4][:4] + b"\x02" + B.P.to_bytes(32, "big")],             # x >= p
             sh[:2] + [sh[2][:4] + b"\x02" + x.to_bytes(32, "big")] + sh[3:5],    # x not on the curve
             pool.cert(2),
             [U.with_id(sh[0], 0)] + sh[1:5],                                      # id 0
             sh[:4] + [U.with_id(sh[4], 2049)],                                    # id 2049
             sh[:4] + [U.with_id(sh[4], 2)],                                       # repeated id
             pool.cert(3),
             [sh[0], U.with_id(sh[0], 2), sh[2]],                                  # sigma_a = sigma_b
             [sh[0], U.with_id(U.negated(sh[0]), 2)],                              # sigma_b = -sigma_a
             [sh[0], (2).to_bytes(4, "big") + bytes(33), sh[2]],                   # an infinite share
             [],                                                                   # empty
             pool.cert(4)]
    ok = [1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1]
    return certs, ok


@pytest.mark.parametrize("multisig", [False, True], ids=["threshold", "multisig"])
def test_crafted_batch(ctx, pool, multisig):
    """Good and refused certificates mixed: status and the zero bytes per certificate, every good
    neighbour exact; sigma_b = -sigma_a sums to infinity under multisig (33 zero bytes, status 1)."""
    certs, ok = _crafted(pool)
    sigs, status = ctx.bls_combine_batch(certs, multisig=multisig)
    assert status.tolist() == ok
    for c, cert in enumerate(certs):
        want = U.crafted_value(cert, multisig) if ok[c] else bytes(33)
        assert sigs[c] == want, f"certificate {c}"
    if multisig:
        assert sigs[11] == bytes(33) and status[11] == 1
    for c in (0, 2, 5, 9, 14):
        assert sigs[c] == ctx.bls_combine(certs[c], multisig=multisig), f"certificate {c} differs from the lone call"


def test_use_mask(ctx, pool):
    """Seven shares per certificate with two spoiled and masked out: the five left combine to the oracle
    value; a certificate whose mask drops everything is refused; unused shares are not looked at."""
    certs, use, want = [], [], []
    for c in range(20):
        sh = list(pool.shares[c % pool.worlds])
        a, b = c % 7, (c + 3) % 7
        sh[a] = sh[a][:4] + b"\x05" + sh[a][5:]
        sh[b] = U.with_id(sh[b], [0, 2049, (b + 1) % 7 + 1][c % 3])  # bad ids, or another share's id
        u = [0 if j in (a, b) else 1 for j in range(7)]
        if c % 6 == 5:
            u = [0] * 7
        certs.append(sh)
        use += u
        want.append(bytes(33) if c % 6 == 5 else pool.want[c % pool.worlds])
    sigs, status = ctx.bls_combine_batch(certs, use=use)
    assert status.tolist() == [0 if c % 6 == 5 else 1 for c in range(20)]
    assert sigs == want
    sigs, status = ctx.bls_combine_batch(certs)  # without the mask every one of them is refused
    assert not status.any() and sigs == [bytes(33)] * 20


def _raw(c, shares, off, m, use, multisig, out, status):
    return c.lib.cbft_bls_combine_batch(c.handle, _p(shares), _p(off), m, _p(use), multisig, _p(out), _p(status))


def test_argument_errors(ctx, pool):
    m = 3
    sh = np.frombuffer(b"".join(s for c in range(m) for s in pool.cert(c)), dtype=np.uint8).copy()
    off = np.arange(0, 5 * m + 1, 5, dtype=np.uint64)

    def refused(rc, *a):
        out = np.full(33 * m, 0xAA, dtype=np.uint8)
        st = np.full(m, 0xAA, dtype=np.uint8)
        return _raw(*a, out, st) == rc and (out == 0xAA).all() and (st == 0xAA).all()

    assert refused(EINVAL, ctx, None, off, m, None, 0), "null shares"
    assert refused(EINVAL, ctx, sh, None, m, None, 0), "null offsets"
    bad = off.copy()
    bad[2] = 4
    assert refused(EINVAL, ctx, sh, bad, m, None, 0), "decreasing offsets"
    bad = np.array([0, 5, 5 + 2049, 5 + 2049 + 5], dtype=np.uint64)
    assert refused(EINVAL, ctx, sh, bad, m, None, 0), "k_c > 2048"
    many = np.arange(0, 2048 * 32769 + 1, 2048, dtype=np.uint64)  # 2^26 + 2048 shares; refused before any is read
    out = np.full(33, 0xAA, dtype=np.uint8)
    assert _raw(ctx, sh, many, many.size - 1, None, 0, out, out) == E2BIG and (out == 0xAA).all()
    st = np.full(m, 0xAA, dtype=np.uint8)
    assert _raw(ctx, None, None, 0, None, 0, None, None) == 0, "m = 0"
    assert ctx.lib.cbft_bls_combine_batch(ctx.handle, _p(sh), _p(off), m, None, 0, None, _p(st)) == EINVAL
    assert ctx.lib.cbft_bls_combine_fixed_device(ctx.handle, None, 2049, 1, None, 0, None, None, None) == EINVAL
    with cb.Context(devices=[0, 0]) as two:  # device pointers belong to one GPU
        assert two.lib.cbft_bls_combine_fixed_device(two.handle, None, 5, 0, None, 0, None, None, None) == EINVAL


def test_device_form(pool):
    """cbft_bls_combine_fixed_device on streams of its own: two calls on two streams share the scratch and
    both come out right (threshold and multisig), k = 0 refuses every certificate."""
    hip = Hip()
    m = 70
    certs = [pool.cert(c) for c in range(m)]
    flat = np.frombuffer(b"".join(s for c in certs for s in c), dtype=np.uint8).copy()
    try:
        with cb.Context(device=0) as c:
            d_sh = hip.to_dev(flat)
            s0, s1 = hip.stream(), hip.stream()
            out = [hip.to_dev(np.full(33 * m, 0xA5, dtype=np.uint8)) for _ in range(3)]
            st = [hip.to_dev(np.full(m, 0xA5, dtype=np.uint8)) for _ in range(3)]
            c.bls_combine_fixed_device(d_sh, 5, m, 0, False, out[0], st[0], s0)
            c.bls_combine_fixed_device(d_sh, 5, m, 0, True, out[1], st[1], s1)
            c.bls_combine_fixed_device(0, 0, m, 0, False, out[2], st[2], 0)
            hip.sync()
            got = [hip.from_dev(o, 33 * m).tobytes() for o in out]
            status = [hip.from_dev(s, m).tolist() for s in st]
    finally:
        hip.close()
    assert status == [[1] * m, [1] * m, [0] * m]
    assert [got[0][33 * i:33 * i + 33] for i in range(m)] == [pool.expected(i) for i in range(m)]
    assert [got[1][33 * i:33 * i + 33] for i in range(16)] == [U.multisig_value(certs[i]) for i in range(16)]
    assert got[2] == bytes(33 * m)


def test_verify_combine_verify_chain():
    """cbft_bls_verify_fixed_device -> cbft_bls_combine_fixed_device (d_valid as d_use) ->
    cbft_bls_verify_fixed_device under slot 0, on one stream, no host synchronisation in between.  64
    certificates of n = 7, k = 5 (one key set, 64 messages, all seven shares sent), one bad share planted
    in every fourth: the first verification masks it out and the six left still interpolate, so every
    certificate verifies.  A 65th certificate whose shares are all undecodable is left with nothing
    used: refused, and verdict 0 at the end."""
    hip = Hip()
    m, n = 65, 7
    last = m - 1
    sk, sks, pk, vks = blsgen.keyset(n, 5, seed=0x24C)
    msgs = [(b"chain message %03d" % c).ljust(32, b".") for c in range(m)]
    shares = [blsgen.shares(sks, range(1, n + 1), msgs[c]) for c in range(m)]
    planted = [(c, (c // 4) % n) for c in range(0, last, 4)]
    for c, j in planted:
        shares[c][j] = blsgen.doubled(shares[c][j])
    shares[last] = [s[:4] + b"\x05" + s[5:] for s in shares[last]]
    flat37 = np.frombuffer(b"".join(s for c in shares for s in c), dtype=np.uint8).copy()
    flat33 = np.frombuffer(b"".join(s[4:] for c in shares for s in c), dtype=np.uint8).copy()
    slots = np.array([j + 1 for _ in range(m) for j in range(n)], dtype=np.uint32)
    mof = np.array([c for c in range(m) for _ in range(n)], dtype=np.uint32)
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    try:
        with cb.Context(device=0) as c:
            kid = c.bls_load_keys(pk, vks)
            s = hip.stream()
            d_blob = hip.to_dev(blob)
            d_valid = hip.to_dev(np.full(m * n, 0xA5, dtype=np.uint8))
            d_out = hip.to_dev(np.full(33 * m, 0xA5, dtype=np.uint8))
            d_st = hip.to_dev(np.full(m, 0xA5, dtype=np.uint8))
            d_final = hip.to_dev(np.full(m, 0xA5, dtype=np.uint8))
            c.bls_verify_fixed_device(kid, hip.to_dev(slots), hip.to_dev(flat33), d_blob, 32, m, hip.to_dev(mof), m * n,
                                      d_valid, s)
            c.bls_combine_fixed_device(hip.to_dev(flat37), n, m, d_valid, False, d_out, d_st, s)
            c.bls_verify_fixed_device(kid, 0, d_out, d_blob, 32, m, 0, m, d_final, s)
            hip.sync()
            valid = hip.from_dev(d_valid, m * n).reshape(m, n)
            sigs = hip.from_dev(d_out, 33 * m).tobytes()
            status = hip.from_dev(d_st, m).tolist()
            final = hip.from_dev(d_final, m).tolist()
            c.bls_unload_keys(kid)
    finally:
        hip.close()
    want_valid = np.ones((m, n), dtype=np.uint8)
    for c_, j in planted:
        want_valid[c_, j] = 0
    want_valid[last] = 0
    assert valid.tolist() == want_valid.tolist()
    assert status == [1] * last + [0]
    for c_ in (0, 1, 4, 63):  # with and without a planted share
        assert sigs[33 * c_:33 * c_ + 33] == U.threshold_value(sk, msgs[c_]), f"certificate {c_}"
    assert sigs[33 * last:] == bytes(33)
    assert final == [1] * last + [0]


def test_two_shards_equal_one_device(ctx, pool, ragged):
    """A two-shard context cuts the certificates in two slices: the same bytes as one device."""
    certs = [pool.cert(c) for c in range(37)] + [ragged[5][0], [], ragged[2][0]]
    use = [1] * sum(len(c) for c in certs)
    use[3] = 0  # certificate 0 is left with four shares: another value, still status 1
    for multisig in (False, True):
        one = ctx.bls_combine_batch(certs, use=use, multisig=multisig)
        with cb.Context(devices=[0, 0]) as two:
            got = two.bls_combine_batch(certs, use=use, multisig=multisig)
        assert got[0] == one[0] and got[1].tolist() == one[1].tolist()
        assert one[1].tolist() == [1] * 38 + [0, 1]
        if not multisig:
            assert one[0][1:37] == [pool.expected(c) for c in range(1, 37)]
            assert one[0][37] == ragged[5][1] and one[0][39] == ragged[2][1]
