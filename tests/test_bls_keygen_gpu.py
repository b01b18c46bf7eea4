"""GPU tests of batched BLS key derivation and threshold key generation through the C ABI.  Keys are
deterministic, so every check is byte for byte: against the oracle-made fixture
(tests/golden/bls_keygen_vectors.json), against the host shim's plain double-and-add
(tests/cpp/bn254_shim.cpp shim_g2_mul_gen_mt, scalar-multiplication code independent of the lane
routine), against the Python oracle and against the lone row kernel (cbft_bls_public_key)."""
import ctypes
import random

import numpy as np
import pytest

import bn254_ref as B
import cbft_hipcrypto as cb
from bls_keygen_vectors import R, ZERO65, horner, load_fixture, plain_keys, sk_bytes
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
EINVAL = -22
NMAX = 1025
BATCH_MIN = 6  # CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT (include/cbft_hipcrypto.h)


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Scalars:
    """NMAX random scalars below 2^256 with zeros planted at lanes 0 and 63; the size tests derive prefixes
    of them.  The shim's keys are computed once, the oracle's on demand (and kept)."""

    def __init__(self):
        rng = random.Random(0x61)
        self.sks = [rng.randrange(2**256) for _ in range(NMAX)]
        self.sks[0], self.sks[63] = 0, R
        self.shim = plain_keys(self.sks)
        self._oracle = {}

    def oracle(self, i: int) -> bytes:
        if i not in self._oracle:
            k = self.sks[i] % R
            self._oracle[i] = B.g2_to_bytes(B.ec_mul(k, B.G2_GEN)) if k else ZERO65
        return self._oracle[i]


@pytest.fixture(scope="module")
def scalars():
    return Scalars()


def _device_keys(c, hip, sks, stream=None):
    n = len(sks)
    d_out = hip.to_dev(np.full(n * 65, 0xA5, dtype=np.uint8))
    d_ok = hip.to_dev(np.full(n, 0xA5, dtype=np.uint8))
    c.bls_public_key_fixed_device(hip.to_dev(sk_bytes(sks)), n, d_out, d_ok, stream)
    return d_out, d_ok


def _fetch_keys(hip, d_out, d_ok, n):
    out = hip.from_dev(d_out, n * 65).reshape(n, 65)
    return [out[i].tobytes() for i in range(n)], hip.from_dev(d_ok, n).tolist()


def test_whole_fixture_one_batch(ctx):
    """The fixture (every edge class: scalars at and above r, zeros, 1 / 2 / 3 / r - 1 / r - 2, every
    recoded nibble at every position, both signs) as ONE shuffled batch through the host form and through
    the device form; 16 sampled items against the lone cbft_bls_public_key."""
    vectors = load_fixture()
    order = list(range(len(vectors)))
    random.Random(5).shuffle(order)
    sks = [vectors[i].sk for i in order]
    keys, ok = ctx.bls_public_key_batch(sks)
    bad = [vectors[i].cls for j, i in enumerate(order) if keys[j] != vectors[i].vk or ok[j] != vectors[i].ok]
    assert not bad, f"host form: {len(bad)} keys differ, first {bad[:8]}"
    hip = Hip()
    try:
        d_out, d_ok = _device_keys(ctx, hip, sks)
        hip.sync()
        dkeys, dok = _fetch_keys(hip, d_out, d_ok, len(sks))
    finally:
        hip.close()
    assert dkeys == keys and dok == ok.tolist(), "device form differs from the host form"
    live = [j for j, i in enumerate(order) if vectors[i].ok]
    for j in random.Random(6).sample(live, 16):
        assert keys[j] == ctx.bls_public_key(sks[j]), f"{vectors[order[j]].cls} differs from cbft_bls_public_key"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, NMAX])
def test_batch_size_edges(ctx, scalars, n):
    """Lane and wave edges.  Every key equals the shim's double-and-add, 16 sampled ones the Python oracle;
    the zero scalars at lanes 0 and 63 give 65 zero bytes and ok = 0 with their neighbours intact."""
    keys, ok = ctx.bls_public_key_batch(scalars.sks[:n])
    bad = [i for i in range(n) if keys[i] != scalars.shim[i]]
    assert not bad, f"{len(bad)} of {n} differ from the shim, first {bad[:8]}"
    zeros = [i for i in (0, 63) if i < n]
    assert ok.tolist() == [0 if i in zeros else 1 for i in range(n)]
    assert all(keys[i] == ZERO65 for i in zeros)
    assert all(keys[i] != ZERO65 for i in (1, 62, 64) if i < n)
    for i in sorted(random.Random(n).sample(range(n), min(n, 16))):
        assert keys[i] == scalars.oracle(i), f"key {i} differs from the oracle"


def _deal_raw(c, coeffs, k, n, fill=0xC3, null=None):
    co = sk_bytes(coeffs)
    m = max(1, min(n, 4096))
    bufs = {"sk": np.full((m, 32), fill, dtype=np.uint8), "vk": np.full((m, 65), fill, dtype=np.uint8),
            "pk": np.full(65, fill, dtype=np.uint8), "ok": np.full(m + 1, fill, dtype=np.uint8)}
    args = {"co": _p(co), **{name: _p(a) for name, a in bufs.items()}}
    if null:
        args[null] = None
    rc = c.lib.cbft_bls_keygen_threshold(c.handle, args["co"], k, n, args["sk"], args["vk"], args["pk"], args["ok"])
    return rc, bufs


def _check_dealing(c, coeffs, n):
    sks, vks, pk, ok = c.bls_keygen_threshold(coeffs, n)
    exp = [horner(coeffs, i) for i in range(1, n + 1)]
    assert sks == exp
    want = plain_keys([coeffs[0]] + exp)
    assert pk == want[0] and vks == want[1:]
    assert ok.tolist() == [1 if x % R else 0 for x in [coeffs[0]] + exp]
    return sks, vks, pk, ok


@pytest.mark.parametrize("k,n", [(1, 1), (2, 3), (3, 5), (22, 64), (43, 65)])
def test_keygen_threshold(ctx, k, n):
    """Shares against Python Horner, vk and PK against the shim's double-and-add; coefficients at and above r
    give what their reductions give."""
    rng = random.Random(100 * k + n)
    coeffs = [rng.randrange(1, R) for _ in range(k)]
    sks, vks, pk, _ = _check_dealing(ctx, coeffs, n)
    if k == 1:
        assert sks == [coeffs[0]] * n and vks == [pk] * n
    above = [c + R * rng.randrange(1, (2**256 - c) // R + 1) for c in coeffs]
    assert all(R <= a < 2**256 for a in above)
    got = ctx.bls_keygen_threshold(above, n)
    assert (got[0], got[1], got[2]) == (sks, vks, pk)


def test_keygen_threshold_zero_cases_and_errors(ctx):
    # c_0 = r - 3, c_1 = 1: f(3) = 0, so share 3 has no key and the rest stay valid
    sks, vks, pk, ok = _check_dealing(ctx, [R - 3, 1], 5)
    assert sks[2] == 0 and vks[2] == ZERO65 and ok.tolist() == [1, 1, 1, 0, 1, 1]
    # c_0 = 0 mod r: no group key
    for c0 in (0, R):
        sks, vks, pk, ok = _check_dealing(ctx, [c0, 5, 9], 4)
        assert pk == ZERO65 and ok.tolist() == [0, 1, 1, 1, 1]
    # k = n is allowed
    _check_dealing(ctx, [7, 11, 13, 17, 19], 5)
    # refused before any launch, outputs untouched
    coeffs = [3, 4, 5]
    for k, n in ((0, 3), (4, 3), (3, 2049), (0, 0)):
        rc, bufs = _deal_raw(ctx, coeffs + [1], k, n)
        assert rc == EINVAL and all((a == 0xC3).all() for a in bufs.values()), (k, n)
    for null in ("co", "sk", "vk", "pk", "ok"):
        rc, bufs = _deal_raw(ctx, coeffs, 3, 5, null=null)
        assert rc == EINVAL and all((a == 0xC3).all() for a in bufs.values()), null
    rc, bufs = _deal_raw(ctx, coeffs, 3, 5)
    assert rc == 0 and [int.from_bytes(bufs["sk"][i].tobytes(), "big") for i in range(5)] == [
        horner(coeffs, i) for i in range(1, 6)]
    # the batch call: null pointers, n = 0, too many
    sk = sk_bytes([5, 6])
    out = np.full((2, 65), 0xC3, dtype=np.uint8)
    okb = np.full(2, 0xC3, dtype=np.uint8)
    lib, h = ctx.lib, ctx.handle
    assert lib.cbft_bls_public_key_batch(h, None, 2, _p(out), _p(okb)) == EINVAL
    assert lib.cbft_bls_public_key_batch(h, _p(sk), 2, None, _p(okb)) == EINVAL
    assert lib.cbft_bls_public_key_batch(h, _p(sk), 2, _p(out), None) == EINVAL
    assert lib.cbft_bls_public_key_batch(h, _p(sk), 0, _p(out), _p(okb)) == 0
    assert lib.cbft_bls_public_key_batch(h, _p(sk), (1 << 20) + 1, _p(out), _p(okb)) == -7
    assert (out == 0xC3).all() and (okb == 0xC3).all()
    assert lib.cbft_bls_public_key_fixed_device(h, None, 2, None, None, None) == EINVAL
    assert lib.cbft_bls_public_key_fixed_device(h, None, 0, None, None, None) == 0
    # a multi-shard context derives keys through the host calls on its first device
    with cb.Context(devices=[0, 0]) as two:
        keys, ok2 = two.bls_public_key_batch([5, 0, 6])
        assert keys == plain_keys([5, 0, 6]) and ok2.tolist() == [1, 0, 1]
        assert two.bls_keygen_threshold(coeffs, 5)[0] == [horner(coeffs, i) for i in range(1, 6)]
        assert two.lib.cbft_bls_public_key_fixed_device(two.handle, None, 0, None, None, None) == EINVAL


@pytest.mark.parametrize("k,n", [(3, 5), (22, 64)])
def test_round_trip(ctx, k, n):
    """A dealt key set through the rest of the library: the keys load as a verifier key set (status all 1),
    the shares load as a signer table, 8 digests are signed by every signer in one batch, two different
    k-subsets per digest combine to the same certificate, every certificate verifies under slot 0 and
    every share under its slot i."""
    rng = random.Random(7 * n + k)
    coeffs = [rng.randrange(1, R) for _ in range(k)]
    sks, vks, pk, ok = ctx.bls_keygen_threshold(coeffs, n)
    assert ok.all()
    digests = [rng.randbytes(32) for _ in range(8)]
    kid = ctx.bls_load_keys(pk, vks)
    tid = ctx.load_bls_signers(sks, list(range(1, n + 1)))
    try:
        assert ctx.bls_key_status(kid, n) == b"\x01" * (n + 1)
        assert ctx.bls_signer_public_keys(tid) == vks
        msgs = [d for d in digests for _ in range(n)]
        idx = [s for _ in digests for s in range(n)]
        shares = ctx.bls_sign_batch(tid, msgs, idx)
        rows = [[shares[m * n + s].tobytes() for s in range(n)] for m in range(8)]
        certs = []
        for m in range(8):
            first = sorted(rng.sample(range(n), k))
            second = sorted(rng.sample(range(n), k))
            while second == first and k < n:
                second = sorted(rng.sample(range(n), k))
            certs += [[rows[m][s] for s in first], [rows[m][s] for s in second]]
        sigs, status = ctx.bls_combine_batch(certs)
        assert status.all()
        assert all(sigs[2 * m] == sigs[2 * m + 1] for m in range(8)), "two subsets, two certificates"
        assert ctx.bls_verify_batch(kid, [sigs[2 * m] for m in range(8)], digests).all()
        assert ctx.bls_verify_batch(kid, [sh[4:] for row in rows for sh in row], digests,
                                    key_idx=[s + 1 for _ in range(8) for s in range(n)],
                                    msg_of=[m for m in range(8) for _ in range(n)]).all()
    finally:
        ctx.unload_bls_signers(tid)
        ctx.bls_unload_keys(kid)


def test_multisig_key_sum(ctx):
    """Multisig key generation is n independent scalars and PK = (sum sk_i mod r) * g2 as one more item of
    the same call: cbft_bls_sum_keys over all 16 keys equals that item."""
    rng = random.Random(16)
    sks = [rng.randrange(1, R) for _ in range(16)]
    keys, ok = ctx.bls_public_key_batch(sks + [sum(sks) % R])
    assert ok.all()
    kid = ctx.bls_load_keys(keys[16], keys[:16])
    try:
        assert ctx.bls_sum_keys(kid, B.signers_bitmap(range(1, 17))) == keys[16]
    finally:
        ctx.bls_unload_keys(kid)


def test_load_signers_same_keys(ctx):
    """A signer table of 257 keys (derived by the batch kernel): its verification keys equal the batch
    call's and the shim's.  Tables on both sides of the switch between the per-key loop and the batch
    launch (CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT - 1 and that many keys), and of one key, agree as well."""
    rng = random.Random(257)
    sks = [rng.randrange(1, R) for _ in range(257)]
    sks[:3] = [1, 2, R - 1]
    keys, ok = ctx.bls_public_key_batch(sks)
    assert ok.all() and keys == plain_keys(sks)
    for lo, n in ((0, 257), (5, 1), (7, BATCH_MIN - 1), (20, BATCH_MIN), (0, 64), (1, 65)):
        tid = ctx.load_bls_signers(sks[lo:lo + n], [1 + i for i in range(n)])
        try:
            assert ctx.bls_signer_public_keys(tid) == keys[lo:lo + n], f"table of {n} keys"
        finally:
            ctx.unload_bls_signers(tid)


def test_two_streams():
    """cbft_bls_public_key_fixed_device: two back-to-back calls on two streams of a fresh context (the
    first one builds the comb of g2) with different scalars and outputs are both exact."""
    hip = Hip()
    rng = random.Random(78)
    batches = [[rng.randrange(2**256) for _ in range(300)] for _ in range(2)]
    batches[1][17] = 0
    try:
        with cb.Context(device=0) as c:
            streams = [hip.stream(), hip.stream()]
            outs = [_device_keys(c, hip, sks, streams[b]) for b, sks in enumerate(batches)]
            hip.sync()
            for b, sks in enumerate(batches):
                keys, ok = _fetch_keys(hip, *outs[b], len(sks))
                assert keys == plain_keys(sks), f"stream {b}"
                assert ok == [1 if x % R else 0 for x in sks], f"stream {b}"
    finally:
        hip.close()


def test_selftest_geometries_agree():
    """tests/hip/bls_keygen_selftest.hip (what tools/bls_keygen_bench.py times): the product kernel and the
    row-parallel comb over a grid give the shim's keys for 65 scalars, the edges 1, 2, r - 1, r - 2 among them."""
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "libbls_keygen_selftest.so")
    assert os.path.exists(path), "tests/hip/libbls_keygen_selftest.so not built (make selftest)"
    cb.load_library()
    st = ctypes.CDLL(path)
    rng = random.Random(65)
    sks = [1, 2, R - 1, R - 2] + [rng.randrange(1, R) for _ in range(61)]
    n = len(sks)
    lane = np.zeros((n, 65), dtype=np.uint8)
    row = np.zeros((n, 65), dtype=np.uint8)
    ms = np.zeros((2, 1), dtype=np.float32)
    assert st.bls_keygen_selftest_geometries(_p(sk_bytes(sks)), n, 1, _p(lane), _p(row), _p(ms[0]), _p(ms[1])) == 0
    exp = plain_keys(sks)
    assert [lane[i].tobytes() for i in range(n)] == exp, "one key per lane"
    assert [row[i].tobytes() for i in range(n)] == exp, "row comb, one key per block"
