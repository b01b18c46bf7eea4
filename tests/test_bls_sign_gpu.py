"""GPU tests of batched BLS share signing through the C ABI.  Shares are deterministic, so every check
is byte for byte: against the oracle-made fixture (tests/golden/bls_sign_vectors.json), against the
host shim's plain double-and-add (tests/cpp/bn254_shim.cpp shim_sign_share, scalar-multiplication
code independent of the lane routine), against the Python oracle and against the one-message row
kernel (cbft_bls_sign)."""
import ctypes
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import blsgen
import bn254_ref as B
import cbft_hipcrypto as cb
from bls_sign_vectors import load_fixture, pack
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -22
NMAX = 1025


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sign_packed(c, tid, idx, blob, off, lens, out=None):
    n = int(lens.shape[0])
    if out is None:
        out = np.zeros((max(n, 1), 37), dtype=np.uint8)
    rc = c.lib.cbft_bls_sign_batch(c.handle, tid, None if idx is None else _p(idx), _p(blob), _p(off), _p(lens), n,
                                   _p(out))
    return rc, out[:n]


def _shim_share(sk: int, sid: int, msg: bytes) -> bytes:
    out = ctypes.create_string_buffer(37)
    blsgen.shim().shim_sign_share(blsgen.be32(sk), sid, msg, len(msg), out)
    return out.raw


def _shim_many(jobs):
    """[(sk, id, msg)] -> (n, 37) uint8 through shim_sign_share on host threads (ctypes drops the GIL)."""
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(lambda j: _shim_share(*j), jobs))
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(jobs), 37)


class OneSigner:
    """One signer and NMAX 32-byte messages; the size tests sign prefixes of them.  The shim's shares are
    computed once, the oracle's on demand (and kept)."""
    sk = random.Random(0x51).randrange(1, B.R)
    sid = 7

    def __init__(self):
        rng = random.Random(0x52)
        self.msgs = [rng.randbytes(32) for _ in range(NMAX)]
        self.shim = _shim_many([(self.sk, self.sid, m) for m in self.msgs])
        self._oracle = {}

    def oracle(self, i: int) -> bytes:
        if i not in self._oracle:
            self._oracle[i] = B.sign_share(self.sk, self.sid, self.msgs[i])
        return self._oracle[i]


@pytest.fixture(scope="module")
def one():
    return OneSigner()


def test_whole_fixture_one_batch(ctx):
    """The fixture as ONE shuffled variable-length batch (lengths 0 .. 4,096, hashes that need 0 .. 16
    increments) over a 24-signer table whose scalars include every degenerate GLV split; and the table's
    verification keys against the oracle's sk * g2."""
    signers, vectors = load_fixture()
    tid = ctx.load_bls_signers([sk for sk, _ in signers], [sid for _, sid in signers])
    try:
        order = list(range(len(vectors)))
        random.Random(5).shuffle(order)  # neighbours in a wave differ in signer, length and tries
        got = ctx.bls_sign_batch(tid, [vectors[i].msg for i in order], [vectors[i].signer for i in order])
        bad = [i for j, i in enumerate(order) if got[j].tobytes() != vectors[i].share]
        assert not bad, f"{len(bad)} shares differ, first records {bad[:8]}"
        vks = ctx.bls_signer_public_keys(tid)
        for (sk, _), vk in zip(signers, vks):
            assert vk == B.g2_to_bytes(B.ec_mul(sk, B.G2_GEN)), f"vk of sk = {sk:#x}"
    finally:
        ctx.unload_bls_signers(tid)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, NMAX])
def test_batch_size_edges(ctx, one, n):
    """One signer, 32-byte messages (a Digest): lane, wave and hash-chunk edges.  Every share equals the
    shim's double-and-add, 32 sampled ones the Python oracle, 16 the row kernel."""
    blob, off, lens = pack(one.msgs[:n])
    tid = ctx.load_bls_signers([one.sk], [one.sid])
    try:
        rc, got = _sign_packed(ctx, tid, None, blob, off, lens)
    finally:
        ctx.unload_bls_signers(tid)
    assert rc == 0
    bad = np.nonzero((got != one.shim[:n]).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} differ from the shim, first {bad[:8]}"
    rng = random.Random(n)
    for i in sorted(rng.sample(range(n), min(n, 32))):
        assert got[i].tobytes() == one.oracle(i), f"share {i} differs from the oracle"
    for i in sorted(rng.sample(range(n), min(n, 16))):
        assert got[i].tobytes() == ctx.bls_sign(one.sk, one.sid, one.msgs[i]), f"share {i} differs from cbft_bls_sign"


def test_threshold_round_trip(ctx):
    """16 signers of an 11-of-16 key set sign one message in one batch through signer_idx: the share
    verifier accepts all 16, 11 of them combine to a signature that verifies under the group key, and
    with one message bit flipped nothing verifies."""
    n, k = 16, 11
    _, sks, pk, vks = blsgen.keyset(n, k, seed=0xB1D)
    msg = random.Random(3).randbytes(32)
    tid = ctx.load_bls_signers([sks[i] for i in range(1, n + 1)], list(range(1, n + 1)))
    try:
        got = ctx.bls_sign_batch(tid, [msg] * n, list(range(n)))
        assert ctx.bls_signer_public_keys(tid) == vks
    finally:
        ctx.unload_bls_signers(tid)
    shares = [got[i].tobytes() for i in range(n)]
    kid = ctx.bls_load_keys(pk, vks)
    try:
        assert ctx.bls_verify_shares(kid, msg, shares).all()
        sig = ctx.bls_combine(shares[2:2 + k])
        assert ctx.bls_verify(kid, msg, sig)
        flipped = bytes([msg[0] ^ 0x10]) + msg[1:]
        assert not ctx.bls_verify_shares(kid, flipped, shares).any()
        assert not ctx.bls_verify(kid, flipped, sig)
    finally:
        ctx.bls_unload_keys(kid)


def test_device_entry_two_streams_and_bad_index():
    """cbft_bls_sign_fixed_device: two back-to-back calls on two streams with different messages and
    outputs are both exact (they share the scratch: the library orders them), and an out-of-range
    d_signer_idx entry gives 37 zero bytes with exact neighbours."""
    hip = Hip()
    n, L, k = 300, 32, 3
    rng = random.Random(77)
    signers = [(rng.randrange(1, B.R), 10 + i) for i in range(k)]
    batches = []
    for b in range(2):
        msgs = [rng.randbytes(L) for _ in range(n)]
        idx = np.array([rng.randrange(k) for _ in range(n)], dtype=np.uint32)
        exp = _shim_many([(signers[s][0], signers[s][1], m) for s, m in zip(idx, msgs)])
        batches.append((np.frombuffer(b"".join(msgs), dtype=np.uint8).copy(), idx, exp))
    bad_at = [0, 63, 64, 150, n - 1]
    idx_bad = batches[0][1].copy()
    idx_bad[bad_at] = np.array([k, k + 1, 0xFFFFFFFF, 1 << 20, k], dtype=np.uint32)
    try:
        with cb.Context(device=0) as c:
            tid = c.load_bls_signers([sk for sk, _ in signers], [sid for _, sid in signers])
            streams = [hip.stream(), hip.stream()]
            outs = []
            for b, (blob, idx, _) in enumerate(batches):
                d_out = hip.to_dev(np.full(n * 37, 0xA5, dtype=np.uint8))
                c.bls_sign_fixed_device(tid, hip.to_dev(idx), hip.to_dev(blob), L, n, d_out, streams[b])
                outs.append(d_out)
            d_out = hip.to_dev(np.full(n * 37, 0xA5, dtype=np.uint8))
            c.bls_sign_fixed_device(tid, hip.to_dev(idx_bad), hip.to_dev(batches[0][0]), L, n, d_out, None)
            hip.sync()
            for b in range(2):
                got = hip.from_dev(outs[b], n * 37).reshape(n, 37)
                bad = np.nonzero((got != batches[b][2]).any(axis=1))[0]
                assert bad.size == 0, f"stream {b}: {bad.size} differ, first {bad[:8]}"
            got = hip.from_dev(d_out, n * 37).reshape(n, 37)
            exp = batches[0][2].copy()
            exp[bad_at] = 0
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert bad.size == 0, f"bad-index batch: rows {bad[:8]} differ"
            c.unload_bls_signers(tid)
    finally:
        hip.close()


def _load_raw(c, sk_bytes: bytes, ids):
    sk = np.frombuffer(sk_bytes, dtype=np.uint8).copy()
    idv = np.array(ids, dtype=np.uint32)
    tid = ctypes.c_uint32(0)
    return c.lib.cbft_bls_load_signers(c.handle, _p(sk), _p(idv), len(ids), ctypes.byref(tid)), tid.value


def test_argument_errors(ctx):
    rng = random.Random(9)
    signers = [(rng.randrange(1, B.R), 1), (rng.randrange(1, B.R), 2048)]
    msgs = [rng.randbytes(32) for _ in range(4)]
    blob, off, lens = pack(msgs)
    use = np.array([0, 1, 1, 0], dtype=np.uint32)
    exp = _shim_many([(signers[s][0], signers[s][1], m) for s, m in zip(use, msgs)])
    tid = ctx.load_bls_signers([sk for sk, _ in signers], [sid for _, sid in signers])
    rc, _ = _sign_packed(ctx, tid + 1000, None, blob, off, lens)
    assert rc == EINVAL, "unknown table id"
    # host index out of range: refused before any launch, out37 untouched
    out = np.full((4, 37), 0xC3, dtype=np.uint8)
    rc, _ = _sign_packed(ctx, tid, np.array([0, 1, 2, 0], dtype=np.uint32), blob, off, lens, out)
    assert rc == EINVAL and (out == 0xC3).all()
    # n = 0
    rc, _ = _sign_packed(ctx, tid, None, blob, off[:0], lens[:0])
    assert rc == 0
    rc, got = _sign_packed(ctx, tid, use, blob, off, lens)
    assert rc == 0 and np.array_equal(got, exp)
    ctx.unload_bls_signers(tid)
    rc, _ = _sign_packed(ctx, tid, None, blob, off, lens)
    assert rc == EINVAL, "sign after unload"
    assert ctx.lib.cbft_bls_unload_signers(ctx.handle, tid) == EINVAL
    # scalars: 0 and r (= 0 mod r) are no keys; a scalar >= r is reduced as cbft_bls_sign does
    good = blsgen.be32(signers[0][0])
    assert _load_raw(ctx, good + blsgen.be32(0), [1, 2])[0] == EINVAL, "sk = 0"
    assert _load_raw(ctx, blsgen.be32(B.R) + good, [1, 2])[0] == EINVAL, "sk = r"
    rc, t3 = _load_raw(ctx, blsgen.be32(B.R + 5), [3])
    assert rc == 0, "sk = r + 5 is reduced"
    assert ctx.bls_sign_batch(t3, [msgs[0]])[0].tobytes() == _shim_share(5, 3, msgs[0])
    ctx.unload_bls_signers(t3)
    # ids outside [1, 2048]
    assert _load_raw(ctx, good, [0])[0] == EINVAL, "id 0"
    assert _load_raw(ctx, good, [2049])[0] == EINVAL, "id 2049"
    # a multi-shard context signs through the host call on its first device; closing it with the
    # table still loaded is fine
    with cb.Context(devices=[0, 0]) as two:
        t2 = two.load_bls_signers([sk for sk, _ in signers], [sid for _, sid in signers])
        rc, got = _sign_packed(two, t2, use, blob, off, lens)
        assert rc == 0 and np.array_equal(got, exp)
        assert two.lib.cbft_bls_sign_fixed_device(two.handle, t2, None, None, 0, 0, None, None) == EINVAL


# ------------------------------------------------------------------------------------------
# inputs a hash never produces (tests/hip/bls_sign_selftest.hip)
# ------------------------------------------------------------------------------------------
def test_try_and_increment_from_given_x():
    """Try-and-increment started at x in {0, 1, p - 1, p - 2, p - 3} (x + 1 wraps mod p) and at 60 random
    x, against the oracle's loop: the final x, y = t^((p + 1) / 4) and the number of increments."""
    path = os.path.join(HERE, "hip", "libbls_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/libbls_sign_selftest.so not built (make selftest)"
    cb.load_library()
    lib = ctypes.CDLL(path)
    rng = random.Random(11)
    xs = [0, 1, B.P - 1, B.P - 2, B.P - 3] + [rng.randrange(B.P) for _ in range(60)]
    n = len(xs)
    xw = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint32).copy()
    out = np.zeros(17 * n, dtype=np.uint32)
    assert lib.bls_sign_selftest_map_from_x(_p(xw), n, _p(out)) == 0
    for i, x0 in enumerate(xs):
        x, inc = x0, 0
        while B.fp_sqrt((x * x * x + B.B1) % B.P) is None:
            x, inc = (x + 1) % B.P, inc + 1
        y = B.fp_sqrt((x * x * x + B.B1) % B.P)
        row = out[17 * i:17 * i + 17]
        assert int.from_bytes(row[:8].tobytes(), "little") == x, f"x0 = {x0:#x}"
        assert int.from_bytes(row[8:16].tobytes(), "little") == y, f"x0 = {x0:#x}"
        assert int(row[16]) == inc
