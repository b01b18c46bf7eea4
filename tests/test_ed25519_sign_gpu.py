"""GPU tests of batched Ed25519 signing through the C ABI.  Signatures are deterministic (RFC 8032
§5.1.6), so every check is byte for byte: against the OpenSSL-generated fixture
(tests/golden/ed25519_sign_vectors.bin), against host OpenSSL run in the test, and through the
library's own batch verify."""
import ctypes
import os
import random

import numpy as np
import pytest

import cbft_hipcrypto as cb
import ed25519_ref as E
from sign_vectors import Hip, load_sign_vectors, openssl_sign_many

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -22


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def vectors():
    return load_sign_vectors()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fixed_batch(n, msg_len, seed):
    """n random messages of msg_len bytes as (blob, off, len)."""
    rng = np.random.default_rng(seed)
    blob = rng.integers(0, 256, size=max(1, n * msg_len), dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(msg_len)
    lens = np.full(n, msg_len, dtype=np.uint32)
    return blob, off, lens


def _sign_packed(c, tid, idx, blob, off, lens, out=None):
    n = int(lens.shape[0])
    if out is None:
        out = np.zeros((max(n, 1), 64), dtype=np.uint8)
    rc = c.lib.cbft_ed25519_sign_batch(c.handle, tid, None if idx is None else _p(idx), _p(blob), _p(off), _p(lens), n,
                                       _p(out))
    return rc, out[:n]


def _seeds(k, seed):
    return np.frombuffer(random.Random(seed).randbytes(32 * k), dtype=np.uint8).reshape(k, 32)


def test_whole_fixture_byte_exact(ctx, vectors):
    """The fixture as ONE variable-length batch (lengths 0 .. 4,096, both hashes' padding edges),
    its signers mixed through signer_idx: all 64 bytes of every signature, and the public keys."""
    seeds = []
    for v in vectors:
        if v.seed not in seeds:
            seeds.append(v.seed)
    assert len(seeds) == 11  # 3 RFC 8032 keys + the 8 fixture seeds
    tid = ctx.load_signers(seeds)
    try:
        pks = ctx.signer_public_keys(tid)
        for s, pk in zip(seeds, pks):
            assert pk.tobytes() == next(v.pk for v in vectors if v.seed == s)
        order = list(range(len(vectors)))
        random.Random(5).shuffle(order)  # neighbours in a wave differ in signer and block count
        got = ctx.sign_batch(tid, [vectors[i].msg for i in order], [seeds.index(vectors[i].seed) for i in order])
        bad = [i for j, i in enumerate(order) if got[j].tobytes() != vectors[i].sig]
        assert not bad, f"{len(bad)} signatures differ, first records {bad[:8]}"
    finally:
        ctx.unload_signers(tid)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_batch_size_edges(ctx, n):
    """One signer, 32-byte messages (a pre-process result hash): lane and block edges of the
    256-lane launch, byte-equal to host OpenSSL."""
    seeds = _seeds(1, 100 + n)
    blob, off, lens = _fixed_batch(n, 32, n)
    exp = openssl_sign_many(seeds, np.zeros(n, dtype=np.uint32), blob, off, lens)
    tid = ctx.load_signers(seeds)
    try:
        rc, got = _sign_packed(ctx, tid, None, blob, off, lens)
        assert rc == 0
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} of {n} differ, first {bad[:8]}"
    finally:
        ctx.unload_signers(tid)


def test_round_trip_through_batch_verify(ctx):
    """GPU signatures verify under the GPU verifier with the signer table's own public keys, and
    fail with one message bit flipped."""
    n, k = 700, 5
    seeds = _seeds(k, 31)
    rng = np.random.default_rng(32)
    lens = rng.integers(1, 300, size=n).astype(np.uint32)
    off = np.zeros(n, dtype=np.uint64)
    np.cumsum(lens[:-1].astype(np.uint64), out=off[1:])
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    tid = ctx.load_signers(seeds)
    try:
        rc, sig = _sign_packed(ctx, tid, idx, blob, off, lens)
        assert rc == 0
        pks = ctx.signer_public_keys(tid)
    finally:
        ctx.unload_signers(tid)
    vt = ctx.load_keys(pks)
    try:
        ok = cb.bitmap_to_bools(ctx.verify_packed(vt, idx, sig, blob, off, lens), n)
        assert ok.all(), np.nonzero(~ok)[0][:8]
        flipped = blob.copy()
        flipped[off.astype(np.int64) + (lens // 2).astype(np.int64)] ^= 0x10  # one bit of every message
        ok = cb.bitmap_to_bools(ctx.verify_packed(vt, idx, sig, flipped, off, lens), n)
        assert not ok.any(), np.nonzero(ok)[0][:8]
    finally:
        ctx.unload_keys(vt)


def test_full_size_batch(ctx):
    """65,536 x 32 B under one signer: every signature verifies on the GPU, every 61st (1,075 of
    them) is byte-equal to host OpenSSL."""
    n = 65536
    seeds = _seeds(1, 77)
    blob, off, lens = _fixed_batch(n, 32, 78)
    tid = ctx.load_signers(seeds)
    try:
        rc, sig = _sign_packed(ctx, tid, None, blob, off, lens)
        assert rc == 0
        pks = ctx.signer_public_keys(tid)
    finally:
        ctx.unload_signers(tid)
    zero = np.zeros(n, dtype=np.uint32)
    vt = ctx.load_keys(pks)
    try:
        ok = cb.bitmap_to_bools(ctx.verify_packed(vt, zero, sig, blob, off, lens), n)
    finally:
        ctx.unload_keys(vt)
    assert ok.all(), f"{int((~ok).sum())} signatures do not verify, first {np.nonzero(~ok)[0][:8]}"
    pick = np.arange(0, n, 61)
    assert pick.size == 1075
    sblob = np.ascontiguousarray(blob.reshape(n, 32)[pick]).reshape(-1)
    exp = openssl_sign_many(seeds, np.zeros(pick.size, dtype=np.uint32), sblob,
                            np.arange(pick.size, dtype=np.uint64) * np.uint64(32),
                            np.full(pick.size, 32, dtype=np.uint32))
    bad = np.nonzero((sig[pick] != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {pick.size} sampled signatures differ, first {pick[bad[:8]]}"


def test_device_entry_two_streams_and_bad_index():
    """cbft_ed25519_sign_fixed_device: two back-to-back calls on two streams with different
    messages and outputs are both exact (they share the nonce scratch: the library orders them),
    and an out-of-range d_signer_idx entry gives 64 zero bytes with exact neighbours."""
    hip = Hip()
    n, L, k = 3000, 32, 3
    seeds = _seeds(k, 55)
    batches = []
    for b in range(2):
        blob, off, lens = _fixed_batch(n, L, 500 + b)
        idx = np.random.default_rng(600 + b).integers(0, k, size=n).astype(np.uint32)
        batches.append((blob, off, lens, idx, openssl_sign_many(seeds, idx, blob, off, lens)))
    bad_at = [0, 63, 64, 1500, n - 1]
    idx_bad = batches[0][3].copy()
    idx_bad[bad_at] = np.array([k, k + 1, 0xFFFFFFFF, 1 << 20, k], dtype=np.uint32)
    try:
        with cb.Context(device=0) as c:
            tid = c.load_signers(seeds)
            streams = [hip.stream(), hip.stream()]
            outs = []
            for b, (blob, _, _, idx, _) in enumerate(batches):
                d_out = hip.to_dev(np.full(n * 64, 0xA5, dtype=np.uint8))
                c.sign_fixed_device(tid, hip.to_dev(idx), hip.to_dev(blob), L, n, d_out, streams[b])
                outs.append(d_out)
            d_out = hip.to_dev(np.full(n * 64, 0xA5, dtype=np.uint8))
            c.sign_fixed_device(tid, hip.to_dev(idx_bad), hip.to_dev(batches[0][0]), L, n, d_out, None)
            hip.sync()
            for b in range(2):
                got = hip.from_dev(outs[b], n * 64).reshape(n, 64)
                bad = np.nonzero((got != batches[b][4]).any(axis=1))[0]
                assert bad.size == 0, f"stream {b}: {bad.size} differ, first {bad[:8]}"
            got = hip.from_dev(d_out, n * 64).reshape(n, 64)
            exp = batches[0][4].copy()
            exp[bad_at] = 0
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert bad.size == 0, f"bad-index batch: rows {bad[:8]} differ"
            c.unload_signers(tid)
    finally:
        hip.close()


def test_argument_errors(ctx):
    seeds = _seeds(2, 9)
    blob, off, lens = _fixed_batch(4, 32, 10)
    exp = openssl_sign_many(seeds, np.array([0, 1, 1, 0], dtype=np.uint32), blob, off, lens)
    tid = ctx.load_signers(seeds)
    rc, _ = _sign_packed(ctx, tid + 1000, None, blob, off, lens)
    assert rc == EINVAL, "unknown table id"
    # host index out of range: refused before any launch, out_sig untouched
    out = np.full((4, 64), 0xC3, dtype=np.uint8)
    rc, _ = _sign_packed(ctx, tid, np.array([0, 1, 2, 0], dtype=np.uint32), blob, off, lens, out)
    assert rc == EINVAL and (out == 0xC3).all()
    # n = 0
    rc, _ = _sign_packed(ctx, tid, None, blob, off[:0], lens[:0])
    assert rc == 0
    rc, got = _sign_packed(ctx, tid, np.array([0, 1, 1, 0], dtype=np.uint32), blob, off, lens)
    assert rc == 0 and np.array_equal(got, exp)
    ctx.unload_signers(tid)
    rc, _ = _sign_packed(ctx, tid, None, blob, off, lens)
    assert rc == EINVAL, "sign after unload"
    assert ctx.lib.cbft_ed25519_unload_signers(ctx.handle, tid) == EINVAL
    # a multi-shard context signs through the host call on its first device; closing it with the
    # table still loaded is fine
    with cb.Context(devices=[0, 0]) as two:
        t2 = two.load_signers(seeds)
        rc, got = _sign_packed(two, t2, np.array([0, 1, 1, 0], dtype=np.uint32), blob, off, lens)
        assert rc == 0 and np.array_equal(got, exp)
        assert two.lib.cbft_ed25519_sign_fixed_device(two.handle, t2, None, None, 0, 0, None, None) == EINVAL


# ------------------------------------------------------------------------------------------
# arithmetic edges a hash output never reaches (tests/hip/sign_selftest.hip)
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selftest():
    path = os.path.join(HERE, "hip", "libsign_selftest.so")
    assert os.path.exists(path), "tests/hip/libsign_selftest.so not built (make selftest)"
    return ctypes.CDLL(path)


def _words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).copy()


def _ints(words, n):
    raw = words.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


C88 = int("88" * 32, 16)  # the recoding offset: 8 in every nibble


def test_comb_edges_vs_oracle(selftest):
    """encode([r]B) for r in {0, 1, 2, 8, L-1, L-2, 2^252} and 64 random r, and for the scalars
    whose 64 signed digits are all -8 / all +7 (given as their offset form)."""
    rng = random.Random(2024)
    rs = [0, 1, 2, 8, E.L - 1, E.L - 2, 2**252] + [rng.randrange(E.L) for _ in range(64)]
    n = len(rs)
    out = np.zeros(8 * n, dtype=np.uint32)
    assert selftest.sign_selftest_mul(_p(_words(rs)), _p(out), n, 0) == 0
    raw = out.tobytes()
    for i, r in enumerate(rs):
        assert raw[32 * i:32 * i + 32] == E.encode_point(E.scalar_mult(r, E.B)), f"r = {r:#x}"
    assert raw[:32] == b"\x01" + b"\x00" * 31  # r = 0: the identity
    # offset form: nibbles - 8 are the digits.  all -8: 0; all +7: 0xff..f; plus mixed extremes
    biased = [0, 2**256 - 1, int("0f" * 32, 16), int("f0" * 32, 16), C88]
    out = np.zeros(8 * len(biased), dtype=np.uint32)
    assert selftest.sign_selftest_mul(_p(_words(biased)), _p(out), len(biased), 1) == 0
    raw = out.tobytes()
    for i, v in enumerate(biased):
        k = (v - C88) % E.L
        assert raw[32 * i:32 * i + 32] == E.encode_point(E.scalar_mult(k, E.B)), f"offset form {v:#x}"


def test_sc_muladd_edges_vs_python(selftest):
    rng = random.Random(7)
    trip = [(r, k, a) for r in (0, 1, E.L - 1) for k in (0, 1, E.L - 1) for a in (2**254, 2**255 - 8)]
    trip += [(rng.randrange(E.L), rng.randrange(E.L), (rng.getrandbits(256) & ~7 & (2**255 - 1)) | 2**254)
             for _ in range(64)]
    n = len(trip)
    out = np.zeros(8 * n, dtype=np.uint32)
    rc = selftest.sign_selftest_muladd(_p(_words([t[0] for t in trip])), _p(_words([t[1] for t in trip])),
                                       _p(_words([t[2] for t in trip])), _p(out), n)
    assert rc == 0
    for (r, k, a), got in zip(trip, _ints(out, n)):
        assert got == (r + k * a) % E.L, (hex(r), hex(k), hex(a))
