"""GPU tests of the batched ECDSA secp256k1 / SHA-256 signing through the C ABI: every signature
must equal tests/ecdsa_sign_ref.py's (RFC 6979 nonces, r || s, no low-s rule) byte for byte, and be
accepted by cbft_ecdsa_verify_batch and by OpenSSL."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import cbft_hipcrypto as cb
import ecdsa_ref as ref
import ecdsa_sign_ref as sref
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N = ref.N
FULL = (1 << 256) - 1
EINVAL, E2BIG = -22, -7
NSIGNERS = 37
POOL = 1000


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def openssl():
    path = os.path.join(ROOT, "tools", "cpu_baseline", "libcbft_cpu_openssl_ecdsa.so")
    assert os.path.exists(path), "tools/cpu_baseline/libcbft_cpu_openssl_ecdsa.so not built (make cpu)"
    lib = ctypes.CDLL(path)
    lib.cbft_cpu_ecdsa_keys_new.restype = ctypes.c_void_p

    def verify(pubs: np.ndarray, kidx, sigs: np.ndarray, msgs, threads=16) -> np.ndarray:
        """OpenSSL's ECDSA_do_verify verdict of every signature."""
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8).reshape(-1, 64)
        kidx = np.ascontiguousarray(np.asarray(kidx, dtype=np.uint32))
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        blob, off, lens = cb.pack_messages(msgs)
        n = len(msgs)
        out = np.zeros(max(1, n), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        cache = ctypes.c_void_p(lib.cbft_cpu_ecdsa_keys_new(p(pubs), ctypes.c_uint32(pubs.shape[0])))
        assert cache
        lib.cbft_cpu_ecdsa_verify(cache, p(kidx), p(sigs), p(blob), p(off), p(lens), ctypes.c_size_t(n), p(out),
                                  ctypes.c_int(threads))
        lib.cbft_cpu_ecdsa_keys_free(cache, ctypes.c_uint32(pubs.shape[0]))
        return out[:n].astype(bool)

    return verify


@pytest.fixture(scope="module")
def shim():
    path = os.path.join(HERE, "cpp", "libecdsa_sign_shim.so")
    assert os.path.exists(path), "tests/cpp/libecdsa_sign_shim.so not built (make ecdsa_sign_shim)"
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def pool():
    """1,000 messages of 0..300 bytes over 37 signers with the restatement's signature of each.  Built
    once; the batch tests take prefixes of it."""
    rng = random.Random(0xEC5169)
    privs = [rng.randrange(1, N) for _ in range(NSIGNERS)]
    idx = [rng.randrange(NSIGNERS) for _ in range(POOL)]
    msgs = [rng.randbytes(rng.randrange(0, 301)) for _ in range(POOL)]
    exp = np.frombuffer(b"".join(sref.sign(privs[i], m) for i, m in zip(idx, msgs)), dtype=np.uint8).reshape(POOL, 64)
    return {"privs": privs, "idx": idx, "msgs": msgs, "exp": exp}


@pytest.fixture(scope="module")
def pool_table(ctx, pool):
    tid = ctx.ecdsa_load_signers([be(x) for x in pool["privs"]])
    assert ctx.ecdsa_signer_status(tid, NSIGNERS).all()
    yield tid
    ctx.ecdsa_unload_signers(tid)


def test_golden_vectors(ctx):
    vecs = json.load(open(os.path.join(HERE, "golden", "ecdsa_sign_vectors.json")))["vectors"]
    xs = sorted({v["x"] for v in vecs})
    tid = ctx.ecdsa_load_signers([bytes.fromhex(x) for x in xs])
    got = ctx.ecdsa_sign(tid, [bytes.fromhex(v["msg"]) for v in vecs], [xs.index(v["x"]) for v in vecs])
    bad = [i for i, v in enumerate(vecs) if got[i].tobytes().hex() != v["sig"]]
    assert not bad, bad[:10]
    ctx.ecdsa_unload_signers(tid)


def edge_keys():
    keys = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255, int("8" * 64, 16) % N, N - int("8" * 64, 16),
            (1 << 256) - int("8" * 64, 16), (1 << 256) - int("8" * 64, 16) - 1, int("7" * 64, 16), int("7" * 64, 16) + 1]
    for j in range(64):
        keys += [16**j, 16**j - 1, 8 * 16**j]
    return [k for k in dict.fromkeys(keys) if 0 < k < N]


def test_public_keys_of_edge_scalars(ctx):
    """x G for scalars that drive the comb's recoding to its corners: chosen scalars on the GPU."""
    keys = edge_keys()
    tid = ctx.ecdsa_load_signers([be(x) for x in keys])
    assert ctx.ecdsa_signer_status(tid, len(keys)).all()
    pub = ctx.ecdsa_signer_public_keys(tid, len(keys))
    bad = [hex(x) for i, x in enumerate(keys) if pub[i].tobytes() != sref.public_key(x)]
    assert not bad, bad[:5]
    ctx.ecdsa_unload_signers(tid)


def test_unusable_keys_sign_zeros_and_leave_neighbours_alone(ctx, pool):
    bad_x = [0, N, N + 1, FULL]
    privs = pool["privs"][:8]
    keys = privs[:2] + bad_x[:2] + privs[2:5] + bad_x[2:] + privs[5:]
    bad_at = [i for i, x in enumerate(keys) if x in bad_x]
    tid = ctx.ecdsa_load_signers([be(x) for x in keys])
    st = ctx.ecdsa_signer_status(tid, len(keys))
    assert [not s for s in st] == [i in bad_at for i in range(len(keys))]
    pub = ctx.ecdsa_signer_public_keys(tid, len(keys))
    msgs = [b"message %d" % i for i in range(64)]
    idx = [i % len(keys) for i in range(64)]  # one wave: usable and unusable signers side by side
    got = ctx.ecdsa_sign(tid, msgs, idx)
    for i, (k, m) in enumerate(zip(idx, msgs)):
        if k in bad_at:
            assert not got[i].any() and not pub[k].any()
        else:
            assert got[i].tobytes() == sref.sign(keys[k], m), i
    ctx.ecdsa_unload_signers(tid)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_ragged_batches_vs_restatement_and_verifiers(ctx, pool, pool_table, openssl, n):
    idx, msgs = pool["idx"][:n], pool["msgs"][:n]
    got = ctx.ecdsa_sign(pool_table, msgs, idx)
    bad = np.nonzero((got != pool["exp"][:n]).any(axis=1))[0]
    assert bad.size == 0, bad[:10]
    pub = ctx.ecdsa_signer_public_keys(pool_table, NSIGNERS)
    vt = ctx.ecdsa_load_keys(pub)
    try:
        assert cb.bitmap_to_bools(ctx.ecdsa_verify(vt, idx, got, msgs), n).all()
    finally:
        ctx.ecdsa_unload_keys(vt)
    assert openssl(pub, idx, got, msgs).all()


def test_large_fixed_batch(ctx, pool, pool_table, openssl, shim):
    """65,536 x 32 B: every signature accepted by OpenSSL and equal to the host build of the lane
    code; 256 sampled ones equal the restatement's."""
    n, L = 65536, 32
    rng = np.random.default_rng(0x10000)
    blob = rng.integers(0, 256, size=n * L, dtype=np.uint8)
    idx = rng.integers(0, NSIGNERS, size=n).astype(np.uint32)
    msgs = [blob[i * L:(i + 1) * L].tobytes() for i in range(n)]
    got = ctx.ecdsa_sign(pool_table, msgs, idx)
    privs = np.frombuffer(b"".join(be(x) for x in pool["privs"]), dtype=np.uint8)
    host = np.zeros((n, 64), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    shim.ecdsa_sign_shim_sign_many(p(privs), p(idx), p(blob), ctypes.c_uint32(L), ctypes.c_size_t(n), p(host),
                                   ctypes.c_int(16))
    bad = np.nonzero((got != host).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} differ from the host build, first {bad[:8]}"
    pub = ctx.ecdsa_signer_public_keys(pool_table, NSIGNERS)
    ok = openssl(pub, idx, got, msgs)
    assert ok.all(), np.nonzero(~ok)[0][:8]
    for i in rng.choice(n, size=256, replace=False):
        assert got[i].tobytes() == sref.sign(pool["privs"][idx[i]], msgs[i]), int(i)


def test_device_entry_two_streams_growing_and_bad_index(ctx, pool, pool_table):
    """cbft_ecdsa_sign_fixed_device on two streams that share the context's nonce scratch (the library
    orders them), batch sizes 8 / 300 / 8 so that the scratch grows and shrinks, against the
    restatement; an out-of-range d_signer_idx entry gives 64 zero bytes with exact neighbours; a null index
    array signs everything with signer 0."""
    hip = Hip()
    L = 48
    rng = np.random.default_rng(0xDE7)
    try:
        streams = [hip.stream(), hip.stream()]
        runs = []
        for j, n in enumerate((8, 300, 8)):
            blob = rng.integers(0, 256, size=n * L, dtype=np.uint8)
            idx = rng.integers(0, NSIGNERS, size=n).astype(np.uint32)
            if n == 300:
                idx[[0, 63, 64, 299]] = np.array([NSIGNERS, NSIGNERS + 1, 0xFFFFFFFF, 1 << 20], dtype=np.uint32)
            d_out = hip.to_dev(np.full(n * 64, 0xA5, dtype=np.uint8))
            ctx.ecdsa_sign_device(pool_table, hip.to_dev(idx), hip.to_dev(blob), L, n, d_out, streams[j % 2])
            runs.append((n, blob, idx, d_out))
        n0 = 8
        blob0 = rng.integers(0, 256, size=n0 * L, dtype=np.uint8)
        d_out0 = hip.to_dev(np.full(n0 * 64, 0xA5, dtype=np.uint8))
        ctx.ecdsa_sign_device(pool_table, None, hip.to_dev(blob0), L, n0, d_out0, 0)
        hip.sync()
        for n, blob, idx, d_out in runs:
            got = hip.from_dev(d_out, n * 64).reshape(n, 64)
            msgs = [blob[i * L:(i + 1) * L].tobytes() for i in range(n)]
            for i in range(n):
                want = bytes(64) if idx[i] >= NSIGNERS else sref.sign(pool["privs"][idx[i]], msgs[i])
                assert got[i].tobytes() == want, (n, i)
        got = hip.from_dev(d_out0, n0 * 64).reshape(n0, 64)
        for i in range(n0):
            assert got[i].tobytes() == sref.sign(pool["privs"][0], blob0[i * L:(i + 1) * L].tobytes())
    finally:
        hip.close()


def _sign_packed(c, tid, idx, msgs, n=None, out=None):
    blob, off, lens = cb.pack_messages(msgs)
    n = len(msgs) if n is None else n
    out = np.zeros((max(1, len(msgs)), 64), dtype=np.uint8) if out is None else out
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = c.lib.cbft_ecdsa_sign_batch(c.handle, tid, p(idx), p(blob), p(off), p(lens), ctypes.c_size_t(n), p(out))
    return rc, out


def test_table_lifetime_and_argument_errors(ctx, pool):
    privs = pool["privs"][:2]
    keys = np.frombuffer(b"".join(be(x) for x in privs), dtype=np.uint8)
    msgs = [b"a", b"", b"ccc", b"dddd" * 20]
    idx = np.array([0, 1, 1, 0], dtype=np.uint32)
    exp = np.frombuffer(b"".join(sref.sign(privs[i], m) for i, m in zip(idx, msgs)), dtype=np.uint8).reshape(4, 64)
    lib, h = ctx.lib, ctx.handle
    tid = ctypes.c_uint32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # load: too many keys is E2BIG even with a null key pointer; then the null and empty cases
    assert lib.cbft_ecdsa_load_signers(h, None, (1 << 20) + 1, ctypes.byref(tid)) == E2BIG
    assert lib.cbft_ecdsa_load_signers(h, None, 2, ctypes.byref(tid)) == EINVAL
    assert lib.cbft_ecdsa_load_signers(h, p(keys), 0, ctypes.byref(tid)) == EINVAL
    assert lib.cbft_ecdsa_load_signers(h, p(keys), 2, None) == EINVAL
    t1 = ctx.ecdsa_load_signers(keys)
    rc, got = _sign_packed(ctx, t1, idx, msgs)
    assert rc == 0 and np.array_equal(got, exp)
    # batch: E2BIG before EINVAL; unknown table; n = 0 answered after the table lookup
    assert _sign_packed(ctx, t1, None, msgs, n=(1 << 26) + 1)[0] == E2BIG
    assert lib.cbft_ecdsa_sign_batch(h, t1, None, None, None, None, ctypes.c_size_t((1 << 26) + 1), None) == E2BIG
    assert lib.cbft_ecdsa_sign_batch(h, t1, None, None, None, None, ctypes.c_size_t(4), None) == EINVAL
    assert _sign_packed(ctx, t1 + 1000, idx, msgs)[0] == EINVAL
    assert _sign_packed(ctx, t1 + 1000, None, [])[0] == EINVAL
    assert _sign_packed(ctx, t1, None, [])[0] == 0
    out = np.full((4, 64), 0xC3, dtype=np.uint8)
    rc, _ = _sign_packed(ctx, t1, np.array([0, 1, 2, 0], dtype=np.uint32), msgs, out=out)
    assert rc == EINVAL and (out == 0xC3).all(), "host index out of range: refused before any launch"
    assert lib.cbft_ecdsa_signer_status(h, t1 + 1000, p(out)) == EINVAL
    assert lib.cbft_ecdsa_signer_public_keys(h, t1, None) == EINVAL
    # device entry: E2BIG first, then alignment and null checks
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 0, ctypes.c_size_t((1 << 26) + 1), None, None) == E2BIG
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 32, ctypes.c_size_t(4), None, None) == EINVAL
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1 + 1000, None, None, 0, ctypes.c_size_t(0), None, None) == EINVAL
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 0, ctypes.c_size_t(0), None, None) == 0
    # unload, reload: a new id, the same bytes; the old id is gone
    ctx.ecdsa_unload_signers(t1)
    assert _sign_packed(ctx, t1, idx, msgs)[0] == EINVAL
    assert lib.cbft_ecdsa_unload_signers(h, t1) == EINVAL
    t2 = ctx.ecdsa_load_signers(keys)
    assert t2 != t1
    rc, got = _sign_packed(ctx, t2, idx, msgs)
    assert rc == 0 and np.array_equal(got, exp)
    ctx.ecdsa_unload_signers(t2)
    # a two-shard context signs on its first device and equals a single device; closing it with the
    # table still loaded is fine
    with cb.Context(devices=[0, 0]) as two:
        t3 = two.ecdsa_load_signers(keys)
        rc, got = _sign_packed(two, t3, idx, msgs)
        assert rc == 0 and np.array_equal(got, exp)
        assert two.ecdsa_signer_public_keys(t3, 2).tobytes() == b"".join(sref.public_key(x) for x in privs)
        assert two.lib.cbft_ecdsa_sign_fixed_device(two.handle, t3, None, None, 0, 0, None, None) == EINVAL


# ------------------------------------------------------------------------------------------
# the lane routines on chosen inputs, one function per launch (tests/hip/ecdsa_sign_selftest.hip);
# the operand sets are the CPU test's
# ------------------------------------------------------------------------------------------
ESS_OUT = 24
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def selftest():
    path = os.path.join(HERE, "hip", "libecdsa_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/libecdsa_sign_selftest.so not built (make selftest)"
    lib = ctypes.CDLL(path)

    def run(op, a, b=None, c=None):
        """Rows of (first result, second result, flag) as integers; fails if a lane wrote nothing."""
        n = len(a)
        words = lambda v: np.frombuffer(b"".join(int(t).to_bytes(32, "little") for t in v), dtype=np.uint32).copy()  # noqa: E731
        p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        wa, wb, wc = words(a), words(b if b is not None else a), words(c if c is not None else a)
        out = np.full(n * ESS_OUT, SENTINEL, dtype=np.uint32)
        assert lib.ecdsa_sign_selftest(op, p(wa), p(wb), p(wc), p(out), n) == 0
        out = out.reshape(n, ESS_OUT)
        assert not (out == SENTINEL).all(axis=1).any(), "a lane left its output unwritten"
        assert not out[:, 17:].any()
        val = lambda row: int.from_bytes(row.tobytes(), "little")  # noqa: E731
        return [(val(r[:8]), val(r[8:16]), int(r[16])) for r in out]

    return run


def test_lane_nonce_retry_path_on_the_gpu(selftest):
    from test_ecdsa_sign_cpu import TEST_ORDER
    rng = random.Random(0x6979)
    xs, hs, exp = [], [], []
    for _ in range(200):
        x, h = rng.randrange(1, TEST_ORDER), rng.getrandbits(256)
        xs.append(x), hs.append(h)
        exp.append(sref.nonce(x, be(h), TEST_ORDER, with_rejections=True))
    got = selftest(0, xs, hs, [TEST_ORDER] * 200)
    assert [(k, f) for k, _, f in got] == exp
    assert 60 <= sum(1 for _, f in exp if f) <= 140
    # and the product's order with digests at and above it
    hs = [0, 1, N - 1, N, N + 1, FULL] + [rng.getrandbits(256) for _ in range(58)]
    xs = [rng.randrange(1, N) for _ in hs]
    got = selftest(0, xs, hs, [N] * len(hs))
    assert [(k, f) for k, _, f in got] == [sref.nonce(x, be(h), N, with_rejections=True) for x, h in zip(xs, hs)]


def test_lane_sign_with_chosen_nonces_on_the_gpu(selftest):
    from test_ecdsa_sign_cpu import edge_nonces
    rng = random.Random(0xC0FFEE)
    ks = edge_nonces()
    xs = [rng.randrange(1, N) if i % 3 else N - 1 for i in range(len(ks))]
    es = [rng.randrange(N) if i % 3 else N - 1 for i in range(len(ks))]
    # s = 0: e = -r x reports "next candidate"
    for _ in range(4):
        x, k = rng.randrange(1, N), rng.randrange(1, N)
        ks.append(k), xs.append(x), es.append(-(ref.mul(k, ref.G)[0] % N) * x % N)
    got = selftest(1, xs, es, ks)
    for (r, s, ok), x, e, k in zip(got, xs, es, ks):
        want = sref.sign_with_k(x, e, k)
        assert (r, s, ok) == ((want[0], want[1], 1) if want else (0, 0, 0)), hex(k)
    assert [ok for _, _, ok in got[-4:]] == [0, 0, 0, 0]


def test_lane_comb_and_inversions_on_the_gpu(selftest):
    from test_ecdsa_sign_cpu import edge_nonces
    eights = int("8" * 64, 16)
    ks = edge_nonces() + [FULL, FULL - 1, N + 1, (1 << 256) - eights, (1 << 256) - eights - 1, 0, N]
    got = selftest(2, ks)
    for (x, y, inf), k in zip(got, ks):
        pt = ref.mul(k % N, ref.G)
        assert (x, y, inf) == ((0, 0, 1) if pt is ref.INF else (pt[0], pt[1], 0)), hex(k)
    rng = random.Random(0x1A7)
    for op, mod in ((3, ref.P), (4, N)):
        ops = [0, 1, 2, 3, mod - 1, mod - 2, mod - 3, FULL % mod, (1 << 255) % mod, (1 << 128) - 1, 1 << 32, 977, mod >> 1]
        ops += [(v + d) % mod for v in (0, mod - 1, FULL) for d in range(-20, 21)]
        ops += [rng.randrange(mod) for _ in range(2000 - len(ops))]
        got = selftest(op, ops)
        bad = [hex(a) for (r, _, _), a in zip(got, ops) if r != (pow(a, -1, mod) if a else 0)]
        assert not bad, bad[:5]


def test_batch_scratch_holds_no_nonce_afterwards(pool):
    """The product's three launches on a scratch the harness owns (filled with 0xA5 before): the
    signatures are the restatement's, the digests in the scratch show that it was used, and the
    nonce words and the state words read back as zeros.  Sizes 8 / 300 / 8: the scratch of the large
    batch does not leak into the small one after it."""
    import hashlib
    path = os.path.join(HERE, "hip", "libecdsa_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/libecdsa_sign_selftest.so not built (make selftest)"
    lib = ctypes.CDLL(path)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    privs = pool["privs"][:5] + [0]  # the last signer is unusable
    keys = np.frombuffer(b"".join(be(x) for x in privs), dtype=np.uint8)
    rng = np.random.default_rng(0x5C7A)
    L = 40
    for n in (8, 300, 8):
        blob = rng.integers(0, 256, size=n * L, dtype=np.uint8)
        idx = rng.integers(0, len(privs), size=n).astype(np.uint32)
        idx[n - 1] = len(privs) + 3  # no such signer
        sig = np.full((n, 64), 0xC3, dtype=np.uint8)
        scr = np.full(17 * n, 0xC3C3C3C3, dtype=np.uint32)
        assert lib.ecdsa_sign_selftest_batch(p(keys), len(privs), p(idx), p(blob), L, n, p(sig), p(scr)) == 0
        k, h1, state = scr[:8 * n].reshape(8, n), scr[8 * n:16 * n].reshape(8, n), scr[16 * n:]
        assert not k.any(), "nonces left in the scratch"
        assert not state.any()
        for i in range(n):
            m = blob[i * L:(i + 1) * L].tobytes()
            if idx[i] >= len(privs) or privs[idx[i]] == 0:
                assert not sig[i].any() and not h1[:, i].any()
            else:
                assert sig[i].tobytes() == sref.sign(privs[idx[i]], m), (n, i)
                assert b"".join(int(w).to_bytes(4, "big") for w in h1[:, i]) == hashlib.sha256(m).digest()
