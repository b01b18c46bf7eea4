"""GPU tests of the batched ECDSA P-256 / SHA-256 signing through the C ABI
(cbft_ecdsa_load_signers_curve with CBFT_CURVE_P256): every signature must equal tests/p256_sign_ref.py's
(RFC 6979 nonces, r || s, no low-s rule) byte for byte, and be accepted by cbft_ecdsa_verify_batch on a
P-256 key table and by OpenSSL on prime256v1."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import cbft_hipcrypto as cb
import ecdsa_ref as k1ref
import ecdsa_sign_ref as k1sref
import p256_ref as ref
import p256_sign_ref as sref
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P, N = ref.P, ref.N
FULL = (1 << 256) - 1
EIGHTS = int("8" * 64, 16)
EINVAL, E2BIG = -22, -7
NSIGNERS = 37
POOL = 1000
TEST_ORDER = (1 << 255) + 0x1B3  # the secp256k1 harness's: rejects about half of all candidates


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def openssl():
    path = os.path.join(ROOT, "tools", "cpu_baseline", "libcbft_cpu_openssl_ecdsa_p256.so")
    assert os.path.exists(path), "tools/cpu_baseline/libcbft_cpu_openssl_ecdsa_p256.so not built (make cpu)"
    lib = ctypes.CDLL(path)
    lib.cbft_cpu_p256_keys_new.restype = ctypes.c_void_p

    def verify(pubs: np.ndarray, kidx, sigs: np.ndarray, msgs, threads=16) -> np.ndarray:
        """OpenSSL's ECDSA_do_verify verdict (prime256v1) of every signature."""
        pubs = np.ascontiguousarray(pubs, dtype=np.uint8).reshape(-1, 64)
        kidx = np.ascontiguousarray(np.asarray(kidx, dtype=np.uint32))
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
        blob, off, lens = cb.pack_messages(msgs)
        n = len(msgs)
        out = np.zeros(max(1, n), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        cache = ctypes.c_void_p(lib.cbft_cpu_p256_keys_new(p(pubs), ctypes.c_uint32(pubs.shape[0])))
        assert cache
        lib.cbft_cpu_p256_verify(cache, p(kidx), p(sigs), p(blob), p(off), p(lens), ctypes.c_size_t(n), p(out),
                                 ctypes.c_int(threads))
        lib.cbft_cpu_p256_keys_free(cache, ctypes.c_uint32(pubs.shape[0]))
        return out[:n].astype(bool)

    return verify


@pytest.fixture(scope="module")
def shim():
    path = os.path.join(HERE, "cpp", "libecdsa_p256_sign_shim.so")
    assert os.path.exists(path), "tests/cpp/libecdsa_p256_sign_shim.so not built (make ecdsa_p256_sign_shim)"
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def pool():
    """1,000 messages of 0..300 bytes over 37 signers with the restatement's signature of each.  Built
    once; the batch tests take prefixes of it."""
    rng = random.Random(0xEC5256)
    privs = [rng.randrange(1, N) for _ in range(NSIGNERS)]
    idx = [rng.randrange(NSIGNERS) for _ in range(POOL)]
    msgs = [rng.randbytes(rng.randrange(0, 301)) for _ in range(POOL)]
    exp = np.frombuffer(b"".join(sref.sign(privs[i], m) for i, m in zip(idx, msgs)), dtype=np.uint8).reshape(POOL, 64)
    return {"privs": privs, "idx": idx, "msgs": msgs, "exp": exp}


@pytest.fixture(scope="module")
def pool_table(ctx, pool):
    tid = ctx.ecdsa_load_signers([be(x) for x in pool["privs"]], curve="p256")
    assert ctx.ecdsa_signer_status(tid, NSIGNERS).all()
    yield tid
    ctx.ecdsa_unload_signers(tid)


def test_golden_vectors(ctx):
    vecs = json.load(open(os.path.join(HERE, "golden", "ecdsa_p256_sign_vectors.json")))["vectors"]
    xs = sorted({v["x"] for v in vecs})
    tid = ctx.ecdsa_load_signers([bytes.fromhex(x) for x in xs], curve="p256")
    got = ctx.ecdsa_sign(tid, [bytes.fromhex(v["msg"]) for v in vecs], [xs.index(v["x"]) for v in vecs])
    bad = [i for i, v in enumerate(vecs) if got[i].tobytes().hex() != v["sig"]]
    assert not bad, bad[:10]
    ctx.ecdsa_unload_signers(tid)


def edge_keys():
    keys = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255, EIGHTS % N, N - EIGHTS, (1 << 256) - EIGHTS,
            (1 << 256) - EIGHTS - 1, int("7" * 64, 16), int("7" * 64, 16) + 1]
    for j in range(64):
        keys += [16**j, 16**j - 1, 8 * 16**j]
    return [k for k in dict.fromkeys(keys) if 0 < k < N]


def test_public_keys_of_edge_scalars(ctx):
    """x G for scalars that drive the comb's recoding to its corners: chosen scalars on the GPU."""
    keys = edge_keys()
    tid = ctx.ecdsa_load_signers([be(x) for x in keys], curve="p256")
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
    tid = ctx.ecdsa_load_signers([be(x) for x in keys], curve="p256")
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
    vt = ctx.ecdsa_load_keys(pub, curve="p256")
    try:
        assert cb.bitmap_to_bools(ctx.ecdsa_verify(vt, idx, got, msgs), n).all()
    finally:
        ctx.ecdsa_unload_keys(vt)
    assert openssl(pub, idx, got, msgs).all()


def test_fixed_batch_equals_the_host_build(ctx, pool, pool_table, openssl, shim):
    """8,193 x 32 B (129 blocks, the last with one lane): every signature equal to the host build of the lane
    code and accepted by OpenSSL; 64 sampled ones equal the restatement's."""
    n, L = 8193, 32
    rng = np.random.default_rng(0x2001)
    blob = rng.integers(0, 256, size=n * L, dtype=np.uint8)
    idx = rng.integers(0, NSIGNERS, size=n).astype(np.uint32)
    msgs = [blob[i * L:(i + 1) * L].tobytes() for i in range(n)]
    got = ctx.ecdsa_sign(pool_table, msgs, idx)
    privs = np.frombuffer(b"".join(be(x) for x in pool["privs"]), dtype=np.uint8)
    host = np.zeros((n, 64), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    shim.ecdsa_p256_sign_shim_sign_many(p(privs), p(idx), p(blob), ctypes.c_uint32(L), ctypes.c_size_t(n), p(host),
                                        ctypes.c_int(16))
    bad = np.nonzero((got != host).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} differ from the host build, first {bad[:8]}"
    pub = ctx.ecdsa_signer_public_keys(pool_table, NSIGNERS)
    ok = openssl(pub, idx, got, msgs)
    assert ok.all(), np.nonzero(~ok)[0][:8]
    for i in rng.choice(n, size=64, replace=False):
        assert got[i].tobytes() == sref.sign(pool["privs"][idx[i]], msgs[i]), int(i)


def test_both_curves_on_one_context(ctx, pool):
    """A secp256k1 and a P-256 signer table side by side, signing alternately: each keeps its own bytes, and neither
    curve's verifier takes the other's signatures under the same scalar's key."""
    xs = pool["privs"][:5]
    keys = [be(x) for x in xs]
    tk = ctx.ecdsa_load_signers(keys)
    tp = ctx.ecdsa_load_signers(keys, curve="p256")
    assert tk != tp
    assert ctx.ecdsa_signer_public_keys(tk, 5).tobytes() == b"".join(k1sref.public_key(x) for x in xs)
    assert ctx.ecdsa_signer_public_keys(tp, 5).tobytes() == b"".join(sref.public_key(x) for x in xs)
    rng = random.Random(0xB07)
    sigs = {tk: [], tp: []}
    batches = []
    for rnd in range(3):
        msgs = [rng.randbytes(rng.randrange(0, 100)) for _ in range(40 + rnd)]
        idx = [rng.randrange(5) for _ in msgs]
        batches.append((msgs, idx))
        for t in (tk, tp) if rnd % 2 == 0 else (tp, tk):
            sigs[t].append(ctx.ecdsa_sign(t, msgs, idx))
    for j, (msgs, idx) in enumerate(batches):
        assert sigs[tk][j].tobytes() == b"".join(k1sref.sign(xs[i], m) for i, m in zip(idx, msgs))
        assert sigs[tp][j].tobytes() == b"".join(sref.sign(xs[i], m) for i, m in zip(idx, msgs))
    vk = ctx.ecdsa_load_keys(ctx.ecdsa_signer_public_keys(tk, 5))
    vp = ctx.ecdsa_load_keys(ctx.ecdsa_signer_public_keys(tp, 5), curve="p256")
    assert ctx.ecdsa_key_status(vk, 5).all() and ctx.ecdsa_key_status(vp, 5).all()
    msgs, idx = batches[0]
    n = len(msgs)
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(vk, idx, sigs[tk][0], msgs), n).all()
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(vp, idx, sigs[tp][0], msgs), n).all()
    assert not cb.bitmap_to_bools(ctx.ecdsa_verify(vk, idx, sigs[tp][0], msgs), n).any()
    assert not cb.bitmap_to_bools(ctx.ecdsa_verify(vp, idx, sigs[tk][0], msgs), n).any()
    for t in (vk, vp):
        ctx.ecdsa_unload_keys(t)
    # unloading one curve's table leaves the other's in place
    ctx.ecdsa_unload_signers(tk)
    assert ctx.ecdsa_sign(tp, batches[1][0], batches[1][1]).tobytes() == sigs[tp][1].tobytes()
    ctx.ecdsa_unload_signers(tp)


def test_device_entry_two_streams_growing_and_bad_index(ctx, pool, pool_table):
    """cbft_ecdsa_sign_fixed_device on two streams that share the context's nonce scratch (the library
    orders them), batch sizes 8 / 300 / 8 so that the scratch grows and shrinks, against the
    restatement; an out-of-range d_signer_idx entry gives 64 zero bytes with exact neighbours; a null index
    array signs everything with signer 0."""
    hip = Hip()
    L = 48
    rng = np.random.default_rng(0xDE8)
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
    CURVE = 1
    privs = pool["privs"][:2]
    keys = np.frombuffer(b"".join(be(x) for x in privs), dtype=np.uint8)
    msgs = [b"a", b"", b"ccc", b"dddd" * 20]
    idx = np.array([0, 1, 1, 0], dtype=np.uint32)
    exp = np.frombuffer(b"".join(sref.sign(privs[i], m) for i, m in zip(idx, msgs)), dtype=np.uint8).reshape(4, 64)
    lib, h = ctx.lib, ctx.handle
    tid = ctypes.c_uint32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    load = lib.cbft_ecdsa_load_signers_curve
    # an unknown curve is EINVAL before anything else; then E2BIG, then the null and empty cases
    for curve in (2, -1, 255):
        assert load(h, curve, p(keys), 2, ctypes.byref(tid)) == EINVAL
    assert load(h, 2, None, (1 << 20) + 1, ctypes.byref(tid)) == EINVAL
    assert load(h, CURVE, None, (1 << 20) + 1, ctypes.byref(tid)) == E2BIG
    assert load(h, CURVE, None, 2, ctypes.byref(tid)) == EINVAL
    assert load(h, CURVE, p(keys), 0, ctypes.byref(tid)) == EINVAL
    assert load(h, CURVE, p(keys), 2, None) == EINVAL
    with pytest.raises(ValueError):
        ctx.ecdsa_load_signers(keys, curve="p384")
    t1 = ctx.ecdsa_load_signers(keys, curve="p256")
    rc, got = _sign_packed(ctx, t1, idx, msgs)
    assert rc == 0 and np.array_equal(got, exp)
    # batch: E2BIG before EINVAL; unknown table; n = 0 answered after the table lookup
    assert _sign_packed(ctx, t1, None, msgs, n=(1 << 26) + 1)[0] == E2BIG
    assert lib.cbft_ecdsa_sign_batch(h, t1, None, None, None, None, ctypes.c_size_t(4), None) == EINVAL
    assert _sign_packed(ctx, t1 + 1000, idx, msgs)[0] == EINVAL
    assert _sign_packed(ctx, t1, None, [])[0] == 0
    out = np.full((4, 64), 0xC3, dtype=np.uint8)
    rc, _ = _sign_packed(ctx, t1, np.array([0, 1, 2, 0], dtype=np.uint32), msgs, out=out)
    assert rc == EINVAL and (out == 0xC3).all(), "host index out of range: refused before any launch"
    # device entry: E2BIG first, then null and alignment checks (a misaligned d_sig is refused before any launch)
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 0, ctypes.c_size_t((1 << 26) + 1), None, None) == E2BIG
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 32, ctypes.c_size_t(4), None, None) == EINVAL
    hip = Hip()
    try:
        d_msg = hip.to_dev(np.zeros(4 * 32, dtype=np.uint8))
        d_sig = hip.to_dev(np.full(4 * 64 + 8, 0xA5, dtype=np.uint8))
        for skew in (1, 2, 3):
            assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, ctypes.c_void_p(d_msg), 32, ctypes.c_size_t(4),
                                                    ctypes.c_void_p(d_sig + skew), None) == EINVAL
        hip.sync()
        assert (hip.from_dev(d_sig, 4 * 64 + 8) == 0xA5).all()
    finally:
        hip.close()
    assert lib.cbft_ecdsa_sign_fixed_device(h, t1, None, None, 0, ctypes.c_size_t(0), None, None) == 0
    # unload, reload: a new id, the same bytes; the old id is gone
    ctx.ecdsa_unload_signers(t1)
    assert _sign_packed(ctx, t1, idx, msgs)[0] == EINVAL
    assert lib.cbft_ecdsa_unload_signers(h, t1) == EINVAL
    assert lib.cbft_ecdsa_signer_status(h, t1, p(out)) == EINVAL
    t2 = ctx.ecdsa_load_signers(keys, curve="p256")
    assert t2 != t1
    rc, got = _sign_packed(ctx, t2, idx, msgs)
    assert rc == 0 and np.array_equal(got, exp)
    ctx.ecdsa_unload_signers(t2)
    # a two-shard context signs on its first device and equals a single device; closing it with the
    # table still loaded is fine
    with cb.Context(devices=[0, 0]) as two:
        t3 = two.ecdsa_load_signers(keys, curve="p256")
        rc, got = _sign_packed(two, t3, idx, msgs)
        assert rc == 0 and np.array_equal(got, exp)
        assert two.ecdsa_signer_public_keys(t3, 2).tobytes() == b"".join(sref.public_key(x) for x in privs)
        assert two.lib.cbft_ecdsa_sign_fixed_device(two.handle, t3, None, None, 0, 0, None, None) == EINVAL


# ------------------------------------------------------------------------------------------
# the lane routines on chosen inputs, one function per launch (tests/hip/ecdsa_p256_sign_selftest.hip)
# ------------------------------------------------------------------------------------------
P2T_OUT = 32
SENTINEL = 0xA5A5A5A5


def word_patterns(mod: int):
    base = 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    out = []
    for pos in range(8):
        m = 0xFFFFFFFF << (32 * pos)
        out += [(base | m) % mod, (base & ~m) % mod, m % mod, (FULL & ~m) % mod]
    return out


def operands(mod: int, rng, count: int):
    ops = [0, 1, 2, mod - 1, mod - 2, FULL % mod, (1 << 255) % mod, (1 << 128) - 1, 1 << 32, mod >> 1] + word_patterns(mod)
    ops += [(v + d) % mod for v in (0, mod - 1, FULL) for d in range(-8, 9)]
    return ops + [rng.randrange(mod) for _ in range(count)]


def edge_nonces():
    ks = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255]
    for j in range(64):
        ks += [16**j, 16**j - 1, 8 * 16**j]
    ks += [(0 - EIGHTS) % (1 << 256), int("F" * 64, 16) - EIGHTS, N - EIGHTS]
    for j in (0, 1, 31, 62, 63):
        ks += [7 * 16**j, (1 << 256) - 8 * 16**j]
    return ks


@pytest.fixture(scope="module")
def selftest():
    path = os.path.join(HERE, "hip", "libecdsa_p256_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/libecdsa_p256_sign_selftest.so not built (make selftest)"
    lib = ctypes.CDLL(path)

    def run(op, *cols):
        """Rows of (first, second, third result, flag) as integers; fails if a lane wrote nothing."""
        n = len(cols[0])
        words = lambda v: np.frombuffer(b"".join(int(t).to_bytes(32, "little") for t in v), dtype=np.uint32).copy()  # noqa: E731
        p = lambda v: None if v is None else v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        w = [words(c) for c in cols] + [None] * (5 - len(cols))
        out = np.full(n * P2T_OUT, SENTINEL, dtype=np.uint32)
        assert lib.ecdsa_p256_sign_selftest(op, p(w[0]), p(w[1]), p(w[2]), p(w[3]), p(w[4]), p(out), n) == 0
        out = out.reshape(n, P2T_OUT)
        assert not (out == SENTINEL).all(axis=1).any(), "a lane left its output unwritten"
        assert not out[:, 25:].any()
        val = lambda row: int.from_bytes(row.tobytes(), "little")  # noqa: E731
        return [(val(r[:8]), val(r[8:16]), val(r[16:24]), int(r[24])) for r in out]

    return run


def test_lane_complete_addition_on_the_gpu(selftest):
    rng = random.Random(0xADD)
    pts = [ref.mul(rng.randrange(1, N), ref.G) for _ in range(60)] + [ref.G, ref.mul(N - 1, ref.G)]
    X, Y, Z, QX, QY, want = [], [], [], [], [], []

    def case(p3, q, expect):
        X.append(p3[0]), Y.append(p3[1]), Z.append(p3[2]), QX.append(q[0]), QY.append(q[1]), want.append(expect)

    for i, q in enumerate(pts):
        case((0, 1, 0), q, q)                                 # P = infinity
        case((0, rng.randrange(1, P), 0), q, q)
        for z in (1, P - 1, rng.randrange(1, P), rng.randrange(1, P)):
            case((q[0] * z % P, q[1] * z % P, z), q, ref.add(q, q))              # P = Q
            case((q[0] * z % P, (P - q[1]) * z % P, z), q, ref.INF)              # P = -Q: Z3 = 0
            p = pts[(i + 7) % len(pts)]
            case((p[0] * z % P, p[1] * z % P, z), q, ref.add(p, q))              # random P, random Z
    got = selftest(7, X, Y, Z, QX, QY)
    assert len(got) >= 300
    for (x3, y3, z3, _), expect in zip(got, want):
        if expect is ref.INF:
            assert z3 == 0 and x3 == 0 and y3 != 0
        else:
            zi = pow(z3, -1, P)
            assert (x3 * zi % P, y3 * zi % P) == expect


def test_lane_field_and_scalar_helpers_on_the_gpu(selftest):
    rng = random.Random(0x1A8)
    for op, mod in ((3, P), (4, N)):
        ops = operands(mod, rng, 400)
        got = selftest(op, ops)
        bad = [hex(a) for (r, _, _, _), a in zip(got, ops) if r != (pow(a, -1, mod) if a else 0)]
        assert not bad, (op, bad[:5])
    ops = operands(P, rng, 300)
    assert [r for r, _, _, _ in selftest(5, ops)] == [ref.B * a % P for a in ops]
    ops = [0, 1, N - 1, N, N + 1, P - 1, (N + P) // 2] + [rng.randrange(P) for _ in range(200)] + \
          [N + rng.randrange(P - N) for _ in range(50)]
    assert [r for r, _, _, _ in selftest(6, ops)] == [a % N for a in ops]


def test_lane_comb_on_the_gpu(selftest):
    ks = edge_nonces() + [FULL, FULL - 1, N + 1, (1 << 256) - EIGHTS - 1, 0, N]
    got = selftest(2, ks)
    for (x, y, _, inf), k in zip(got, ks):
        pt = ref.mul(k % N, ref.G)
        assert (x, y, inf) == ((0, 0, 1) if pt is ref.INF else (pt[0], pt[1], 0)), hex(k)


def test_lane_sign_with_chosen_nonces_and_the_s_zero_retry_on_the_gpu(selftest):
    rng = random.Random(0xC0FFEF)
    ks = [k % N for k in edge_nonces() if k % N]
    xs = [rng.randrange(1, N) if i % 3 else N - 1 for i in range(len(ks))]
    es = [rng.randrange(N) if i % 3 else N - 1 for i in range(len(ks))]
    for _ in range(4):  # s = 0: e = -r x reports "next candidate"
        x, k = rng.randrange(1, N), rng.randrange(1, N)
        ks.append(k), xs.append(x), es.append(-(ref.mul(k, ref.G)[0] % N) * x % N)
    got = selftest(1, xs, es, ks)
    for (r, s, _, ok), x, e, k in zip(got, xs, es, ks):
        want = sref.sign_with_k(x, e, k)
        if want:
            assert (r, s, ok) == (want[0], want[1], 1), hex(k)
        else:
            assert (r, s, ok) == (ref.mul(k, ref.G)[0] % N, 0, 0), hex(k)
    assert [ok for _, _, _, ok in got[-4:]] == [0, 0, 0, 0]
    # the lane routine with e = -r x under the first nonce passes on to the next candidate; beside lanes that do not
    xs, hs, es, want = [], [], [], []
    for i in range(64):
        x, h = rng.randrange(1, N), rng.getrandbits(256)
        e = h % N
        if i % 4 == 1:
            e = -(ref.mul(sref.nonce(x, be(h)), ref.G)[0] % N) * x % N
        k, r, s = sref.sign_digest(x, be(h), e=e)
        assert (k != sref.nonce(x, be(h))) == (i % 4 == 1)
        xs.append(x), hs.append(h), es.append(e), want.append((r, s))
    got = selftest(8, xs, hs, es)
    assert [(r, s) for r, s, _, _ in got] == want


def test_lane_nonce_retry_path_on_the_gpu(selftest):
    rng = random.Random(0x6980)
    xs, hs, exp = [], [], []
    for _ in range(200):
        x, h = rng.randrange(1, TEST_ORDER), rng.getrandbits(256)
        xs.append(x), hs.append(h)
        exp.append(k1sref.nonce(x, be(h), TEST_ORDER, with_rejections=True))
    got = selftest(0, xs, hs, [TEST_ORDER] * 200)
    assert [(k, f) for k, _, _, f in got] == exp
    assert 60 <= sum(1 for _, f in exp if f) <= 140
    # and P-256's order with digests at and above it
    hs = [0, 1, N - 1, N, N + 1, FULL] + [rng.getrandbits(256) for _ in range(58)]
    xs = [rng.randrange(1, N) for _ in hs]
    got = selftest(0, xs, hs, [N] * len(hs))
    assert [(k, f) for k, _, _, f in got] == [sref.nonce(x, be(h), with_rejections=True) for x, h in zip(xs, hs)]


def test_batch_scratch_holds_no_nonce_afterwards(pool):
    """The product's three launches on a scratch the harness owns (filled with 0xA5 before): the
    signatures are the restatement's, the digests in the scratch show that it was used, and the
    nonce words and the state words read back as zeros.  Sizes 8 / 300 / 8."""
    path = os.path.join(HERE, "hip", "libecdsa_p256_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/libecdsa_p256_sign_selftest.so not built (make selftest)"
    lib = ctypes.CDLL(path)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    privs = pool["privs"][:5] + [0]  # the last signer is unusable
    keys = np.frombuffer(b"".join(be(x) for x in privs), dtype=np.uint8)
    rng = np.random.default_rng(0x5C7B)
    L = 40
    for n in (8, 300, 8):
        blob = rng.integers(0, 256, size=n * L, dtype=np.uint8)
        idx = rng.integers(0, len(privs), size=n).astype(np.uint32)
        idx[n - 1] = len(privs) + 3  # no such signer
        sig = np.full((n, 64), 0xC3, dtype=np.uint8)
        scr = np.full(17 * n, 0xC3C3C3C3, dtype=np.uint32)
        assert lib.ecdsa_p256_sign_selftest_batch(p(keys), len(privs), p(idx), p(blob), L, n, p(sig), p(scr)) == 0
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
