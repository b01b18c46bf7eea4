"""GPU tests of the ECDSA P-256 / SHA-256 batch verify through the C ABI (cbft_ecdsa_load_keys_curve with
CBFT_CURVE_P256, then the same cbft_ecdsa_* calls): every verdict must equal OpenSSL's on the golden
vectors (tests/golden/ecdsa_p256_vectors.json) and the restatement's (tests/p256_ref.py) on generated
batches, and a secp256k1 table on the same context must keep its verdicts."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import cbft_hipcrypto as cb
import ecdsa_ref as k1ref
import p256_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = ref.N
NKEYS = 96
POOL = 1000
USABLE_KEY_CLASSES = ("key_x_zero",)  # classes named key_* whose key OpenSSL loads


def _load(name):
    g = json.load(open(os.path.join(HERE, "golden", name)))
    g["keys"] = [bytes.fromhex(k) for k in g["keys"]]
    for v in g["vectors"]:
        v["sig"], v["msg"] = bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])
    return g


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return _load("ecdsa_p256_vectors.json")


@pytest.fixture(scope="module")
def golden_k1():
    return _load("ecdsa_vectors.json")


@pytest.fixture(scope="module")
def pool():
    """1,000 signatures over 96 keys and messages of 0..300 bytes, one in ten damaged (r, s, the
    message or the key index, in turn), with the restatement's verdict for each.  Built once; the
    batch tests take prefixes of it.  Nonces step by one so that each R costs one point addition."""
    rng = random.Random(0x9256A)
    privs = [rng.randrange(1, N) for _ in range(NKEYS)]
    pubs = [ref.pub_bytes(ref.mul(d, ref.G)) for d in privs]
    k = rng.randrange(1, N - POOL)
    R = ref.mul(k, ref.G)
    kidx, sigs, msgs = [], [], []
    for i in range(POOL):
        ki = rng.randrange(NKEYS)
        m = rng.randbytes(rng.randrange(0, 301))
        r = R[0] % N
        s = pow(k, -1, N) * (ref.digest_int(m) + r * privs[ki]) % N
        assert r and s
        k, R = k + 1, ref.add(R, ref.G)
        if i % 10 == 7:
            kind = (i // 10) % 4
            if kind == 0:
                r ^= 1 << rng.randrange(256)
            elif kind == 1:
                s ^= 1 << rng.randrange(256)
            elif kind == 2:
                m = m + b"!"
            else:
                ki = (ki + 1) % NKEYS
        kidx.append(ki), sigs.append(ref.sig_bytes(r, s)), msgs.append(m)
    exp = np.array([ref.verify(pubs[ki], s, m) for ki, s, m in zip(kidx, sigs, msgs)])
    assert exp[0] and exp.sum() >= POOL * 0.9 - 1 and (~exp).sum() >= POOL // 10 - 1
    return {"pubs": pubs, "kidx": kidx, "sigs": sigs, "msgs": msgs, "exp": exp}


@pytest.fixture(scope="module")
def pool_table(ctx, pool):
    tid = ctx.ecdsa_load_keys(pool["pubs"], curve="p256")
    assert ctx.ecdsa_key_status(tid, NKEYS).all()
    yield tid
    ctx.ecdsa_unload_keys(tid)


def _mismatches(vecs, got):
    exp = np.array([bool(v["ok"]) for v in vecs])
    by_class = {}
    for i in np.nonzero(got != exp)[0]:
        by_class.setdefault(vecs[i]["cls"], []).append((int(i), bool(got[i])))
    return by_class


def _run(ctx, tid, vecs):
    bm = ctx.ecdsa_verify(tid, [v["key"] for v in vecs], [v["sig"] for v in vecs], [v["msg"] for v in vecs])
    return cb.bitmap_to_bools(bm, len(vecs))


def test_golden_vectors(ctx, golden):
    keys, vecs = golden["keys"], golden["vectors"]
    tid = ctx.ecdsa_load_keys(keys, curve="p256")
    by_class = _mismatches(vecs, _run(ctx, tid, vecs))
    assert not by_class, by_class
    # key_status agrees with OpenSSL's refusal of the key
    st = ctx.ecdsa_key_status(tid, len(keys))
    refused = {v["key"] for v in vecs if v["cls"].startswith("key_") and v["cls"] not in USABLE_KEY_CLASSES}
    assert refused and [not s for s in st] == [k in refused for k in range(len(keys))]
    x_zero = {v["key"] for v in vecs if v["cls"] == "key_x_zero"}
    assert len(x_zero) == 2 and all(st[k] for k in x_zero)
    ctx.ecdsa_unload_keys(tid)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_ragged_batches_vs_restatement(ctx, pool, pool_table, n):
    got = cb.bitmap_to_bools(ctx.ecdsa_verify(pool_table, pool["kidx"][:n], pool["sigs"][:n], pool["msgs"][:n]), n)
    exp = pool["exp"][:n]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert exp.sum() > 0
    if n >= 63:
        assert (~exp).sum() > 0


def test_mixed_keys_and_edge_vectors_within_a_wave(ctx, golden, pool):
    """256 items over 96 + the fixture's keys: edge vectors interleaved among valid signatures, so
    that lanes of one wave run different keys and different branches; each verdict must equal the
    same item verified alone (no verdict depends on its neighbours)."""
    keys = pool["pubs"] + golden["keys"]
    edge = [v for v in golden["vectors"] if v["cls"] not in ("valid", "high_s_twin") and len(v["msg"]) < 512]
    kidx, sigs, msgs, exp = [], [], [], []
    e = 0
    for i in range(256):
        if i % 3 == 1 and e < len(edge):
            v = edge[e]
            e += 1
            kidx.append(NKEYS + v["key"]), sigs.append(v["sig"]), msgs.append(v["msg"]), exp.append(bool(v["ok"]))
        else:
            kidx.append(pool["kidx"][i]), sigs.append(pool["sigs"][i]), msgs.append(pool["msgs"][i])
            exp.append(bool(pool["exp"][i]))
    assert e >= 80 and len({k for k in kidx[:64]}) > 32
    tid = ctx.ecdsa_load_keys(keys, curve="p256")
    got = cb.bitmap_to_bools(ctx.ecdsa_verify(tid, kidx, sigs, msgs), 256)
    assert np.array_equal(got, np.array(exp)), np.nonzero(got != np.array(exp))[0][:10]
    alone = [cb.bitmap_to_bools(ctx.ecdsa_verify(tid, [kidx[i]], [sigs[i]], [msgs[i]]), 1)[0] for i in range(256)]
    assert np.array_equal(got, np.array(alone))
    ctx.ecdsa_unload_keys(tid)


def test_tables_of_both_curves_interleaved_on_one_context(ctx, golden, golden_k1):
    """A secp256k1 table and a P-256 table, verified in consecutive calls in turn: neither bleeds into the
    other (G's table, the records, the digest scratch), and ids share one space."""
    t_k1 = ctx.ecdsa_load_keys(golden_k1["keys"])
    t_p = ctx.ecdsa_load_keys(golden["keys"], curve="p256")
    t_k1b = ctx.ecdsa_load_keys(golden_k1["keys"], curve="secp256k1")
    assert len({t_k1, t_p, t_k1b}) == 3
    for _ in range(2):
        assert not _mismatches(golden_k1["vectors"], _run(ctx, t_k1, golden_k1["vectors"]))
        assert not _mismatches(golden["vectors"], _run(ctx, t_p, golden["vectors"]))
        assert not _mismatches(golden_k1["vectors"], _run(ctx, t_k1b, golden_k1["vectors"]))
    for t in (t_k1, t_p, t_k1b):
        ctx.ecdsa_unload_keys(t)


def test_signature_of_the_other_curve_is_a_plain_reject(ctx):
    m = b"which curve"
    dp, dk = 0x9256, 0x256C1
    qp, qk = ref.pub_bytes(ref.mul(dp, ref.G)), k1ref.pub_bytes(k1ref.mul(dk, k1ref.G))
    sp, sk = ref.sig_bytes(*ref.sign(dp, m, 0x1234567)), k1ref.sig_bytes(*k1ref.sign(dk, m, 0x1234567))
    tp = ctx.ecdsa_load_keys([qp, qk], curve="p256")  # the secp256k1 point is not on P-256
    tk = ctx.ecdsa_load_keys([qk, qp])
    assert ctx.ecdsa_key_status(tp, 2).tolist() == [True, False]
    assert ctx.ecdsa_key_status(tk, 2).tolist() == [True, False]
    got_p = cb.bitmap_to_bools(ctx.ecdsa_verify(tp, [0, 0, 1, 1], [sp, sk, sp, sk], [m] * 4), 4)
    got_k = cb.bitmap_to_bools(ctx.ecdsa_verify(tk, [0, 0, 1, 1], [sk, sp, sk, sp], [m] * 4), 4)
    assert got_p.tolist() == [True, False, False, False]
    assert got_k.tolist() == [True, False, False, False]
    ctx.ecdsa_unload_keys(tp)
    ctx.ecdsa_unload_keys(tk)


class _Hip:
    """Device buffers and a stream from the HIP runtime libcbft_hipcrypto itself links (torch ships
    its own runtime, and a second runtime in one process sees no GPUs once the first owns them)."""

    def __init__(self):
        cb.load_library()
        self.lib = ctypes.CDLL("libamdhip64.so.7")  # the soname libcbft_hipcrypto loaded
        self.bufs, self.streams = [], []

    def _ok(self, rc, what):
        assert rc == 0, f"{what}: hipError {rc}"

    def to_dev(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        self._ok(self.lib.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(a.nbytes, 1))), "hipMalloc")
        self.bufs.append(p.value)
        self._ok(self.lib.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1), "hipMemcpy")
        return p.value

    def from_dev(self, ptr: int, nbytes: int) -> np.ndarray:
        out = np.zeros(nbytes, dtype=np.uint8)
        self._ok(self.lib.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes),
                                    2), "hipMemcpy")
        return out

    def stream(self) -> int:
        s = ctypes.c_void_p()
        self._ok(self.lib.hipStreamCreate(ctypes.byref(s)), "hipStreamCreate")
        self.streams.append(s.value)
        return s.value

    def sync(self):
        self._ok(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def close(self):
        self.sync()
        for s in self.streams:
            self.lib.hipStreamDestroy(ctypes.c_void_p(s))
        for b in self.bufs:
            self.lib.hipFree(ctypes.c_void_p(b))


def test_device_entry_on_a_stream_equals_host_entry(ctx, pool, pool_table):
    n = POOL
    nwords = (n + 63) // 64
    host = np.frombuffer(ctx.ecdsa_verify(pool_table, pool["kidx"], pool["sigs"], pool["msgs"]), dtype=np.uint8)
    blob, offs, lens = cb.pack_messages(pool["msgs"])
    hip = _Hip()
    try:
        kidx = np.asarray(pool["kidx"], dtype=np.uint32)
        d_kidx = hip.to_dev(kidx)
        d_sig = hip.to_dev(np.frombuffer(b"".join(pool["sigs"]), dtype=np.uint8))
        d_msg, d_off, d_len = hip.to_dev(blob), hip.to_dev(offs), hip.to_dev(lens)
        d_words = hip.to_dev(np.full(nwords, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
        stream = hip.stream()
        ctx.ecdsa_verify_device(pool_table, d_kidx, d_sig, d_msg, d_off, d_len, n, d_words, stream)
        hip.sync()
        got = hip.from_dev(d_words, nwords * 8)
        assert np.array_equal(got[: n // 8], host[: n // 8])
        assert np.array_equal(cb.bitmap_to_bools(got.tobytes(), nwords * 64)[:n], pool["exp"])
        assert not cb.bitmap_to_bools(got.tobytes(), nwords * 64)[n:].any()  # spare lanes of the last word
        # an out-of-range key index verifies false here (it is CBFT_EINVAL on the host entry)
        kidx2 = kidx.copy()
        kidx2[0] = NKEYS
        d_kidx2 = hip.to_dev(kidx2)
        ctx.ecdsa_verify_device(pool_table, d_kidx2, d_sig, d_msg, d_off, d_len, 64, d_words, stream)
        hip.sync()
        again = hip.from_dev(d_words, 8)
        assert again[0] == got[0] & 0xFE and np.array_equal(again[1:], got[1:8])
        assert pool["exp"][0]
    finally:
        hip.close()


def test_load_unload_reload(ctx):
    m = b"tables"
    sig = ref.sig_bytes(*ref.sign(77, m, 991))
    q77, q78 = ref.pub_bytes(ref.mul(77, ref.G)), ref.pub_bytes(ref.mul(78, ref.G))
    t1 = ctx.ecdsa_load_keys([q77, q78], curve="p256")
    t2 = ctx.ecdsa_load_keys([q78, q77], curve="p256")
    assert t1 != t2
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(t1, [0, 1], [sig, sig], [m, m]), 2).tolist() == [True, False]
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(t2, [0, 1], [sig, sig], [m, m]), 2).tolist() == [False, True]
    ctx.ecdsa_unload_keys(t1)
    with pytest.raises(cb.CbftError) as ei:
        ctx.ecdsa_verify(t1, [0], [sig], [m])
    assert ei.value.code == -22
    with pytest.raises(cb.CbftError):
        ctx.ecdsa_unload_keys(t1)
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(t2, [1], [sig], [m]), 1).tolist() == [True]
    t3 = ctx.ecdsa_load_keys([q77], curve="p256")
    assert cb.bitmap_to_bools(ctx.ecdsa_verify(t3, [0], [sig], [m]), 1).tolist() == [True]
    t0 = ctx.ecdsa_load_keys([], curve="p256")  # an empty table loads; every index is out of range
    assert ctx.ecdsa_key_status(t0, 0).size == 0
    for t in (t2, t3, t0):
        ctx.ecdsa_unload_keys(t)


def test_sharded_context_equals_single_device(pool):
    """A context over two shards (the same GPU twice): tables load on every shard under one id and
    a host-array batch is cut into whole verdict words, one slice per shard."""
    with cb.Context(devices=[0, 0]) as c2:
        tid = c2.ecdsa_load_keys(pool["pubs"], curve="p256")
        assert c2.ecdsa_key_status(tid, NKEYS).all()
        for n in (1, 64, 65, 333):
            got = cb.bitmap_to_bools(c2.ecdsa_verify(tid, pool["kidx"][:n], pool["sigs"][:n], pool["msgs"][:n]), n)
            assert np.array_equal(got, pool["exp"][:n]), n
        with pytest.raises(cb.CbftError):
            c2.ecdsa_verify(tid, [NKEYS], [pool["sigs"][0]], [pool["msgs"][0]])
        c2.ecdsa_unload_keys(tid)
        with pytest.raises(cb.CbftError):
            c2.ecdsa_unload_keys(tid)


def test_argument_errors(ctx, pool, pool_table):
    lib = ctx.lib
    one = np.zeros(64, dtype=np.uint8)
    tid = ctypes.c_uint32()
    for curve in (2, -1, 415):  # an unknown curve id
        assert lib.cbft_ecdsa_load_keys_curve(ctx.handle, curve, one.ctypes.data, 1, ctypes.byref(tid)) == -22
    assert lib.cbft_ecdsa_load_keys_curve(ctx.handle, 1, None, 1, ctypes.byref(tid)) == -22
    assert lib.cbft_ecdsa_load_keys_curve(ctx.handle, 1, one.ctypes.data, (1 << 20) + 1, ctypes.byref(tid)) == -7
    with pytest.raises(ValueError):
        ctx.ecdsa_load_keys([bytes(64)], curve="secp384r1")
    with pytest.raises(cb.CbftError) as ei:
        ctx.ecdsa_verify(pool_table, [NKEYS], [pool["sigs"][0]], [pool["msgs"][0]])  # key index out of range
    assert ei.value.code == -22
    assert ctx.ecdsa_verify(pool_table, [], [], []) == b""  # n = 0 is CBFT_OK


def test_kernel_time_with_profiling(ctx, pool, pool_table):
    ctx.set_profiling(True)
    try:
        ctx.ecdsa_verify(pool_table, pool["kidx"][:64], pool["sigs"][:64], pool["msgs"][:64])
        assert ctx.ecdsa_kernel_ms() > 0
    finally:
        ctx.set_profiling(False)
