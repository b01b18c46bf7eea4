"""GPU tests of batched RSA-2048 PKCS#1 v1.5 / SHA-256 signing through the C ABI.  Signatures are
deterministic, so every check is byte for byte: against the OpenSSL-generated fixture
(tests/golden/rsa_sign_vectors.json), against the oracle's CRT signer, and through the library's
own batch verify."""
import ctypes
import os
import random

import numpy as np
import pytest

import cbft_hipcrypto as cb
import rsagen
from rsa_sign_vectors import crt_edge_ems, crt_params, load_rsa_sign_vectors
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -22
ZERO = bytes(256)
BLOCK = 32  # signatures per block of the signing kernel (RSAS_PSIG)


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def keys():
    return rsagen.load_keys()


@pytest.fixture(scope="module")
def table(ctx, keys):
    """One signer table of all eight fixture keys, shared by the tests that only sign."""
    tid = ctx.rsa_load_signers([crt_params(k) for k in keys])
    yield tid
    ctx.rsa_unload_signers(tid)


@pytest.fixture(scope="module")
def mixed(keys):
    """2 * BLOCK + 1 messages of mixed lengths under mixed signers with the oracle's signatures,
    computed once; the batch-size tests sign prefixes of it."""
    rng = random.Random(77)
    lens = [0, 1, 32, 55, 56, 63, 64, 119, 120, 300]
    n = 2 * BLOCK + 1
    msgs = [rng.randbytes(lens[(i * 7) % len(lens)]) for i in range(n)]
    idx = [(i * 5 + i // 8) % len(keys) for i in range(n)]
    sigs = [rsagen.sign(keys[k], m) for k, m in zip(idx, msgs)]
    return msgs, idx, sigs


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_whole_fixture_byte_exact(ctx, table, keys):
    """The fixture as one variable-length batch (lengths 0 .. 4,096, the SHA-256 padding edges),
    all eight keys (e = 3, 17, 65537, 0xC0000001; p > q and p < q) mixed through signer_idx."""
    vectors = load_rsa_sign_vectors()
    assert ctx.rsa_signer_status(table).all()
    order = list(range(len(vectors)))
    random.Random(5).shuffle(order)
    got, failed = ctx.rsa_sign_batch(table, [vectors[i].msg for i in order], [vectors[i].key for i in order])
    assert failed == 0
    bad = [i for j, i in enumerate(order) if got[j].tobytes() != vectors[i].sig]
    assert not bad, f"{len(bad)} signatures differ, first records {bad[:8]}"


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_batch_size_edges(ctx, table, keys, mixed, n):
    """One block less one, one block, one block plus one, two blocks plus a tail: signers and
    lengths mixed inside the batch, byte-equal to the oracle and accepted by the GPU verifier."""
    msgs, idx, sigs = (x[:n] for x in mixed)
    got, failed = ctx.rsa_sign_batch(table, msgs, idx)
    assert failed == 0
    bad = [i for i in range(n) if got[i].tobytes() != sigs[i]]
    assert not bad, f"{len(bad)} of {n} differ, first {bad[:8]}"
    vt = ctx.rsa_load_keys([(k["n"], k["e"]) for k in keys])
    try:
        ok = cb.bitmap_to_bools(ctx.rsa_verify(vt, idx, got, msgs), n)
        assert ok.all()
    finally:
        ctx.rsa_unload_keys(vt)


def test_null_signer_idx_is_signer_zero(ctx, table, mixed):
    msgs = mixed[0][:BLOCK + 1]
    a, fa = ctx.rsa_sign_batch(table, msgs, None)
    b, fb = ctx.rsa_sign_batch(table, msgs, [0] * len(msgs))
    assert fa == fb == 0
    assert np.array_equal(a, b) and a.any(axis=1).all()


def test_einval_leaves_out_sig_untouched_and_empty_batch_is_ok(ctx, table, mixed):
    msgs = mixed[0][:3]
    blob, off, lens = cb.pack_messages(msgs)
    out = np.full((3, 256), 0xAB, dtype=np.uint8)
    idx = np.array([0, 8, 1], dtype=np.uint32)  # 8 == nkeys
    failed = ctypes.c_uint32(7)
    rc = ctx.lib.cbft_rsa_sign_batch(ctx.handle, table, _p(idx), _p(blob), _p(off), _p(lens), 3, _p(out),
                                     ctypes.byref(failed))
    assert rc == EINVAL and (out == 0xAB).all()
    rc = ctx.lib.cbft_rsa_sign_batch(ctx.handle, table, None, None, None, None, 0, None, ctypes.byref(failed))
    assert rc == 0 and failed.value == 0


def test_fixed_device_equals_host_arrays_and_out_of_range_is_zero(ctx, table, keys):
    """32-byte messages resident on the device: equal to the host-array call; an index out of
    range gives 256 zero bytes and its neighbours stay correct."""
    n = BLOCK + 3
    rng = np.random.default_rng(9)
    blob = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    idx = (np.arange(n, dtype=np.uint32) * 3) % 8
    msgs = [blob[32 * i:32 * i + 32].tobytes() for i in range(n)]
    exp, failed = ctx.rsa_sign_batch(table, msgs, idx)
    assert failed == 0
    assert exp[0].tobytes() == rsagen.sign(keys[int(idx[0])], msgs[0])
    bad_idx = idx.copy()
    bad_idx[5] = 8
    bad_idx[n - 1] = 0xFFFFFFFF
    hip = Hip()
    try:
        d_msg, d_idx, d_bad = hip.to_dev(blob), hip.to_dev(idx), hip.to_dev(bad_idx)
        d_sig = hip.to_dev(np.full(n * 256, 0xCD, dtype=np.uint8))
        ctx.rsa_sign_fixed_device(table, d_idx, d_msg, 32, n, d_sig)
        hip.sync()
        got = hip.from_dev(d_sig, n * 256).reshape(n, 256)
        assert np.array_equal(got, exp)
        ctx.rsa_sign_fixed_device(table, d_bad, d_msg, 32, n, d_sig, hip.stream())
        hip.sync()
        got = hip.from_dev(d_sig, n * 256).reshape(n, 256)
        for i in range(n):
            assert got[i].tobytes() == (ZERO if i in (5, n - 1) else exp[i].tobytes()), i
    finally:
        hip.close()


def test_inconsistent_key_is_reported_and_withheld(ctx, keys, mixed):
    """A key whose dQ has one bit flipped (still a valid-shape exponent) beside good keys: a wrong
    number, caught by the load-time self-test; its signatures are withheld and counted, the good
    keys' signatures are unchanged."""
    good0, good1 = crt_params(keys[1]), crt_params(keys[0])
    p, q, dP, dQ, qInv, e = crt_params(keys[2])
    tid = ctx.rsa_load_signers([good0, (p, q, dP, dQ ^ (1 << 77), qInv, e), good1])
    try:
        assert ctx.rsa_signer_status(tid).tolist() == [True, False, True]
        msgs = mixed[0][:12]
        idx = [0, 1, 2, 1, 1, 0, 2, 2, 1, 0, 0, 1]
        got, failed = ctx.rsa_sign_batch(tid, msgs, idx)
        assert failed == idx.count(1)
        for i, (k, m) in enumerate(zip(idx, msgs)):
            exp = ZERO if k == 1 else rsagen.sign(keys[1] if k == 0 else keys[0], m)
            assert got[i].tobytes() == exp, i
    finally:
        ctx.rsa_unload_signers(tid)


def test_malformed_keys_are_accepted_and_reported(ctx, keys):
    """Even p, p == q, a short q, a wrong qInv: accepted into the table, status 0, zero signatures."""
    p, q, dP, dQ, qInv, e = crt_params(keys[3])
    table = [(p, q, dP, dQ, qInv, e), (p - 1, q, dP, dQ, qInv, e), (p, p, dP, dP, qInv, e),
             (p, q >> 1 | 1, dP, dQ, qInv, e), (p, q, dP, dQ, qInv + 2, e)]
    tid = ctx.rsa_load_signers(table)
    try:
        assert ctx.rsa_signer_status(tid).tolist() == [True, False, False, False, False]
        got, failed = ctx.rsa_sign_batch(tid, [b"m"] * 5, [0, 1, 2, 3, 4])
        assert failed == 4
        assert got[0].tobytes() == rsagen.sign(keys[3], b"m")
        assert all(got[i].tobytes() == ZERO for i in range(1, 5))
    finally:
        ctx.rsa_unload_signers(tid)


def test_signer_moduli(ctx, table, keys):
    assert ctx.rsa_signer_moduli(table) == [k["p"] * k["q"] for k in keys]


def test_unload_then_sign_is_einval(ctx, keys):
    tid = ctx.rsa_load_signers([crt_params(keys[0])])
    ctx.rsa_unload_signers(tid)
    blob, off, lens = cb.pack_messages([b"x"])
    out = np.zeros((1, 256), dtype=np.uint8)
    rc = ctx.lib.cbft_rsa_sign_batch(ctx.handle, tid, None, _p(blob), _p(off), _p(lens), 1, _p(out), None)
    assert rc == EINVAL
    assert ctx.lib.cbft_rsa_unload_signers(ctx.handle, tid) == EINVAL
    st = np.zeros(1, dtype=np.uint8)
    assert ctx.lib.cbft_rsa_signer_status(ctx.handle, tid, _p(st)) == EINVAL


def test_crt_core_on_raw_representatives(keys):
    """The test-only harness (tests/hip/rsa_sign_selftest.hip) drives the CRT core on raw EM
    integers that messages cannot reach, for a key with p > q and one with p < q: EM = 0, 1, n - 1,
    multiples of p and of q, m_p == m_q (h = 0), m_p < m_q, m_q >= p; and CRT exponents of all ones
    and with mostly zero windows.  Each result is checked against Python pow; the window-table
    scratch must be all zero afterwards."""
    path = os.path.join(HERE, "hip", "librsa_sign_selftest.so")
    assert os.path.exists(path), "tests/hip/librsa_sign_selftest.so not built (make selftest)"
    cb.load_library()
    lib = ctypes.CDLL(path)
    gt, lt = crt_params(keys[1]), crt_params(keys[0])
    assert gt[0] > gt[1] and lt[0] < lt[1]
    ones = (1 << 1024) - 1
    sparse_p, sparse_q = (1 << 1020) | 1, (1 << 1023) | (1 << 512)
    table, items = [], []
    for kp in (gt, lt):
        p, q, dP, dQ, qInv, e = kp
        base = len(table)
        table += [kp, (p, q, ones, ones, qInv, e), (p, q, sparse_p, sparse_q, qInv, e)]
        for name, em in crt_edge_ems(p, q, dP, dQ, qInv).items():
            items.append((base, em, name))
        rng = random.Random(p & 0xFFFF)
        for j in (1, 2):
            for t in range(3):
                items.append((base + j, rng.randrange(p * q), f"exponent{j}"))
            items.append((base + j, 0, f"exponent{j}_zero"))
            items.append((base + j, p * q - 1, f"exponent{j}_top"))
    assert len(items) > BLOCK  # more than one block
    priv = np.frombuffer(b"".join(int(v).to_bytes(128, "big") for k in table for v in k[:5]), dtype=np.uint8)
    exps = np.array([k[5] for k in table], dtype=np.uint32)
    kidx = np.array([i[0] for i in items], dtype=np.uint32)
    em = np.frombuffer(b"".join(i[1].to_bytes(256, "big") for i in items), dtype=np.uint8)
    out = np.zeros((len(items), 256), dtype=np.uint8)
    mod = np.zeros((len(table), 256), dtype=np.uint8)
    struct = np.zeros(len(table), dtype=np.uint32)
    scr = ctypes.c_uint32(1)
    rc = lib.rsa_sign_selftest_crt(_p(priv), _p(exps), len(table), _p(kidx), _p(em), len(items), _p(out), _p(mod),
                                   _p(struct), ctypes.byref(scr))
    assert rc == 0
    assert struct.tolist() == [1] * len(table)  # the structural checks do not look at dP, dQ
    assert scr.value == 0, "window tables left in the scratch"
    for k, row in zip(table, mod):
        assert int.from_bytes(row.tobytes(), "big") == k[0] * k[1]
    for (ki, e_m, name), row in zip(items, out):
        p, q, dP, dQ, qInv, _ = table[ki]
        m_p, m_q = pow(e_m, dP, p), pow(e_m, dQ, q)
        exp = m_q + (qInv * (m_p - m_q) % p) * q
        assert int.from_bytes(row.tobytes(), "big") == exp, (name, ki)
        if ki % 3 == 0:
            d = pow(k_e(table[ki]), -1, (p - 1) * (q - 1))
            assert exp == pow(e_m, d, p * q), name


def k_e(k):
    return k[5]
