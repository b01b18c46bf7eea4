"""GPU tests of what the host front ends share (concord-bft_amd/csrc/cbft_host_util.h and the scratch
guard, secret clearing and packed-image upload of cbft_internal.h), through the C ABI of all six:
Ed25519 signing, RSA signing, BLS share signing, RSA verification, ECDSA verification and batched
BLS verification.

Each front end has one pool of 300 items with its expected results, computed once by the project's
CPU references (host OpenSSL for Ed25519 signing, tests/rsagen.py for RSA signing, the host shim's
double-and-add for BLS shares, oracle/rsa_ref.py and tests/ecdsa_ref.py for the two verifiers).  The
Python pairing takes seconds per item, so batched BLS verification is checked against verdicts known
by construction (shares made by cbft_bls_sign_batch, which its own tests pin to the oracle, every
7th one on a changed message) and against the Python oracle on two of them.  The first 130 messages
of a pool are 32 bytes long: the fixed-length device entry points sign those."""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import blsgen
import bn254_ref as B
import cbft_hipcrypto as cb
import ecdsa_ref
import rsa_ref
import rsagen
from rsa_sign_vectors import crt_params
from sign_vectors import Hip, openssl_sign_many

pytestmark = pytest.mark.gpu
EINVAL = -22
MAX_MSG_LEN = 0xFFFFFF00  # CBFT_MAX_MSG_LEN
POOL = 300
FIXED = 130  # the pool's first messages, 32 bytes each
NS = 65      # one full wave plus one lane; crosses a 64-bit verdict word
FILL = 0xC3  # what an output buffer holds before a call


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _messages(seed):
    rng = random.Random(seed)
    lens = [0, 1, 31, 32, 55, 56, 64, 111, 112, 119, 120, 128, 300]
    return [rng.randbytes(32) for _ in range(FIXED)] + [rng.randbytes(lens[i % len(lens)]) for i in range(POOL - FIXED)]


class FrontEnd:
    """One front end's pool and its calls.  call() is the raw host-array entry point on the pool items
    `sel`, with any of its arrays replaced; it returns (status, result, untouched), `untouched` saying
    that the output buffer still holds FILL."""
    checks_len = True
    has_device = True
    is_signer = False
    nkeys = 3

    def arrays(self, sel):
        blob, off, lens = cb.pack_messages([self.msgs[i] for i in sel])
        return np.array([self.idx[i] for i in sel], dtype=np.uint32), blob.copy(), off, lens

    def call(self, c, tid, sel, idx="pool", blob="pool", off=None, lens=None):
        a_idx, a_blob, a_off, a_lens = self.arrays(sel)
        idx = a_idx if isinstance(idx, str) else idx
        blob = a_blob if isinstance(blob, str) else blob
        off = a_off if off is None else off
        lens = a_lens if lens is None else lens
        return self.raw(c, tid, sel, idx, blob, off, lens)

    def expected(self, sel):
        return self.exp[list(sel)]


class Signer(FrontEnd):
    is_signer = True

    def raw(self, c, tid, sel, idx, blob, off, lens):
        out = np.full((len(sel), self.width), FILL, dtype=np.uint8)
        rc = self.entry(c, tid, _p(idx), _p(blob), _p(off), _p(lens), len(sel), _p(out))
        return rc, out, bool((out == FILL).all())

    def device(self, c, hip, tid, sel, stream):
        """Queue the fixed-length device call for pool items sel on stream; returns the reader."""
        n = len(sel)
        assert all(len(self.msgs[i]) == 32 for i in sel)
        d_msg = hip.to_dev(np.frombuffer(b"".join(self.msgs[i] for i in sel), dtype=np.uint8))
        d_idx = hip.to_dev(np.array([self.idx[i] for i in sel], dtype=np.uint32))
        d_out = hip.to_dev(np.full(n * self.width, FILL, dtype=np.uint8))
        self.device_entry(c)(tid, d_idx, d_msg, 32, n, d_out, stream)
        return lambda: hip.from_dev(d_out, n * self.width).reshape(n, self.width)


class EdSign(Signer):
    width = 64

    def __init__(self, ctx):
        self.seeds = np.frombuffer(random.Random(0xE1).randbytes(32 * self.nkeys), dtype=np.uint8).reshape(-1, 32)
        self.msgs = _messages(0xE2)
        self.idx = [random.Random(0xE3 + i).randrange(self.nkeys) for i in range(POOL)]
        blob, off, lens = cb.pack_messages(self.msgs)
        self.exp = openssl_sign_many(self.seeds, np.array(self.idx, dtype=np.uint32), blob, off, lens)

    def load(self, c):
        return c.load_signers(self.seeds)

    def unload(self, c, tid):
        c.unload_signers(tid)

    def entry(self, c, *a):
        return c.lib.cbft_ed25519_sign_batch(c.handle, *a)

    def device_entry(self, c):
        return c.sign_fixed_device


class RsaSign(Signer):
    width = 256

    def __init__(self, ctx):
        self.keys = rsagen.load_keys()[:self.nkeys]
        self.msgs = _messages(0xA1)
        self.idx = [random.Random(0xA3 + i).randrange(self.nkeys) for i in range(POOL)]
        rows = [rsagen.sign(self.keys[k], m) for k, m in zip(self.idx, self.msgs)]
        self.exp = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(POOL, 256)

    def load(self, c):
        return c.rsa_load_signers([crt_params(k) for k in self.keys])

    def unload(self, c, tid):
        c.rsa_unload_signers(tid)

    def entry(self, c, *a):
        return c.lib.cbft_rsa_sign_batch(c.handle, *a, None)

    def device_entry(self, c):
        return c.rsa_sign_fixed_device


class BlsSign(Signer):
    width = 37

    def __init__(self, ctx):
        rng = random.Random(0xB1)
        self.sks = [rng.randrange(1, B.R) for _ in range(self.nkeys)]
        self.ids = [5, 1, 2048]
        self.msgs = _messages(0xB2)
        self.idx = [random.Random(0xB3 + i).randrange(self.nkeys) for i in range(POOL)]

        def share(j):
            out = ctypes.create_string_buffer(37)
            m = self.msgs[j]
            blsgen.shim().shim_sign_share(blsgen.be32(self.sks[self.idx[j]]), self.ids[self.idx[j]], m, len(m), out)
            return out.raw

        with ThreadPoolExecutor(16) as ex:  # ctypes drops the GIL
            rows = list(ex.map(share, range(POOL)))
        self.exp = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(POOL, 37)

    def load(self, c):
        return c.load_bls_signers(self.sks, self.ids)

    def unload(self, c, tid):
        c.unload_bls_signers(tid)

    def entry(self, c, *a):
        return c.lib.cbft_bls_sign_batch(c.handle, *a)

    def device_entry(self, c):
        return c.bls_sign_fixed_device


class Verifier(FrontEnd):
    checks_len = False

    def raw(self, c, tid, sel, idx, blob, off, lens):
        n = len(sel)
        sig = np.frombuffer(b"".join(self.sigs[i] for i in sel), dtype=np.uint8).copy()
        bm = np.full((n + 7) // 8, FILL, dtype=np.uint8)
        rc = self.entry(c, tid, _p(idx), _p(sig), _p(blob), _p(off), _p(lens), n, _p(bm))
        return rc, cb.bitmap_to_bools(bm.tobytes(), n), bool((bm == FILL).all())

    def device(self, c, hip, tid, sel, stream):
        n = len(sel)
        idx, blob, off, lens = self.arrays(sel)
        d_sig = hip.to_dev(np.frombuffer(b"".join(self.sigs[i] for i in sel), dtype=np.uint8))
        d_words = hip.to_dev(np.full((n + 63) // 64, 0xC3C3C3C3C3C3C3C3, dtype=np.uint64))
        self.device_entry(c)(tid, hip.to_dev(idx), d_sig, hip.to_dev(blob), hip.to_dev(off), hip.to_dev(lens), n,
                             d_words, stream)
        return lambda: cb.bitmap_to_bools(hip.from_dev(d_words, (n + 63) // 64 * 8).tobytes(), n)


class RsaVerify(Verifier):
    nkeys = 8

    def __init__(self, ctx):
        keys, self.idx, self.sigs, self.msgs, _ = rsagen.signed_batch(POOL, nuniq=96, msg_len=(0, 200), seed=0x4A)
        self.keys = [(k["n"], k["e"]) for k in keys]
        assert len(self.keys) == self.nkeys
        self.exp = np.array([rsa_ref.verify(*self.keys[k], m, s) for k, s, m in zip(self.idx, self.sigs, self.msgs)])
        assert self.exp[:8].any() and self.exp.sum() > POOL // 2 and (~self.exp).sum() > 8

    def load(self, c):
        return c.rsa_load_keys(self.keys)

    def unload(self, c, tid):
        c.rsa_unload_keys(tid)

    def entry(self, c, *a):
        return c.lib.cbft_rsa_verify_batch(c.handle, *a)

    def device_entry(self, c):
        return c.rsa_verify_device


class EcdsaVerify(Verifier):
    def __init__(self, ctx):
        rng = random.Random(0xEC)
        N = ecdsa_ref.N
        privs = [rng.randrange(1, N) for _ in range(self.nkeys)]
        self.pubs = [ecdsa_ref.pub_bytes(ecdsa_ref.mul(d, ecdsa_ref.G)) for d in privs]
        self.msgs = _messages(0xED)
        k = rng.randrange(1, N - POOL)
        R = ecdsa_ref.mul(k, ecdsa_ref.G)  # nonces step by one: each R costs one point addition
        self.idx, self.sigs = [], []
        for i in range(POOL):
            ki = rng.randrange(self.nkeys)
            r = R[0] % N
            s = pow(k, -1, N) * (ecdsa_ref.digest_int(self.msgs[i]) + r * privs[ki]) % N
            k, R = k + 1, ecdsa_ref.add(R, ecdsa_ref.G)
            if i % 7 == 3:
                s ^= 1 << rng.randrange(255)
            self.idx.append(ki)
            self.sigs.append(ecdsa_ref.sig_bytes(r, s))
        self.exp = np.array([ecdsa_ref.verify(self.pubs[ki], s, m) for ki, s, m in zip(self.idx, self.sigs, self.msgs)])
        assert self.exp.tolist() == [i % 7 != 3 for i in range(POOL)]

    def load(self, c):
        return c.ecdsa_load_keys(self.pubs)

    def unload(self, c, tid):
        c.ecdsa_unload_keys(tid)

    def entry(self, c, *a):
        return c.lib.cbft_ecdsa_verify_batch(c.handle, *a)

    def device_entry(self, c):
        return c.ecdsa_verify_device


class BlsVerify(Verifier):
    """Item i: the share of signer i % 3 + 1 on message i under key slot i % 3 + 1; every 7th item
    names a message with one bit changed.  idx holds key slots (0 = the group key, so nkeys itself is
    a valid slot)."""
    checks_len = True
    has_device = False  # tests/test_bls_verify_batch_gpu.py::test_device_form runs two streams

    def __init__(self, ctx):
        _, sks, self.pk, self.vks = blsgen.keyset(self.nkeys, 2, seed=0xB7)
        signed = _messages(0xB8)
        self.idx = [i % self.nkeys + 1 for i in range(POOL)]
        tid = ctx.load_bls_signers([sks[i] for i in range(1, self.nkeys + 1)], list(range(1, self.nkeys + 1)))
        try:
            out = ctx.bls_sign_batch(tid, signed, [s - 1 for s in self.idx])
        finally:
            ctx.unload_bls_signers(tid)
        self.sigs = [out[i].tobytes()[4:] for i in range(POOL)]
        self.msgs = [m if i % 7 != 3 else bytes([(m or b"\0")[0] ^ 0x40]) + m[1:] for i, m in enumerate(signed)]
        self.exp = np.array([i % 7 != 3 for i in range(POOL)])
        for i in (2, 3):  # the construction itself, against the Python pairing: one of each kind
            key = B.g2_from_bytes(self.vks[self.idx[i] - 1])
            assert B.verify(self.msgs[i], self.sigs[i], key) == bool(self.exp[i])

    def load(self, c):
        return c.bls_load_keys(self.pk, self.vks)

    def unload(self, c, tid):
        c.bls_unload_keys(tid)

    def entry(self, c, tid, idx, sig, blob, off, lens, n, bm):
        return c.lib.cbft_bls_verify_batch(c.handle, tid, idx, sig, blob, off, lens, n, None, n, bm)


FRONT_ENDS = {"ed25519_sign": EdSign, "rsa_sign": RsaSign, "bls_sign": BlsSign, "rsa_verify": RsaVerify,
              "ecdsa_verify": EcdsaVerify, "bls_verify_batch": BlsVerify}
_built = {}


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture
def fe(request, ctx):
    """The front end named by the test's parameter; its pool is built once for the module."""
    name = request.param
    if name not in _built:
        _built[name] = FRONT_ENDS[name](ctx)
    return _built[name]


def _same(fe, got, sel):
    exp = fe.expected(sel)
    bad = np.nonzero((got != exp).reshape(len(sel), -1).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(sel)} differ from the reference, first {bad[:8]}"


@pytest.mark.parametrize("fe", [k for k, v in FRONT_ENDS.items() if v.has_device], indirect=True)
def test_two_streams_share_the_scratch(fe):
    """Two device-entry batches of 65 different items on two non-default streams, synchronised only
    after both are queued: each equals the host-array call on the same items (and the reference)."""
    hip = Hip()
    a, b = list(range(NS)), list(range(NS, 2 * NS))
    try:
        with cb.Context(device=0) as c:
            tid = fe.load(c)
            host = [fe.call(c, tid, sel) for sel in (a, b)]
            readers = [fe.device(c, hip, tid, sel, hip.stream()) for sel in (a, b)]
            hip.sync()
            got = [r() for r in readers]
            fe.unload(c, tid)
    finally:
        hip.close()
    for sel, (rc, h, _), g in zip((a, b), host, got):
        assert rc == 0
        assert np.array_equal(g, h), "device entry differs from the host-array call"
        _same(fe, g, sel)
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("fe", list(FRONT_ENDS), indirect=True)
def test_growth_and_shrink(fe):
    """Host-array batches of 8, 300 and 8 items on one fresh context: the buffers grow with the
    scratch guard's event already recorded, then a small batch runs in the large buffers."""
    with cb.Context(device=0) as c:
        tid = fe.load(c)
        for sel in (range(8), range(POOL), range(POOL - 8, POOL)):
            rc, got, _ = fe.call(c, tid, list(sel))
            assert rc == 0
            _same(fe, got, list(sel))
        fe.unload(c, tid)


CASES = ["unknown_id", "index_past_end", "length_over_cap", "null_blob", "offset_wraps"]
# RSA and ECDSA verification hash messages of any length: no length case for them
ARG_TABLE = [(k, case) for k, v in FRONT_ENDS.items() for case in CASES if case != "length_over_cap" or v.checks_len]


@pytest.mark.parametrize("fe,case", ARG_TABLE, indirect=["fe"])
def test_argument_table(ctx, fe, case):
    """Each bad argument gives CBFT_EINVAL with the output untouched, and a valid batch of 8 right
    after it on the same context is correct."""
    sel = list(range(8))
    idx, blob, off, lens = fe.arrays(sel)
    assert int(lens.sum()) > 0
    tid = fe.load(ctx)
    try:
        if case == "unknown_id":
            rc, _, untouched = fe.call(ctx, tid + 1000, sel)
        elif case == "index_past_end":
            idx[3] = fe.nkeys + (1 if isinstance(fe, BlsVerify) else 0)
            rc, _, untouched = fe.call(ctx, tid, sel, idx=idx)
        elif case == "length_over_cap":
            lens[2] = MAX_MSG_LEN + 1
            rc, _, untouched = fe.call(ctx, tid, sel, lens=lens)
        elif case == "null_blob":
            rc, _, untouched = fe.call(ctx, tid, sel, blob=None)
        else:
            assert int(lens[5]) > 0
            off[5] = np.uint64(2 ** 64 - int(lens[5]))  # message 5 would end at 2^64: one byte too far
            rc, _, untouched = fe.call(ctx, tid, sel, off=off)
        assert rc == EINVAL and untouched
        rc, got, _ = fe.call(ctx, tid, sel)
        assert rc == 0
        _same(fe, got, sel)
    finally:
        fe.unload(ctx, tid)


@pytest.mark.parametrize("fe", [k for k, v in FRONT_ENDS.items() if v.is_signer], indirect=True)
def test_reload_signer_table(ctx, fe):
    """A signer table of 3 keys is unloaded (its records zeroed and freed) and loaded again: a batch
    of 8 under the new id is correct, the old id is unknown."""
    sel = list(range(8))
    old = fe.load(ctx)
    rc, got, _ = fe.call(ctx, old, sel)
    assert rc == 0
    _same(fe, got, sel)
    fe.unload(ctx, old)
    new = fe.load(ctx)
    try:
        assert new != old
        rc, got, _ = fe.call(ctx, new, sel)
        assert rc == 0
        _same(fe, got, sel)
        rc, _, untouched = fe.call(ctx, old, sel)
        assert rc == EINVAL and untouched
    finally:
        fe.unload(ctx, new)
