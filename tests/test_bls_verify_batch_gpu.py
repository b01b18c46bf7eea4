"""GPU tests of batched BLS verification over many messages (cbft_bls_verify_batch,
cbft_bls_verify_fixed_device) through the C ABI.  Shares come from ctx.bls_sign_batch and combined
signatures from ctx.bls_combine (both pinned to the oracle by their own tests); expected verdicts
come by construction, from the lone calls (cbft_bls_verify, cbft_bls_verify_shares: independent
kernels) and, on samples, from the Python oracle's pairing."""
import ctypes
import random

import numpy as np
import pytest

import blsgen
import bn254_ref as B
import cbft_hipcrypto as cb
from bls_sign_vectors import load_fixture, pack
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
EINVAL = -22
NMAX = 1100
NKEYS, THRESH = 16, 11
GRID_MSGS = 7  # messages every signer signs (msg_of, multi-device)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class World:
    """One 11-of-16 key set, NMAX distinct 32-byte messages, item i = the share of signer i % 16 + 1 on
    message i, or (every 5th i) the combined signature under the group key; and every signer's share
    of the first GRID_MSGS messages."""

    def __init__(self, ctx):
        self.sk, self.sks, self.pk, self.vks = blsgen.keyset(NKEYS, THRESH, seed=0x20B)
        rng = random.Random(0x20C)
        self.msgs = [rng.randbytes(32) for _ in range(NMAX)]
        self.slot = [0 if i % 5 == 0 else i % NKEYS + 1 for i in range(NMAX)]
        jobs = []  # (signer index, message index)
        for i, s in enumerate(self.slot):
            jobs += [(j, i) for j in range(THRESH)] if s == 0 else [(s - 1, i)]
        grid_at = len(jobs)
        jobs += [(s, j) for j in range(GRID_MSGS) for s in range(NKEYS)]
        tid = ctx.load_bls_signers([self.sks[i] for i in range(1, NKEYS + 1)], list(range(1, NKEYS + 1)))
        try:
            out = ctx.bls_sign_batch(tid, [self.msgs[m] for _, m in jobs], [s for s, _ in jobs])
        finally:
            ctx.unload_bls_signers(tid)
        self.sig, at = [], 0
        for s in self.slot:
            if s == 0:
                self.sig.append(ctx.bls_combine([out[at + j].tobytes() for j in range(THRESH)]))
                at += THRESH
            else:
                self.sig.append(out[at].tobytes()[4:])
                at += 1
        assert at == grid_at
        # grid[j][s]: 33-byte point of signer s + 1 on message j
        self.grid = [[out[grid_at + j * NKEYS + s].tobytes()[4:] for s in range(NKEYS)] for j in range(GRID_MSGS)]
        self.kid = ctx.bls_load_keys(self.pk, self.vks)
        self._oracle = {}

    def key(self, slot):
        return B.g2_from_bytes(self.pk if slot == 0 else self.vks[slot - 1])

    def oracle(self, slot, msg, sig33):
        k = (slot, msg, sig33)
        if k not in self._oracle:
            self._oracle[k] = B.verify(msg, sig33, self.key(slot))
        return self._oracle[k]

    def lone(self, ctx, slot, msg, sig33):
        if slot == 0:
            return ctx.bls_verify(self.kid, msg, sig33)
        return bool(ctx.bls_verify_shares(self.kid, msg, [slot.to_bytes(4, "big") + sig33])[0])


@pytest.fixture(scope="module")
def ctx():
    with cb.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def w(ctx):
    world = World(ctx)
    yield world
    ctx.bls_unload_keys(world.kid)


def _doubled(sig33):
    return blsgen.doubled(b"\0\0\0\1" + sig33)[4:]


def _spoiled(w, n):
    """Items 0 .. n - 1 with every 7th spoiled, cycling through wrong message, wrong key slot and doubled
    point: (slots, sigs, msgs, expected)."""
    slots, sigs, msgs = list(w.slot[:n]), list(w.sig[:n]), list(w.msgs[:n])
    exp = [True] * n
    for c, i in enumerate(range(3, n, 7)):
        exp[i] = False
        if c % 3 == 0:
            msgs[i] = bytes([msgs[i][0] ^ 0x40]) + msgs[i][1:]
        elif c % 3 == 1:
            slots[i] = slots[i] % NKEYS + 1
        else:
            sigs[i] = _doubled(sigs[i])
    return slots, sigs, msgs, exp


def test_verdict_table(ctx, w):
    """Every malformed case of test_bls_gpu.py::test_share_verification_verdicts, each on its own
    message, once under a vk slot and once under slot 0, shuffled among valid items: all equal the
    oracle."""
    x = next(x for x in range(1, 100) if pow((x ** 3 + 2) % B.P, (B.P - 1) // 2, B.P) != 1)
    items = []  # (slot, msg, sig33)
    share_at = [i for i in range(NMAX) if w.slot[i] != 0]
    comb_at = [i for i in range(NMAX) if w.slot[i] == 0]
    for base in (share_at, comb_at):
        it = iter(base)
        for case in range(9):
            i = next(it)
            s = w.sig[i]
            if case == 1:  # signer 6's point on this message, under this item's slot
                assert i < GRID_MSGS and w.slot[i] != 6
                s = w.grid[i][5]
            bad = [_doubled(s), s, b"\x05" + s[1:], b"\x02" + B.P.to_bytes(32, "big"), b"\x02" + x.to_bytes(32, "big"),
                   b"\x03" + x.to_bytes(32, "big"), bytes(33), b"\x00\x01" + bytes(31), bytes([s[0] ^ 1]) + s[1:]][case]
            items.append((w.slot[i], w.msgs[i], bad))
        for _ in range(3):
            i = next(it)
            items.append((w.slot[i], w.msgs[i], w.sig[i]))
    random.Random(1).shuffle(items)
    got = ctx.bls_verify_batch(w.kid, [s for _, _, s in items], [m for _, m, _ in items], [k for k, _, _ in items])
    exp = [w.oracle(*it) for it in items]
    assert got.tolist() == exp
    assert sum(exp) == 6


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, NMAX])
def test_size_edges(ctx, w, n):
    """Distinct 32-byte messages: lane and wave edges of the decode, the hash kernel's 256-message block,
    more waves than the chip's 1,024 SIMDs.  Every 7th item spoiled."""
    slots, sigs, msgs, exp = _spoiled(w, n)
    got = ctx.bls_verify_batch(w.kid, sigs, msgs, slots)
    bad = np.nonzero(got != np.array(exp))[0]
    assert bad.size == 0, f"{bad.size} of {n} differ from the construction, first {bad[:8]}"
    rng = random.Random(n)
    for i in sorted(rng.sample(range(n), min(n, 32))):
        assert bool(got[i]) == w.lone(ctx, slots[i], msgs[i], sigs[i]), f"item {i} differs from the lone call"
    pool = sorted(set(range(3, n, 7)) | set(range(0, n, 5)))[:8] or [0]  # shared by every n: cached
    for i in pool[:8]:
        assert bool(got[i]) == w.oracle(slots[i], msgs[i], sigs[i]), f"item {i} differs from the oracle"


def test_msg_of(ctx, w):
    """m = 5, n = 200 over 16 signers with repeats; m = 1 equals cbft_bls_verify_shares on the same
    shares; msg_of = None equals an explicit identity."""
    rng = random.Random(4)
    m, n = 5, 200
    signer = [rng.randrange(NKEYS) for _ in range(n)]
    signed = [rng.randrange(m) for _ in range(n)]
    named = [(j + 1) % m if i % 9 == 4 else j for i, j in enumerate(signed)]  # every 9th names another message
    sigs = [w.grid[j][s] for s, j in zip(signer, signed)]
    got = ctx.bls_verify_batch(w.kid, sigs, w.msgs[:m], [s + 1 for s in signer], named)
    assert got.tolist() == [a == b for a, b in zip(signed, named)]
    # one message: the whole bitmap against the share verifier
    sig1 = [_doubled(w.grid[0][s]) if i % 11 == 2 else w.grid[0][s] for i, s in enumerate(signer)]
    got = ctx.bls_verify_batch(w.kid, sig1, w.msgs[:1], [s + 1 for s in signer], [0] * n)
    want = ctx.bls_verify_shares(w.kid, w.msgs[0], [(s + 1).to_bytes(4, "big") + g for s, g in zip(signer, sig1)])
    assert got.tolist() == want.tolist() == [i % 11 != 2 for i in range(n)]
    slots, sigs, msgs, exp = _spoiled(w, 65)
    a = ctx.bls_verify_batch(w.kid, sigs, msgs, slots)
    b = ctx.bls_verify_batch(w.kid, sigs, msgs, slots, list(range(65)))
    assert a.tolist() == b.tolist() == exp


def test_mixed_slots(ctx, w):
    """Certificates under slot 0 and shares under slots 1 .. 16 in one batch; a batch of certificates
    alone with key_idx = None; slot-0 verdicts equal cbft_bls_verify."""
    slots, sigs, msgs, exp = _spoiled(w, 120)
    assert 0 in slots and len(set(slots)) == NKEYS + 1
    got = ctx.bls_verify_batch(w.kid, sigs, msgs, slots)
    assert got.tolist() == exp
    for i in [i for i in range(120) if slots[i] == 0]:
        assert bool(got[i]) == ctx.bls_verify(w.kid, msgs[i], sigs[i]), i
    cert = [i for i in range(120) if w.slot[i] == 0]
    csig = [_doubled(w.sig[i]) if c % 4 == 1 else w.sig[i] for c, i in enumerate(cert)]
    got = ctx.bls_verify_batch(w.kid, csig, [w.msgs[i] for i in cert])
    assert got.tolist() == [c % 4 != 1 for c in range(len(cert))]


def test_hash_tries_and_lengths(ctx):
    """The whole signing fixture as one batch (lengths 0 .. 4,096, 0 .. 16 increments) under a key set of
    the fixture signers' vks: valid under their own keys, invalid under the next signer's."""
    signers, vectors = load_fixture()
    tid = ctx.load_bls_signers([sk for sk, _ in signers], [sid for _, sid in signers])
    try:
        vks = ctx.bls_signer_public_keys(tid)
    finally:
        ctx.unload_bls_signers(tid)
    ns = len(signers)
    assert len({sk % B.R for sk, _ in signers}) == ns  # no two signers share a key: "next" is another key
    order = list(range(len(vectors)))
    random.Random(6).shuffle(order)
    kid = ctx.bls_load_keys(vks[0], vks)
    try:
        assert all(ctx.bls_key_status(kid, ns))
        sigs = [vectors[i].share[4:] for i in order]
        msgs = [vectors[i].msg for i in order]
        own = ctx.bls_verify_batch(kid, sigs, msgs, [vectors[i].signer + 1 for i in order])
        nxt = ctx.bls_verify_batch(kid, sigs, msgs, [(vectors[i].signer + 1) % ns + 1 for i in order])
    finally:
        ctx.bls_unload_keys(kid)
    assert own.all(), f"records {[order[j] for j in np.nonzero(~own)[0][:8]]} rejected under their own key"
    assert not nxt.any()


def test_bad_keys(ctx, w):
    """An undecodable vk_j and an undecodable PK give 0 exactly for the items under those slots."""
    vks = list(w.vks)
    vks[6] = b"\x05" + bytes(64)
    kid = ctx.bls_load_keys(b"\x02" + B.P.to_bytes(32, "big") + bytes(32), vks)
    try:
        st = ctx.bls_key_status(kid, NKEYS)
        assert [bool(s) for s in st] == [i not in (0, 7) for i in range(NKEYS + 1)]
        got = ctx.bls_verify_batch(kid, w.sig[:80], w.msgs[:80], w.slot[:80])
    finally:
        ctx.bls_unload_keys(kid)
    assert got.tolist() == [s not in (0, 7) for s in w.slot[:80]]
    assert {0, 7} <= set(w.slot[:80])


def _raw(c, kid, key_idx, sigs, blob, off, lens, m, msg_of, n, bitmap):
    return c.lib.cbft_bls_verify_batch(c.handle, kid, _p(key_idx), _p(sigs), _p(blob), _p(off), _p(lens), m, _p(msg_of),
                                       n, _p(bitmap))


def test_argument_errors(ctx, w):
    n = 5
    blob, off, lens = pack(w.msgs[:n])
    sigs = np.frombuffer(b"".join(w.sig[:n]), dtype=np.uint8).copy()
    slots = np.array(w.slot[:n], dtype=np.uint32)
    ident = np.arange(n, dtype=np.uint32)

    def refused(*a):
        bm = np.full(1, 0xAA, dtype=np.uint8)
        return _raw(*a, bm) == EINVAL and bm[0] == 0xAA

    assert refused(ctx, w.kid + 1000, slots, sigs, blob, off, lens, n, None, n), "unknown key set"
    bad = slots.copy()
    bad[3] = NKEYS + 1
    assert refused(ctx, w.kid, bad, sigs, blob, off, lens, n, None, n), "key_idx > n_keys"
    bad = ident.copy()
    bad[4] = n
    assert refused(ctx, w.kid, slots, sigs, blob, off, lens, n, bad, n), "msg_of >= m"
    big = lens.copy()
    big[2] = 0xFFFFFF01
    assert refused(ctx, w.kid, slots, sigs, blob, off, big, n, None, n), "msg_len > 0xFFFFFF00"
    assert refused(ctx, w.kid, slots, sigs, blob, off, lens, n - 1, None, n), "msg_of = nullptr with m != n"
    bm = np.full(1, 0xAA, dtype=np.uint8)
    assert _raw(ctx, w.kid, None, None, None, None, None, 0, None, 0, bm) == 0 and bm[0] == 0xAA, "n = 0"
    bm = np.full(1, 0xFF, dtype=np.uint8)  # trailing bits of the last byte are cleared
    assert _raw(ctx, w.kid, slots, sigs, blob, off, lens, n, ident, n, bm) == 0 and bm[0] == 0x1F
    slots[n - 1] = NKEYS  # the last slot itself is in range
    bm = np.full(1, 0xFF, dtype=np.uint8)
    assert _raw(ctx, w.kid, slots, sigs, blob, off, lens, n, None, n, bm) == 0 and bm[0] == (0x0F if w.slot[4] != NKEYS else 0x1F)
    with cb.Context(devices=[0, 0]) as two:  # device pointers belong to one GPU
        assert two.lib.cbft_bls_verify_fixed_device(two.handle, 1, None, None, None, 0, 0, None, 0, None, None) == EINVAL


def test_device_form(w):
    """cbft_bls_verify_fixed_device: the host form's verdicts for n = 257; two calls on two streams that
    share the scratch both come out right; out-of-range d_key_idx / d_msg_of entries give 0."""
    hip = Hip()
    n = 257
    slots, sigs, msgs, exp = _spoiled(w, n)
    # second batch: the same items in reverse, through an explicit msg_of over the forward messages
    sig_b = np.frombuffer(b"".join(reversed(sigs)), dtype=np.uint8).copy()
    slot_b = np.array(slots[::-1], dtype=np.uint32)
    mof_b = np.arange(n - 1, -1, -1, dtype=np.uint32)
    sig_a = np.frombuffer(b"".join(sigs), dtype=np.uint8).copy()
    slot_a = np.array(slots, dtype=np.uint32)
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    bad_key, bad_msg = [0, 64, 200], [1, 63, n - 1]
    slot_c = slot_a.copy()
    slot_c[bad_key] = np.array([NKEYS + 1, 0xFFFFFFFF, 1 << 20], dtype=np.uint32)
    mof_c = np.arange(n, dtype=np.uint32)
    mof_c[bad_msg] = np.array([n, 0xFFFFFFFF, n + 7], dtype=np.uint32)
    try:
        with cb.Context(device=0) as c:
            kid = c.bls_load_keys(w.pk, w.vks)
            host = c.bls_verify_batch(kid, sigs, msgs, slots)
            d_blob = hip.to_dev(blob)
            s0, s1 = hip.stream(), hip.stream()
            out = [hip.to_dev(np.full(n, 0xA5, dtype=np.uint8)) for _ in range(3)]
            c.bls_verify_fixed_device(kid, hip.to_dev(slot_a), hip.to_dev(sig_a), d_blob, 32, n, 0, n, out[0], s0)
            c.bls_verify_fixed_device(kid, hip.to_dev(slot_b), hip.to_dev(sig_b), d_blob, 32, n, hip.to_dev(mof_b), n,
                                      out[1], s1)
            c.bls_verify_fixed_device(kid, hip.to_dev(slot_c), hip.to_dev(sig_a), d_blob, 32, n, hip.to_dev(mof_c), n,
                                      out[2], 0)
            hip.sync()
            got = [hip.from_dev(o, n) for o in out]
            c.bls_unload_keys(kid)
    finally:
        hip.close()
    assert host.tolist() == exp
    assert got[0].tolist() == [int(e) for e in exp]
    assert got[1].tolist() == [int(e) for e in exp[::-1]]
    want = [int(e and i not in bad_key and i not in bad_msg) for i, e in enumerate(exp)]
    assert got[2].tolist() == want


@pytest.mark.parametrize("devices", [[0, 0], [0] * 4])
def test_multi_device(ctx, w, devices):
    """n = 301 items over m = 7 messages cut into one slice per device, each hashing only the messages
    its slice names: the merged bitmap equals the single-device one."""
    rng = random.Random(8)
    n, m = 301, GRID_MSGS
    signer = [rng.randrange(NKEYS) for _ in range(n)]
    # runs of one message, so that a slice names a subset of the messages
    signed = sorted(rng.randrange(m) for _ in range(n))
    named = [(j + 3) % m if i % 13 == 5 else j for i, j in enumerate(signed)]
    sigs = [w.grid[j][s] for s, j in zip(signer, signed)]
    slots = [s + 1 for s in signer]
    want = ctx.bls_verify_batch(w.kid, sigs, w.msgs[:m], slots, named)
    assert want.tolist() == [a == b for a, b in zip(signed, named)]
    s2, g2, m2, e2 = _spoiled(w, n)
    with cb.Context(devices=devices) as g:
        gk = g.bls_load_keys(w.pk, w.vks)
        try:
            got = g.bls_verify_batch(gk, sigs, w.msgs[:m], slots, named)
            ident = g.bls_verify_batch(gk, g2, m2, s2)  # msg_of = None: each slice's own message range
        finally:
            g.bls_unload_keys(gk)
    assert got.tolist() == want.tolist()
    assert ident.tolist() == e2
