"""GPU tests of batched BLS multisig verification over many signer sets (cbft_bls_verify_multisig_batch,
cbft_bls_verify_multisig_fixed_device, cbft_bls_sum_keys_batch) through the C ABI.  Shares come from
ctx.bls_sign_batch and certificates from ctx.bls_combine(..., multisig=True) (both pinned to the oracle
by their own tests); expected verdicts come by construction, from the lone cbft_bls_verify_multisig (an
independent kernel) and, on at most 8 cached samples per test, from the Python oracle's pairing under
the sum of the decoded keys."""
import ctypes
import random

import numpy as np
import pytest

import blsgen
import bn254_ref as B
import cbft_hipcrypto as cb
import relic_keys
from bls_sign_vectors import pack
from sign_vectors import Hip

pytestmark = pytest.mark.gpu
EINVAL = -22
NMAX = 1100
NKEYS, THRESH = 16, 11
NSETS = 16
GRID_MSGS = 7  # messages every signer signs (free subsets, msg_of, multi-device)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ids(r):
    """Signer subset r of the 16-key world: 11 consecutive ids starting at r + 1, wrapping."""
    return sorted((r + t) % NKEYS + 1 for t in range(THRESH))


def _bitmap(ids):
    return B.signers_bitmap(ids)


class World:
    """One 16-key set, NMAX distinct 32-byte messages; item i = the multisig certificate of subset
    i % 16 (11 signers) on message i; and every signer's share of the first GRID_MSGS messages."""

    def __init__(self, ctx):
        self.sk, self.sks, self.pk, self.vks = blsgen.keyset(NKEYS, THRESH, seed=0x25B)
        rng = random.Random(0x25C)
        self.msgs = [rng.randbytes(32) for _ in range(NMAX)]
        self.subset = [i % NSETS for i in range(NMAX)]
        self.sets = [_bitmap(_ids(r)) for r in range(NSETS)]
        jobs = [(s - 1, i) for i in range(NMAX) for s in _ids(self.subset[i])]  # (signer index, message index)
        grid_at = len(jobs)
        jobs += [(s, j) for j in range(GRID_MSGS) for s in range(NKEYS)]
        tid = ctx.load_bls_signers([self.sks[i] for i in range(1, NKEYS + 1)], list(range(1, NKEYS + 1)))
        try:
            out = ctx.bls_sign_batch(tid, [self.msgs[m] for _, m in jobs], [s for s, _ in jobs])
        finally:
            ctx.unload_bls_signers(tid)
        self.sig = [ctx.bls_combine([out[THRESH * i + j].tobytes() for j in range(THRESH)], multisig=True)
                    for i in range(NMAX)]
        # grid[j][s]: 37-byte share of signer s + 1 on message j
        self.grid = [[out[grid_at + j * NKEYS + s].tobytes() for s in range(NKEYS)] for j in range(GRID_MSGS)]
        self.ctx = ctx
        self.kid = ctx.bls_load_keys(self.pk, self.vks)
        self._keys = {}
        self._oracle = {}

    def cert(self, j, ids):
        """The multisig certificate of signers ids on message j < GRID_MSGS."""
        return self.ctx.bls_combine([self.grid[j][s - 1] for s in ids], multisig=True)

    def oracle(self, bitmap, msg, sig33):
        k = (bitmap, msg, sig33)
        if k not in self._oracle:
            pk = None
            for i in range(NKEYS):
                if (bitmap[i >> 3] >> (i & 7)) & 1:
                    if i not in self._keys:
                        self._keys[i] = B.g2_from_bytes(self.vks[i])
                    pk = B.ec_add(pk, self._keys[i], None)
            self._oracle[k] = pk is not None and B.verify(msg, sig33, pk)
        return self._oracle[k]

    def lone(self, ctx, bitmap, msg, sig33):
        return ctx.bls_verify_multisig(self.kid, msg, sig33, bitmap)


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
    """Items 0 .. n - 1 with every 7th spoiled, cycling through wrong message, wrong set (the next
    subset) and doubled point: (set indices, sigs, msgs, expected)."""
    sof, sigs, msgs = list(w.subset[:n]), list(w.sig[:n]), list(w.msgs[:n])
    exp = [True] * n
    for c, i in enumerate(range(3, n, 7)):
        exp[i] = False
        if c % 3 == 0:
            msgs[i] = bytes([msgs[i][0] ^ 0x40]) + msgs[i][1:]
        elif c % 3 == 1:
            sof[i] = (sof[i] + 1) % NSETS
        else:
            sigs[i] = _doubled(sigs[i])
    return sof, sigs, msgs, exp


def test_verdict_table(ctx, w):
    """Every malformed sigma of test_bls_verify_batch_gpu.py::test_verdict_table under a good set, each on
    its own message; a good sigma under a set missing one signer, under a set with one extra signer and
    under the right set on the wrong message; valid items among them.  All equal the lone call, samples
    the oracle."""
    x = next(x for x in range(1, 100) if pow((x ** 3 + 2) % B.P, (B.P - 1) // 2, B.P) != 1)
    items = []  # (bitmap, msg, sig33)
    for case in range(9):
        i = case
        s = w.sig[i]
        if case == 1:  # signer 6's lone point on this message, under this item's set
            assert i < GRID_MSGS
            s = w.grid[i][5][4:]
        bad = [_doubled(s), s, b"\x05" + s[1:], b"\x02" + B.P.to_bytes(32, "big"), b"\x02" + x.to_bytes(32, "big"),
               b"\x03" + x.to_bytes(32, "big"), bytes(33), b"\x00\x01" + bytes(31), bytes([s[0] ^ 1]) + s[1:]][case]
        items.append((w.sets[w.subset[i]], w.msgs[i], bad))
    ids = _ids(w.subset[9])
    items.append((_bitmap(ids[1:]), w.msgs[9], w.sig[9]))  # one signer missing from the set
    extra = next(e for e in range(1, NKEYS + 1) if e not in ids)
    items.append((_bitmap(ids + [extra]), w.msgs[9], w.sig[9]))  # one signer too many
    items.append((w.sets[w.subset[9]], w.msgs[10], w.sig[9]))  # the right set, another message
    items += [(w.sets[w.subset[i]], w.msgs[i], w.sig[i]) for i in (9, 10, 11)]
    random.Random(1).shuffle(items)
    got = ctx.bls_verify_multisig_batch(w.kid, [s for _, _, s in items], [m for _, m, _ in items],
                                        [b for b, _, _ in items])
    lone = [w.lone(ctx, *it) for it in items]
    assert got.tolist() == lone
    assert sum(lone) == 3
    for it, g in list(zip(items, got))[:8]:
        assert bool(g) == w.oracle(*it)


def test_exceptional_sets(ctx, w):
    """Key sums that meet the exceptional cases of the group law: vk_2 = -vk_1, vk_4 = vk_3, vk_6
    undecodable."""
    sk, sks, pk, vks = blsgen.keyset(6, 4, seed=0x25D)
    vks = list(vks)
    vks[1] = bytes([vks[0][0] ^ 1]) + vks[0][1:]
    vks[3] = vks[2]
    vks[5] = b"\x05" + bytes(64)
    msg = w.msgs[0]
    sg = {i: blsgen.sign_point(sks[i], msg) for i in (1, 3, 5)}
    wide = bytearray(_bitmap([5, 7]))
    wide[255] |= 0x80  # id 2048
    cases = [  # (ids or bitmap, sigma, expected)
        ([1, 2], sg[1], False),            # the sum is the point at infinity
        ([1, 2], bytes(33), False),        # and stays unusable for an infinite sigma
        ([3, 4], _doubled(sg[3]), True),   # a doubling inside the key sum
        ([3, 4], sg[3], False),
        ([1, 2, 5], sg[5], True),          # an infinite running sum, then a key
        ([5, 6], sg[5], False),            # selects the undecodable key
        ([5], sg[5], True),                # its neighbours are unaffected
        ([1, 2, 5, 6], sg[5], False),
        ([], sg[5], False),                # the empty set
        ([], bytes(33), False),
        (bytes(wide), sg[5], True),        # ids 7 and 2048 are above n_keys: ignored
        ([5], sg[5], True),
    ]
    sets = [c[0] if isinstance(c[0], bytes) else _bitmap(c[0]) for c in cases]
    kid = ctx.bls_load_keys(pk, vks)
    try:
        assert [bool(s) for s in ctx.bls_key_status(kid, 6)][1:] == [True] * 5 + [False]
        got = ctx.bls_verify_multisig_batch(kid, [c[1] for c in cases], [msg], sets, msg_of=[0] * len(cases))
        lone = [ctx.bls_verify_multisig(kid, msg, c[1], b) for c, b in zip(cases, sets)]
        sums, ok = ctx.bls_sum_keys_batch(kid, sets)
        lone_sums = [ctx.bls_sum_keys(kid, b) for b in sets]
    finally:
        ctx.bls_unload_keys(kid)
    assert got.tolist() == [c[2] for c in cases]
    assert lone == [c[2] for c in cases]
    assert sums == lone_sums
    assert ok.tolist() == [0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1]
    assert sums[0] == bytes(65) and sums[5] == bytes(65) and sums[8] == bytes(65)
    assert sums[4] == vks[4] == sums[6] == sums[10]
    two_vk3 = B.g2_from_bytes(vks[2])
    assert sums[2] == B.g2_to_bytes(B.ec_add(two_vk3, two_vk3, None))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, NMAX])
def test_size_edges(ctx, w, n):
    """Distinct 32-byte messages over the 16 sets: lane and wave edges of the decode, the hash kernel's
    256-message block, more waves than the chip's 1,024 SIMDs.  Every 7th item spoiled."""
    sof, sigs, msgs, exp = _spoiled(w, n)
    got = ctx.bls_verify_multisig_batch(w.kid, sigs, msgs, w.sets, set_of=sof)
    bad = np.nonzero(got != np.array(exp))[0]
    assert bad.size == 0, f"{bad.size} of {n} differ from the construction, first {bad[:8]}"
    rng = random.Random(n)
    for i in sorted(rng.sample(range(n), min(n, 16))):
        assert bool(got[i]) == w.lone(ctx, w.sets[sof[i]], msgs[i], sigs[i]), f"item {i} differs from the lone call"
    pool = sorted(set(range(3, n, 7)) | set(range(0, n, 5)))[:8] or [0]  # shared by every n: cached
    for i in pool[:8]:
        assert bool(got[i]) == w.oracle(w.sets[sof[i]], msgs[i], sigs[i]), f"item {i} differs from the oracle"


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 257])
def test_set_count_edges(ctx, w, s):
    """s set entries (the world's 16 subsets, repeats as distinct entries), item i under entry i: set_of =
    None equals an explicit identity and the construction; every 7th spoiled."""
    sof, sigs, msgs, exp = _spoiled(w, s)
    sets = [w.sets[j] for j in sof]
    a = ctx.bls_verify_multisig_batch(w.kid, sigs, msgs, sets)
    b = ctx.bls_verify_multisig_batch(w.kid, sigs, msgs, sets, set_of=list(range(s)), msg_of=list(range(s)))
    assert a.tolist() == b.tolist() == exp
    sums, ok = ctx.bls_sum_keys_batch(w.kid, sets)
    assert ok.tolist() == [1] * s
    for j in sorted({0, s // 2, s - 1}):
        assert sums[j] == ctx.bls_sum_keys(w.kid, sets[j])


def test_wide_bitmaps(ctx):
    """A key set of 2,048 keys: cbft_bls_sum_keys_batch equals cbft_bls_sum_keys byte for byte on bitmaps
    that fill, start, end and straddle the key-sum chunks, and a certificate of 683 signers verifies."""
    n = 2048
    rng = random.Random(0x25E)
    sks = [rng.randrange(1, B.R) for _ in range(n)]
    pick = sorted(rng.sample(range(1, n + 1), 683))
    sets = [_bitmap(range(1, n + 1)), _bitmap([1]), _bitmap([n]), _bitmap([64, 65, 128, 129]), _bitmap(pick)]
    msg = b"wide bitmap certificate".ljust(32, b".")
    tid = ctx.load_bls_signers(sks, list(range(1, n + 1)))
    try:
        vks = ctx.bls_signer_public_keys(tid)
        shares = ctx.bls_sign_batch(tid, [msg] * len(pick), [i - 1 for i in pick])
    finally:
        ctx.unload_bls_signers(tid)
    sig = ctx.bls_combine([s.tobytes() for s in shares], multisig=True)
    kid = ctx.bls_load_keys(vks[0], vks)
    try:
        sums, ok = ctx.bls_sum_keys_batch(kid, sets)
        lone = [ctx.bls_sum_keys(kid, b) for b in sets]
        got = ctx.bls_verify_multisig_batch(kid, [sig, _doubled(sig), sig, sig], [msg], [sets[4], sets[0]],
                                            set_of=[0, 0, 1, 0], msg_of=[0] * 4)
        assert ctx.bls_verify_multisig(kid, msg, sig, sets[4])
    finally:
        ctx.bls_unload_keys(kid)
    assert sums == lone
    assert ok.tolist() == [1] * 5
    assert sums[1] == vks[0] and sums[2] == vks[n - 1]
    assert got.tolist() == [True, False, False, True]


def test_sum_keys_batch_oracle(ctx):
    """The reference's RELIC key files, 8 subsets per set: the 65 bytes are g2_to_bytes of the oracle's sum
    of the decoded keys."""
    rng = random.Random(0x25F)
    for sysm in relic_keys.load():
        keys = [B.g2_from_bytes(v) for v in sysm.vks]
        subsets = [list(range(1, sysm.n + 1)), [1], [sysm.n]]
        while len(subsets) < 8:
            subsets.append(sorted(rng.sample(range(1, sysm.n + 1), rng.randrange(1, sysm.n + 1))))
        kid = ctx.bls_load_keys(sysm.pk, sysm.vks)
        try:
            sums, ok = ctx.bls_sum_keys_batch(kid, [_bitmap(s) for s in subsets])
        finally:
            ctx.bls_unload_keys(kid)
        for ids, got, good in zip(subsets, sums, ok):
            want = None
            for i in ids:
                want = B.ec_add(want, keys[i - 1], None)
            assert got == B.g2_to_bytes(want), f"{sysm.name} {ids}"
            assert good == 1


def test_bad_keys(ctx, w):
    """The key set of test_bls_verify_batch_gpu.py::test_bad_keys (vk_7 and the PK undecodable): exactly
    the items whose set selects id 7 give 0."""
    vks = list(w.vks)
    vks[6] = b"\x05" + bytes(64)
    kid = ctx.bls_load_keys(b"\x02" + B.P.to_bytes(32, "big") + bytes(32), vks)
    try:
        got = ctx.bls_verify_multisig_batch(kid, w.sig[:80], w.msgs[:80], w.sets, set_of=w.subset[:80])
    finally:
        ctx.bls_unload_keys(kid)
    want = [7 not in _ids(r) for r in w.subset[:80]]
    assert got.tolist() == want
    assert 0 < sum(want) < 80


def _raw(c, kid, sets, s, set_of, sigs, blob, off, lens, m, msg_of, n, bitmap):
    return c.lib.cbft_bls_verify_multisig_batch(c.handle, kid, _p(sets), s, _p(set_of), _p(sigs), _p(blob), _p(off),
                                                _p(lens), m, _p(msg_of), n, _p(bitmap))


def test_argument_errors(ctx, w):
    n = 5
    blob, off, lens = pack(w.msgs[:n])
    sigs = np.frombuffer(b"".join(w.sig[:n]), dtype=np.uint8).copy()
    sets = np.frombuffer(b"".join(w.sets), dtype=np.uint8).copy()
    sof = np.array(w.subset[:n], dtype=np.uint32)
    ident = np.arange(n, dtype=np.uint32)

    def refused(*a):
        bm = np.full(1, 0xAA, dtype=np.uint8)
        return _raw(*a, bm) == EINVAL and bm[0] == 0xAA

    assert refused(ctx, w.kid + 1000, sets, NSETS, sof, sigs, blob, off, lens, n, None, n), "unknown key set"
    assert refused(ctx, w.kid, None, NSETS, sof, sigs, blob, off, lens, n, None, n), "null bitmaps"
    assert refused(ctx, w.kid, sets, NSETS, sof, None, blob, off, lens, n, None, n), "null signatures"
    assert refused(ctx, w.kid, sets, NSETS, sof, sigs, blob, None, lens, n, None, n), "null offsets"
    assert refused(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, None, n, None, n), "null lengths"
    assert _raw(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, lens, n, None, n, None) == EINVAL, "null output"
    bad = sof.copy()
    bad[3] = NSETS
    assert refused(ctx, w.kid, sets, NSETS, bad, sigs, blob, off, lens, n, None, n), "set_of >= s"
    bad = ident.copy()
    bad[4] = n
    assert refused(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, lens, n, bad, n), "msg_of >= m"
    big = lens.copy()
    big[2] = 0xFFFFFF01
    assert refused(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, big, n, None, n), "msg_len > 0xFFFFFF00"
    assert refused(ctx, w.kid, sets, NSETS, None, sigs, blob, off, lens, n, None, n), "set_of = nullptr with s != n"
    assert refused(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, lens, n - 1, None, n), "msg_of = nullptr with m != n"
    bm = np.full(1, 0xAA, dtype=np.uint8)
    assert _raw(ctx, w.kid, None, 0, None, None, None, None, None, 0, None, 0, bm) == 0 and bm[0] == 0xAA, "n = 0"
    bm = np.full(1, 0xFF, dtype=np.uint8)  # trailing bits of the last byte are cleared
    assert _raw(ctx, w.kid, sets, NSETS, sof, sigs, blob, off, lens, n, ident, n, bm) == 0 and bm[0] == 0x1F
    out = np.full(65, 0xAA, dtype=np.uint8)
    okb = np.full(1, 0xAA, dtype=np.uint8)
    assert ctx.lib.cbft_bls_sum_keys_batch(ctx.handle, w.kid + 1000, _p(sets), 1, _p(out), _p(okb)) == EINVAL
    assert ctx.lib.cbft_bls_sum_keys_batch(ctx.handle, w.kid, None, 1, _p(out), _p(okb)) == EINVAL
    assert out[0] == 0xAA and okb[0] == 0xAA
    assert ctx.lib.cbft_bls_sum_keys_batch(ctx.handle, w.kid, None, 0, None, None) == 0
    with cb.Context(devices=[0, 0]) as two:  # device pointers belong to one GPU
        assert two.lib.cbft_bls_verify_multisig_fixed_device(two.handle, 1, None, 0, None, None, None, 0, 0, None, 0,
                                                             None, None) == EINVAL


def test_device_form(w):
    """cbft_bls_verify_multisig_fixed_device: the host form's verdicts for n = 257; two calls on two streams
    that share the scratch both come out right; out-of-range d_set_of / d_msg_of entries give 0."""
    hip = Hip()
    n = 257
    sof, sigs, msgs, exp = _spoiled(w, n)
    # first batch: one bitmap per item (d_set_of = 0); second: the items in reverse over the 16 sets
    own = np.frombuffer(b"".join(w.sets[j] for j in sof), dtype=np.uint8).copy()
    sets = np.frombuffer(b"".join(w.sets), dtype=np.uint8).copy()
    sig_a = np.frombuffer(b"".join(sigs), dtype=np.uint8).copy()
    sig_b = np.frombuffer(b"".join(reversed(sigs)), dtype=np.uint8).copy()
    sof_a = np.array(sof, dtype=np.uint32)
    sof_b = np.array(sof[::-1], dtype=np.uint32)
    mof_b = np.arange(n - 1, -1, -1, dtype=np.uint32)
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    bad_set, bad_msg = [0, 64, 200], [1, 63, n - 1]
    sof_c = sof_a.copy()
    sof_c[bad_set] = np.array([NSETS, 0xFFFFFFFF, 1 << 20], dtype=np.uint32)
    mof_c = np.arange(n, dtype=np.uint32)
    mof_c[bad_msg] = np.array([n, 0xFFFFFFFF, n + 7], dtype=np.uint32)
    try:
        with cb.Context(device=0) as c:
            kid = c.bls_load_keys(w.pk, w.vks)
            host = c.bls_verify_multisig_batch(kid, sigs, msgs, w.sets, set_of=sof)
            d_blob, d_sets = hip.to_dev(blob), hip.to_dev(sets)
            s0, s1 = hip.stream(), hip.stream()
            out = [hip.to_dev(np.full(n, 0xA5, dtype=np.uint8)) for _ in range(3)]
            c.bls_verify_multisig_fixed_device(kid, hip.to_dev(own), n, 0, hip.to_dev(sig_a), d_blob, 32, n, 0, n,
                                               out[0], s0)
            c.bls_verify_multisig_fixed_device(kid, d_sets, NSETS, hip.to_dev(sof_b), hip.to_dev(sig_b), d_blob, 32, n,
                                               hip.to_dev(mof_b), n, out[1], s1)
            c.bls_verify_multisig_fixed_device(kid, d_sets, NSETS, hip.to_dev(sof_c), hip.to_dev(sig_a), d_blob, 32, n,
                                               hip.to_dev(mof_c), n, out[2], 0)
            hip.sync()
            got = [hip.from_dev(o, n) for o in out]
            c.bls_unload_keys(kid)
    finally:
        hip.close()
    assert host.tolist() == exp
    assert got[0].tolist() == [int(e) for e in exp]
    assert got[1].tolist() == [int(e) for e in exp[::-1]]
    want = [int(e and i not in bad_set and i not in bad_msg) for i, e in enumerate(exp)]
    assert got[2].tolist() == want


def test_pipeline(w):
    """cbft_bls_sign_fixed_device -> cbft_bls_combine_fixed_device (multisig) ->
    cbft_bls_verify_multisig_fixed_device on one stream with nothing copied to the host in between: 65
    certificates of k = 11 whose signer subsets rotate through the 16 sets all verify; with the bitmaps of 5
    certificates shifted by one signer exactly those 5 do not."""
    hip = Hip()
    m, k = 65, THRESH
    msgs = w.msgs[:m]
    signer = np.array([s - 1 for c in range(m) for s in _ids(c % NSETS)], dtype=np.uint32)
    rep = np.frombuffer(b"".join(msgs[c] for c in range(m) for _ in range(k)), dtype=np.uint8).copy()
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    good = np.frombuffer(b"".join(w.sets[c % NSETS] for c in range(m)), dtype=np.uint8).copy()
    shifted = [2, 17, 33, 48, 64]
    off = np.frombuffer(b"".join(w.sets[(c + 1) % NSETS] if c in shifted else w.sets[c % NSETS] for c in range(m)),
                        dtype=np.uint8).copy()
    try:
        with cb.Context(device=0) as c:
            kid = c.bls_load_keys(w.pk, w.vks)
            tid = c.load_bls_signers([w.sks[i] for i in range(1, NKEYS + 1)], list(range(1, NKEYS + 1)))
            s = hip.stream()
            d_sh = hip.to_dev(np.full(37 * m * k, 0xA5, dtype=np.uint8))
            d_sig = hip.to_dev(np.full(33 * m, 0xA5, dtype=np.uint8))
            d_st = hip.to_dev(np.full(m, 0xA5, dtype=np.uint8))
            d_v = [hip.to_dev(np.full(m, 0xA5, dtype=np.uint8)) for _ in range(2)]
            d_blob = hip.to_dev(blob)
            c.bls_sign_fixed_device(tid, hip.to_dev(signer), hip.to_dev(rep), 32, m * k, d_sh, s)
            c.bls_combine_fixed_device(d_sh, k, m, 0, True, d_sig, d_st, s)
            c.bls_verify_multisig_fixed_device(kid, hip.to_dev(good), m, 0, d_sig, d_blob, 32, m, 0, m, d_v[0], s)
            c.bls_verify_multisig_fixed_device(kid, hip.to_dev(off), m, 0, d_sig, d_blob, 32, m, 0, m, d_v[1], s)
            hip.sync()
            status = hip.from_dev(d_st, m).tolist()
            sigs = hip.from_dev(d_sig, 33 * m).tobytes()
            v = [hip.from_dev(d, m).tolist() for d in d_v]
            c.unload_bls_signers(tid)
            c.bls_unload_keys(kid)
    finally:
        hip.close()
    assert status == [1] * m
    assert [sigs[33 * c:33 * c + 33] for c in range(NSETS)] == w.sig[:NSETS]  # the world's own certificates
    assert v[0] == [1] * m
    assert v[1] == [0 if c in shifted else 1 for c in range(m)]


@pytest.mark.parametrize("devices", [[0, 0], [0] * 4])
def test_multi_device(ctx, w, devices):
    """n = 301 items over 7 messages and 9 sets, in runs, cut into one slice per device, each summing only
    the sets and hashing only the messages its slice names: the merged bitmap equals the single-device one."""
    rng = random.Random(8)
    n, m, s = 301, GRID_MSGS, 9
    subsets = [sorted(rng.sample(range(1, NKEYS + 1), rng.randrange(1, NKEYS + 1))) for _ in range(s)]
    sets = [_bitmap(x) for x in subsets]
    cert = {(j, r): w.cert(j, subsets[r]) for j in range(m) for r in range(s)}
    signed = sorted(rng.randrange(m) for _ in range(n))  # runs of one message
    used = sorted((rng.randrange(s) for _ in range(n)), key=lambda r: (r * 5) % s)  # runs of one set
    named = [(j + 3) % m if i % 13 == 5 else j for i, j in enumerate(signed)]
    under = [(r + 1) % s if i % 17 == 9 else r for i, r in enumerate(used)]
    sigs = [cert[(j, r)] for j, r in zip(signed, used)]
    want = ctx.bls_verify_multisig_batch(w.kid, sigs, w.msgs[:m], sets, set_of=under, msg_of=named)
    assert want.tolist() == [a == b and subsets[q] == subsets[r] for a, b, q, r in zip(signed, named, used, under)]
    sof2, g2, m2, e2 = _spoiled(w, n)
    own = [w.sets[j] for j in sof2]
    with cb.Context(devices=devices) as g:
        gk = g.bls_load_keys(w.pk, w.vks)
        try:
            got = g.bls_verify_multisig_batch(gk, sigs, w.msgs[:m], sets, set_of=under, msg_of=named)
            ident = g.bls_verify_multisig_batch(gk, g2, m2, own)  # set_of = msg_of = None: each slice's own ranges
        finally:
            g.bls_unload_keys(gk)
    assert got.tolist() == want.tolist()
    assert ident.tolist() == e2
