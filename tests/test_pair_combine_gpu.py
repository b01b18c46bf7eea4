"""The pair ladder's split closing sum (pair_combine_split in ed25519_comb2_ladder_kernel) on the GPU:
bit-exact verdicts on the golden vectors at comb geometries with odd position counts (lane 1's last
step is then an identity addition before the closing sum), and on a crafted batch whose lane sums are
the identity on one or both sides of the closing sum."""
import numpy as np
import pytest

import cbft_hipcrypto as cb
import ed25519_ref as ref
from golden_io import load_ed25519_vectors
import workload as sigsets

pytestmark = pytest.mark.gpu

IDENTITY_KEY = bytes([1]) + bytes(31)  # y = 1, x = 0


@pytest.fixture(scope="module")
def golden():
    vs = load_ed25519_vectors()
    keys = sorted({v.pk for v in vs})
    index = {k: i for i, k in enumerate(keys)}
    return (keys, [index[v.pk] for v in vs], [v.sig for v in vs], [v.msg for v in vs],
            np.array([bool(v.verdict) for v in vs]))


# radix 14: 19 key positions, B radix 23: 11 positions (odd counts); 13 + 22 is the default 20 + 12
@pytest.mark.parametrize("b_radix", [16, 22, 23])
@pytest.mark.parametrize("radix", [8, 13, 14])
def test_pair_combine_golden(golden, radix, b_radix):
    keys, kidx, sigs, msgs, exp = golden
    with cb.Context(device=0) as c:
        c.set_option(cb.OPT_LADDER_LANES, 2).set_option(cb.OPT_B_RADIX, b_radix)
        tid = c.load_keys(keys, radix=radix)
        got = cb.bitmap_to_bools(c.verify(tid, kidx, sigs, msgs), len(exp))
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]


def crafted_batch():
    """130 signatures (two full 128-lane blocks and two live pairs in a third).  Under the key whose
    encoding is the identity point [h]A vanishes, so R' = [S]B: with B's 12 radix-2^22 positions
    split 6 + 6 over the lanes, S below 2^132 leaves lane 1's sum the identity, S with bits from 132
    up only leaves lane 0's, S = 0 both.  R is the encoding of [S]B; a second copy has a bit of R
    flipped.  The rest are ordinary valid and planted-invalid signatures."""
    n, nkeys = 130, 8
    ss = sigsets.make_sigset(n, nkeys=nkeys, msg_len=256, seed=0x9A12C0, invalid_frac=0.2, threads=4,
                             compute_expected=False)
    ss.pk = np.ascontiguousarray(np.vstack([ss.pk, np.frombuffer(IDENTITY_KEY, dtype=np.uint8)[None, :]]))
    rng = np.random.default_rng(132)
    low = int.from_bytes(rng.bytes(17), "little") % 2**132 | 1
    high = (int.from_bytes(rng.bytes(15), "little") % 2**118 | 1) << 132
    assert 0 < low < 2**132 and high % 2**132 == 0 and high < ref.L
    scalars = [0, 1, 2**132, low, high]
    crafted = []
    for s in scalars:
        r = ref.encode_point(ref.scalar_mult(s, ref.B))
        crafted.append(np.frombuffer(r + s.to_bytes(32, "little"), dtype=np.uint8))
    flipped = []
    for k, sig in enumerate(crafted):
        f = sig.copy()
        f[3 * k] ^= 1 << k  # one bit of R
        flipped.append(f)
    # the crafted ones at the head of the first block, and one pair of them in the tail block
    where = list(range(10)) + [128, 129]
    sigs = crafted + flipped + [crafted[3], flipped[4]]
    for i, sig in zip(where, sigs):
        ss.sig[i] = sig
        ss.key_idx[i] = nkeys
    ss.expected = sigsets.cpu_verify(ss, threads=4).astype(bool)
    return ss, where


@pytest.fixture(scope="module")
def crafted():
    ss, where = crafted_batch()
    exp = ss.expected
    # both verdicts occur among the crafted signatures and among the ordinary ones, so neither an
    # all-zero nor an all-one bitmap can pass
    rest = np.setdiff1d(np.arange(ss.n), where)
    assert exp[where].any() and not exp[where].all()
    assert exp[rest].any() and not exp[rest].all()
    return ss


def test_pair_combine_crafted_identity_sums(crafted):
    ss = crafted
    with cb.Context(device=0) as c:
        c.set_option(cb.OPT_LADDER_LANES, 2)
        tid = c.load_keys(ss.pk)
        got = cb.bitmap_to_bools(c.verify_packed(tid, ss.key_idx, ss.sig, ss.blob, ss.off, ss.len), ss.n)
    assert np.array_equal(got, ss.expected), np.nonzero(got != ss.expected)[0]
