"""The pair ladder (ed25519_comb2_ladder_kernel) on the fold32 multiply and the uncarried
subtractions: bit-exact verdicts on the golden vectors at the key / B comb geometries that change
which table, digit sign and zero digit a lane's first point set and its additions see, and on one
batch of one full 64-signature block plus a tail pair with every kind of invalid signature planted."""
import numpy as np
import pytest

import cbft_hipcrypto as cb
from golden_io import load_ed25519_vectors
import workload as sigsets

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def golden():
    vs = load_ed25519_vectors()
    keys = sorted({v.pk for v in vs})
    index = {k: i for i, k in enumerate(keys)}
    return (keys, [index[v.pk] for v in vs], [v.sig for v in vs], [v.msg for v in vs],
            np.array([bool(v.verdict) for v in vs]))


@pytest.mark.parametrize("b_radix", [16, 22])
@pytest.mark.parametrize("radix", [8, 13, 15])
def test_fold_pair_ladder_golden(golden, radix, b_radix):
    keys, kidx, sigs, msgs, exp = golden
    with cb.Context(device=0) as c:
        c.set_option(cb.OPT_LADDER_LANES, 2).set_option(cb.OPT_B_RADIX, b_radix)
        tid = c.load_keys(keys, radix=radix)
        got = cb.bitmap_to_bools(c.verify(tid, kidx, sigs, msgs), len(exp))
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]


def test_fold_pair_ladder_block_plus_tail():
    """65 signatures = 130 lanes: one full 128-lane block and a second block holding one live pair
    (the rest compute copies of it).  Invalid signatures of every kind, the tail one included."""
    n, nkeys = 65, 8
    ss = sigsets.make_sigset(n, nkeys=nkeys, msg_len=256, seed=65, threads=4, compute_expected=False)
    ss.sig[3, 5] ^= 0x10                                   # a bit of R
    ss.sig[17, 40] ^= 0x02                                 # a bit of S
    s = int.from_bytes(ss.sig[29, 32:].tobytes(), "little") + L
    ss.sig[29, 32:] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)  # S + L
    ss.blob[int(ss.off[42]) + 100] ^= 0x5A                 # a message byte
    ss.key_idx[63] = (ss.key_idx[63] + 1) % nkeys          # the wrong key, last pair of the full block
    ss.sig[64, 33] ^= 0x80                                 # the tail pair: a bit of S
    ss.expected = sigsets.cpu_verify(ss, threads=4).astype(bool)
    assert not ss.expected[[3, 17, 29, 42, 63, 64]].any() and ss.expected.sum() == n - 6
    with cb.Context(device=0) as c:
        c.set_option(cb.OPT_LADDER_LANES, 2)
        tid = c.load_keys(ss.pk)
        got = cb.bitmap_to_bools(c.verify_packed(tid, ss.key_idx, ss.sig, ss.blob, ss.off, ss.len), n)
    assert np.array_equal(got, ss.expected), np.nonzero(got != ss.expected)[0]
