"""The pair ladder (ed25519_comb2_ladder_kernel) with ONE entry stage per wave: every step reads its
entry out of the stage before the next entry is requested into the same stage, and with 22 KB of LDS
per group ladder waves of different batches share a SIMD.  All at small shapes, the pair ladder
forced with CBFT_OPT_LADDER_LANES = 2 and CBFT_OPT_SMALL_MAX = 0; verdicts are bit-exact against the
golden / OpenSSL ones."""
import ctypes

import numpy as np
import pytest

import cbft_hipcrypto as cb
from golden_io import load_ed25519_vectors
import workload as sigsets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_ed25519_vectors()


def _pair_ctx(**kw):
    return cb.Context(device=0, **kw).set_option(cb.OPT_LADDER_LANES, 2).set_option(cb.OPT_SMALL_MAX, 0)


class _Hip:
    """Device buffers and streams from the HIP runtime libcbft_hipcrypto itself links."""

    def __init__(self):
        cb.load_library()
        self.lib = ctypes.CDLL("libamdhip64.so.7")
        self.bufs, self.streams = [], []

    def _ok(self, rc, what):
        assert rc == 0, f"{what}: hipError {rc}"

    def to_dev(self, a: np.ndarray) -> int:
        p = ctypes.c_void_p()
        self._ok(self.lib.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(a.nbytes, 1))), "hipMalloc")
        self.bufs.append(p.value)
        a = np.ascontiguousarray(a)
        self._ok(self.lib.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1), "hipMemcpy")
        return p.value

    def words(self, ptr: int, nwords: int) -> np.ndarray:
        out = np.zeros(nwords, dtype=np.uint64)
        self._ok(self.lib.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr),
                                    ctypes.c_size_t(nwords * 8), 2), "hipMemcpy")
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


def _expected_words(expected: np.ndarray) -> np.ndarray:
    """ceil(n / 64) whole verdict words, bit i of word i / 64 = verdict i, bits past n zero."""
    n = expected.shape[0]
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = expected
    return np.packbits(bits, bitorder="little").view(np.uint64)


@pytest.mark.parametrize("radix,b_radix", [(8, 16), (9, 17), (13, 22), (15, 24)])
def test_single_stage_golden_geometries(golden, radix, b_radix):
    """The golden OpenSSL vectors through the pair ladder at 24 steps per lane (8 / 16: 32 + 16
    positions, the maximum), at odd position counts (9 / 17: 29 + 15 positions, one lane of a pair
    takes an identity step in each phase), at the default (13 / 22) and at the fewest steps (15 / 24:
    the stage is overwritten soonest).  Verdicts equal the recorded ones and the four-lane ladder's."""
    keys = sorted({v.pk for v in golden})
    index = {k: i for i, k in enumerate(keys)}
    args = ([index[v.pk] for v in golden], [v.sig for v in golden], [v.msg for v in golden])
    got = {}
    for lanes in (2, 4):
        with cb.Context(device=0) as c:
            c.set_option(cb.OPT_LADDER_LANES, lanes).set_option(cb.OPT_SMALL_MAX, 0).set_option(cb.OPT_B_RADIX, b_radix)
            tid = c.load_keys(keys, radix=radix)
            got[lanes] = cb.bitmap_to_bools(c.verify(tid, *args), len(golden))
    exp = np.array([bool(v.verdict) for v in golden])
    assert np.array_equal(got[2], exp), np.nonzero(got[2] != exp)[0][:10]
    assert np.array_equal(got[2], got[4]), np.nonzero(got[2] != got[4])[0][:10]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 4097])
def test_batch_size_edges_whole_words(n):
    """One wave holds 32 pairs: batches around one and two waves and one past 4,096 (the last
    work-group's tail pairs compute a copy of signature n - 1 and store nothing), about 5 % planted
    invalid signatures.  The verdict words, whole and with the bits past n zero, equal OpenSSL's."""
    L = 256
    ss = sigsets.make_sigset(n, nkeys=61, msg_len=L, seed=0x1AD0 + n, invalid_frac=0.05)
    nwords = (n + 63) // 64
    hip = _Hip()
    try:
        with _pair_ctx() as c:
            tid = c.load_keys(ss.pk)
            d_kidx, d_sig, d_blob = hip.to_dev(ss.key_idx), hip.to_dev(ss.sig.reshape(-1)), hip.to_dev(ss.blob)
            out = hip.to_dev(np.full(nwords + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
            c.verify_fixed_device(tid, 0, d_kidx, d_sig, d_blob, L, n, out, None)
            hip.sync()
            words = hip.words(out, nwords + 1)
            c.unload_keys(tid)
    finally:
        hip.close()
    assert np.array_equal(words[:nwords], _expected_words(ss.expected)), np.nonzero(
        words[:nwords] != _expected_words(ss.expected))[0][:8]
    assert words[nwords] == np.uint64(0xA5A5A5A5A5A5A5A5), "wrote past ceil(n / 64) words"


def test_co_resident_ladders_three_streams():
    """Three streams x six batches of 4,096 signatures, each batch with its own invalid schedule,
    launched back to back through verify_fixed_device: ladder waves of different batches share a
    SIMD, each with its own stage.  Every launch's words equal its own batch's OpenSSL verdicts."""
    n, L, nb, streams = 4096, 256, 6, 3
    nwords = n // 64
    sets = [sigsets.make_sigset(n, nkeys=128, msg_len=L, seed=0xC0DE + 17 * b, invalid_frac=0.03 + 0.01 * b)
            for b in range(nb)]
    for s in sets[1:]:
        assert np.array_equal(s.pk, sets[0].pk)
    assert len({s.expected.tobytes() for s in sets}) == nb and all((~s.expected).any() for s in sets)
    hip = _Hip()
    try:
        with _pair_ctx(max_batch=n) as c:
            tid = c.load_keys(sets[0].pk)
            dev = [(hip.to_dev(s.key_idx), hip.to_dev(s.sig.reshape(-1)), hip.to_dev(s.blob)) for s in sets]
            ss = [hip.stream() for _ in range(streams)]
            fill = np.full(nwords, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            runs = [((r + s) % nb, s) for r in range(nb) for s in range(streams)]  # every batch once per stream
            outs = [hip.to_dev(fill) for _ in runs]
            for (b, s), out in zip(runs, outs):
                c.verify_fixed_device(tid, 0, *dev[b], L, n, out, ss[s])
            hip.sync()
            got = [hip.words(out, nwords) for out in outs]
            c.unload_keys(tid)
    finally:
        hip.close()
    for (b, s), w in zip(runs, got):
        exp = _expected_words(sets[b].expected)
        assert np.array_equal(w, exp), f"batch {b} on stream {s}: words {np.nonzero(w != exp)[0][:8]} differ"
