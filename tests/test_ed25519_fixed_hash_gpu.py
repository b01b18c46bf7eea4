"""The fixed-length front end of the hash kernel (ed25519_hash_kernel<true>: one message length for
all, a multiple of 4, a 4-byte aligned blob) on the GPU: verdicts equal to OpenSSL's and to the
variable-length device call's on the same data, at the lengths where the 0x80 marker and the length
word change block or word, for batches that must not take it (odd lengths, a misaligned blob), and
on three streams.  The three-kernel path and the pair ladder are forced, as in the other tests."""
import ctypes

import numpy as np
import pytest

import cbft_hipcrypto as cb
import workload as sigsets

pytestmark = pytest.mark.gpu

NKEYS = 7
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)


class _Hip:
    """Device buffers and streams from the HIP runtime libcbft_hipcrypto itself links."""

    def __init__(self):
        cb.load_library()
        self.lib = ctypes.CDLL("libamdhip64.so.7")
        self.bufs, self.streams = [], []

    def _ok(self, rc, what):
        assert rc == 0, f"{what}: hipError {rc}"

    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self._ok(self.lib.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 1))), "hipMalloc")
        self.bufs.append(p.value)
        return p.value

    def put(self, ptr: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        self._ok(self.lib.hipMemcpy(ctypes.c_void_p(ptr), a.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_size_t(a.nbytes), 1), "hipMemcpy")

    def to_dev(self, a: np.ndarray) -> int:
        p = self.alloc(a.nbytes)
        self.put(p, a)
        return p

    def from_dev(self, ptr: int, nbytes: int) -> bytes:
        out = np.zeros(nbytes, dtype=np.uint8)
        self._ok(self.lib.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr),
                                    ctypes.c_size_t(nbytes), 2), "hipMemcpy")
        return out.tobytes()

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


@pytest.fixture(scope="module")
def gpu():
    """One context (three-kernel path, pair ladder) with the NKEYS keys every sigset here uses."""
    hip = _Hip()
    c = cb.Context(device=0)
    c.set_option(cb.OPT_SMALL_MAX, 0).set_option(cb.OPT_LADDER_LANES, 2)
    tid = c.load_keys(sigsets.make_sigset(1, nkeys=NKEYS, msg_len=4, seed=1).pk)
    try:
        yield hip, c, tid
    finally:
        hip.sync()
        c.unload_keys(tid)
        c.close()
        hip.close()


def _words(hip, out, n):
    """(verdict bits of the ceil(n/64) words, the word behind them) of a buffer of nwords + 1."""
    nwords = (n + 63) // 64
    words = np.frombuffer(hip.from_dev(out, (nwords + 1) * 8), dtype=np.uint64)
    return np.unpackbits(words[:nwords].view(np.uint8), bitorder="little").astype(bool), words[nwords]


def _check(bits, guard, ss, what):
    bad = np.nonzero(bits[:ss.n] != ss.expected)[0]
    assert bad.size == 0, f"{what}: {bad.size} mismatches, first {bad[:8]}"
    assert not bits[ss.n:].any(), f"{what}: stale bits past n in the last verdict word"
    assert guard == FILL, f"{what}: wrote past ceil(n/64) words"


def _both_calls(gpu, ss, L, msg_ptr=None):
    """The fixed-length and the variable-length device call on the same device data."""
    hip, c, tid = gpu
    n = ss.n
    nwords = (n + 63) // 64
    d_kidx, d_sig = hip.to_dev(ss.key_idx), hip.to_dev(ss.sig.reshape(-1))
    d_blob = hip.to_dev(ss.blob) if msg_ptr is None else msg_ptr
    d_off, d_len = hip.to_dev(ss.off), hip.to_dev(ss.len)
    assert ss.expected.any() and not ss.expected.all()
    out_f = hip.to_dev(np.full(nwords + 1, FILL, dtype=np.uint64))
    out_v = hip.to_dev(np.full(nwords + 1, FILL, dtype=np.uint64))
    c.verify_fixed_device(tid, 0, d_kidx, d_sig, d_blob, L, n, out_f, None)
    c.verify_device(tid, 0, d_kidx, d_sig, d_blob, d_off, d_len, n, out_v, None)
    hip.sync()
    fixed, guard_f = _words(hip, out_f, n)
    var, guard_v = _words(hip, out_v, n)
    _check(fixed, guard_f, ss, f"fixed call, L={L}, n={n}")
    _check(var, guard_v, ss, f"variable-length call, L={L}, n={n}")
    assert np.array_equal(fixed, var)


# 0: empty; 4: smallest; 44: marker mid-word, length word in the same block; 48: 64 + L = 112, the
# length word moves to a second block; 60 / 64 / 68 around the first block's end; 172 / 176 and
# 188 / 192 the same edges one block later; 256 the headline; 300 four blocks
ELIGIBLE = [0, 4, 44, 48, 60, 64, 68, 172, 176, 188, 192, 256, 300]


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("L", ELIGIBLE)
def test_fixed_front_end_lengths(gpu, L, n):
    ss = sigsets.make_sigset(n, nkeys=NKEYS, msg_len=L, seed=5000 + 7 * L + n, invalid_frac=0.2, threads=4)
    assert np.array_equal(ss.off, np.arange(n, dtype=ss.off.dtype) * L)
    _both_calls(gpu, ss, L)


@pytest.mark.parametrize("L", [1, 47, 255])
def test_odd_lengths_take_the_general_path(gpu, L):
    ss = sigsets.make_sigset(130, nkeys=NKEYS, msg_len=L, seed=6000 + L, invalid_frac=0.2, threads=4)
    _both_calls(gpu, ss, L)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_blob_takes_the_general_path(gpu, shift):
    """L = 256 is eligible, the message base is not: the blob starts `shift` bytes into a larger
    device buffer."""
    hip = gpu[0]
    L, n = 256, 130
    ss = sigsets.make_sigset(n, nkeys=NKEYS, msg_len=L, seed=6100 + shift, invalid_frac=0.2, threads=4)
    big = hip.alloc(ss.blob.nbytes + 8)
    assert big % 4 == 0
    hip.put(big + shift, ss.blob)
    _both_calls(gpu, ss, L, msg_ptr=big + shift)


def test_fixed_front_end_three_streams(gpu):
    """Four distinct batches of 1,100 at L = 256, cycled twice over three streams; every call has a
    verdict buffer of its own and every call's words are checked."""
    hip, c, tid = gpu
    n, L, nb, calls = 1100, 256, 4, 8
    nwords = (n + 63) // 64
    sets = [sigsets.make_sigset(n, nkeys=NKEYS, msg_len=L, seed=6200 + b, invalid_frac=0.2, threads=4)
            for b in range(nb)]
    assert len({s.expected.tobytes() for s in sets}) == nb
    dev = [(hip.to_dev(s.key_idx), hip.to_dev(s.sig.reshape(-1)), hip.to_dev(s.blob)) for s in sets]
    streams = [hip.stream() for _ in range(3)]
    outs = [hip.to_dev(np.full(nwords + 1, FILL, dtype=np.uint64)) for _ in range(calls)]
    for j in range(calls):
        d_kidx, d_sig, d_blob = dev[j % nb]
        c.verify_fixed_device(tid, 0, d_kidx, d_sig, d_blob, L, n, outs[j], streams[j % 3])
    hip.sync()
    for j in range(calls):
        bits, guard = _words(hip, outs[j], n)
        _check(bits, guard, sets[j % nb], f"call {j} (batch {j % nb})")
