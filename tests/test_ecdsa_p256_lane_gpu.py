"""GPU tests of the ECDSA P-256 lane code, one function per launch (tests/hip/ecdsa_p256_selftest.hip): fe_mul,
fe_sqr, fe_add, fe_sub, the 512-bit reduction with the exact compares, sc_mul, the two inversions, ge_dbl and
ge_madd on a few hundred seeded operand sets that include the edge list, every output word against Python
integers.  This sees what the verdict bit of a whole verification hides: a device-only miscompile or a lost
carry."""
import ctypes
import os
import random

import numpy as np
import pytest

import p256_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P, N = ref.P, ref.N
FULL = (1 << 256) - 1
EPS_OUT = 24
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def selftest():
    path = os.path.join(HERE, "hip", "libecdsa_p256_selftest.so")
    assert os.path.exists(path), "tests/hip/libecdsa_p256_selftest.so not built (make selftest)"
    lib = ctypes.CDLL(path)

    def run(op, *cols):
        """cols: up to five operand lists.  Rows of (first result, second result, flag) as integers."""
        n = len(cols[0])
        cols = list(cols) + [[0] * n] * (5 - len(cols))
        assert all(len(c) == n for c in cols)
        blob = b"".join(int(t).to_bytes(32, "little") for c in cols for t in c)
        win = np.frombuffer(blob, dtype=np.uint32).copy()
        out = np.full(n * EPS_OUT, SENTINEL, dtype=np.uint32)
        rc = lib.ecdsa_p256_selftest(op, win.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), n)
        assert rc == 0, f"hipError {rc}"
        out = out.reshape(n, EPS_OUT)
        assert not (out == SENTINEL).all(axis=1).any(), "a lane left its output unwritten"
        assert not out[:, 17:].any()
        val = lambda row: int.from_bytes(row.tobytes(), "little")  # noqa: E731
        return [(val(r[:8]), val(r[8:16]), int(r[16])) for r in out]

    return run


def edge_values(mod):
    e = [0, 1, 2, mod - 1, mod - 2, mod, mod + 1, FULL, FULL - 1, 1 << 224, (1 << 224) - 1, (1 << 224) + 1, 1 << 192,
         (1 << 192) - 1, (1 << 192) + 1, 1 << 96, (1 << 96) - 1, (1 << 96) + 1, P - 1, N - 1]
    for i in range(8):
        e += [0xFFFFFFFF << (32 * i), FULL & ~(0xFFFFFFFF << (32 * i))]
    return e


def operand_pairs(seed, mod, reduce):
    """Every edge value against every edge value's neighbourhood (a sample), then random pairs: ~400 sets."""
    rng = random.Random(seed)
    e = edge_values(mod)
    pairs = [(a, b) for a in e for b in rng.sample(e, 6)]
    for i in range(8):
        pairs.append((rng.randrange(1 << 256) | (0xFFFFFFFF << (32 * i)), rng.randrange(1 << 256)))
    pairs += [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(150)]
    if reduce:
        pairs = [(a % mod, b % mod) for a, b in pairs]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("op,fn", [(0, lambda a, b: a * b % P), (1, lambda a, b: a * a % P),
                                   (2, lambda a, b: (a + b) % P), (3, lambda a, b: (a - b) % P)],
                         ids=["fe_mul", "fe_sqr", "fe_add", "fe_sub"])
def test_field_ops_on_the_gpu(selftest, op, fn):
    a, b = operand_pairs(0x100 + op, P, True)
    assert len(a) >= 300
    got = selftest(op, a, b)
    bad = [(hex(x), hex(y)) for x, y, g in zip(a, b, got) if g[0] != fn(x, y) or g[1] or g[2]]
    assert not bad, bad[:4]


def test_reduction_of_any_product_and_exact_compares_on_the_gpu(selftest):
    a, b = operand_pairs(0x204, P, False)
    a += [5, 0, P, P - 1, P + 1]
    b += [5, 0, 0, P - 1, 1]
    got = selftest(4, a, b)
    for x, y, g in zip(a, b, got):
        assert g[0] == x * y % P, (hex(x), hex(y))
        assert g[2] == (1 if x == y else 0) | (2 if x == 0 else 0) | (4 if x < P else 0), (hex(x), hex(y))


def test_scalar_product_and_range_on_the_gpu(selftest):
    a, b = operand_pairs(0x305, N, False)
    got = selftest(5, a, b)
    for x, y, g in zip(a, b, got):
        assert g == (x * y % N, x % N, 1 if x < N else 0), (hex(x), hex(y))


@pytest.mark.parametrize("op,mod", [(6, P), (7, N)], ids=["fe_inv", "sc_inv"])
def test_inversions_on_the_gpu(selftest, op, mod):
    a, _ = operand_pairs(0x400 + op, mod, True)
    a = sorted(set(a))
    assert len(a) >= 150 and 0 in a and 1 in a and mod - 1 in a
    got = selftest(op, a)
    for x, g in zip(a, got):
        assert g[0] == (pow(x, -1, mod) if x else 0), hex(x)


@pytest.fixture(scope="module")
def points():
    rng = random.Random(0x9E)
    pts = [ref.G, ref.neg(ref.G), ref.lift_x(0), ref.lift_x(0, True)]
    x = ref.N + 2  # x(R) >= n
    while ref.lift_x(x) is None:
        x += 1
    pts.append(ref.lift_x(x))
    for i in range(8):  # x with a word of all ones
        while True:
            x = (rng.randrange(1 << 256) | (0xFFFFFFFF << (32 * i))) % P
            if i == 7:
                x = (0xFFFFFFFF << 224) | rng.randrange(1 << 192)
            if ref.lift_x(x) is not None:
                break
        pts.append(ref.lift_x(x, bool(i & 1)))
    k = rng.randrange(1, N)
    q = ref.mul(k, ref.G)
    for _ in range(40):
        pts.append(q)
        q = ref.add(q, ref.G)
    return pts


def _unpack(g):
    return None if g[2] else (g[0], g[1])


def test_ge_dbl_on_the_gpu(selftest, points):
    rng = random.Random(0x8D)
    zs = [1, P - 1, 2] + [rng.randrange(1, P) for _ in range(len(points) - 3)]
    xs, ys = [p[0] for p in points] + [1], [p[1] for p in points] + [1]
    got = selftest(8, xs, ys, zs + [0])  # the last one is infinity
    for p, g in zip(points + [None], got):
        assert _unpack(g) == ref.add(p, p), p


def test_ge_madd_on_the_gpu(selftest, points):
    rng = random.Random(0x9A)
    cases = []
    for i, p in enumerate(points):
        cases += [(p, p), (p, ref.neg(p)), (None, p), (p, points[(i + 7) % len(points)])]
    xs = [a[0] if a else 1 for a, _ in cases]
    ys = [a[1] if a else 1 for a, _ in cases]
    zs = [rng.randrange(1, P) if a else 0 for a, _ in cases]
    got = selftest(9, xs, ys, zs, [b[0] for _, b in cases], [b[1] for _, b in cases])
    assert len(cases) >= 200
    for (a, b), g in zip(cases, got):
        assert _unpack(g) == ref.add(a, b), (a, b)
