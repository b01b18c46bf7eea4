"""CPU tests of the ECDSA P-256 lane code (concord-bft_amd/csrc/ecdsa_p256_verify.h and the field, scalar
and point headers under it), built for the host as tests/cpp/libecdsa_p256_shim.so: the same source that
runs on gfx950, against Python integers (tests/p256_ref.py) and OpenSSL's verdicts
(tests/golden/ecdsa_p256_vectors.json)."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import p256_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
P, N = ref.P, ref.N
FULL = (1 << 256) - 1


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(HERE, "cpp", "libecdsa_p256_shim.so"))
    lib.ecdsa_p256_shim_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "ecdsa_p256_vectors.json")))


def be(v):
    return v.to_bytes(32, "big")


def edge_operands(rng, mod, count):
    """Operands near 0, 1, mod - 1, 2^256 - 1, 2^224, 2^192, 2^96, with a word of all ones at every limb
    position, then random ones."""
    near = [0, 1, 2, mod - 1, mod - 2, mod, mod + 1, FULL, FULL - 1, 1 << 224, (1 << 224) - 1, (1 << 224) + 1,
            1 << 192, (1 << 192) - 1, (1 << 192) + 1, 1 << 96, (1 << 96) - 1, (1 << 96) + 1, P - 1, N - 1]
    for i in range(8):
        near.append(0xFFFFFFFF << (32 * i))
        near.append(rng.randrange(1 << 256) | (0xFFFFFFFF << (32 * i)))
        near.append(FULL & ~(0xFFFFFFFF << (32 * i)))
    while len(near) < count:
        near.append(rng.randrange(1 << 256))
    return near


def test_field_ops_vs_python_integers(shim):
    rng = random.Random(0xF256)
    ops = edge_operands(rng, P, 64)
    out = ctypes.create_string_buffer(32)
    n = 0
    pairs = [(a, b) for a in ops[:45] for b in ops[:45]][:1600] + [(rng.choice(ops), rng.randrange(1 << 256))
                                                                  for _ in range(400)]
    for a, b in pairs:
        # the 512-bit reduction on ANY 256-bit operands
        assert shim.ecdsa_p256_shim_fe_op(6, be(a), be(b), out) == 0
        assert int.from_bytes(out.raw, "big") == a * b % P, (hex(a), hex(b))
        n += 1
        x, y = a % P, b % P
        for op, want in ((0, (x + y) % P), (1, (x - y) % P), (2, x * y % P), (3, x * x % P), (5, -x % P)):
            assert shim.ecdsa_p256_shim_fe_op(op, be(x), be(y), out) == 0
            assert int.from_bytes(out.raw, "big") == want, (op, hex(x), hex(y))
        assert shim.ecdsa_p256_shim_fe_op(7, be(x), be(y), out) == (1 if x == y else 0)
        assert shim.ecdsa_p256_shim_fe_op(8, be(x), be(y), out) == (1 if x == 0 else 0)
    assert n >= 2000
    for a in ops:
        x = a % P
        assert shim.ecdsa_p256_shim_fe_op(4, be(x), be(0), out) == 0
        assert int.from_bytes(out.raw, "big") == (pow(x, -1, P) if x else 0)
    assert shim.ecdsa_p256_shim_fe_op(0, be(P), be(0), out) == -1  # not below p


def test_scalar_ops_vs_python_integers(shim):
    rng = random.Random(0x5C256)
    ops = edge_operands(rng, N, 64)
    out = ctypes.create_string_buffer(32)
    pairs = [(a, b) for a in ops[:45] for b in ops[:45]][:1600] + [(rng.choice(ops), rng.randrange(1 << 256))
                                                                  for _ in range(400)]
    assert len(pairs) >= 2000
    rinv = pow(1 << 256, -1, N)
    for a, b in pairs:
        assert shim.ecdsa_p256_shim_sc_op(0, be(a), be(b), out) == 0
        assert int.from_bytes(out.raw, "big") == a * b % N, (hex(a), hex(b))
        assert shim.ecdsa_p256_shim_sc_op(4, be(a), be(b % N), out) == 0
        assert int.from_bytes(out.raw, "big") == a * (b % N) * rinv % N
        assert shim.ecdsa_p256_shim_sc_op(2, be(a), be(0), out) == 0
        assert int.from_bytes(out.raw, "big") == a % N
        assert shim.ecdsa_p256_shim_sc_op(3, be(a), be(0), out) == (1 if a < N else 0)
    for a in ops:
        x = a % N
        assert shim.ecdsa_p256_shim_sc_op(1, be(x), be(0), out) == 0
        assert int.from_bytes(out.raw, "big") == (pow(x, -1, N) if x else 0)


def test_accept_under_the_keys_with_x_zero_for_a_chosen_digest(shim):
    """(0, +-sqrt(b)) is on P-256.  An accepted signature over a SHA-256 output needs the key's discrete logarithm,
    so e is chosen here: R = a G + b Q, r = x(R) mod n, s = r / b, e = a s.  The lane code from the digest accepts
    it and its high-s twin as the restatement does, and rejects its neighbours."""
    rng = random.Random(0xE0)
    shim.ecdsa_p256_shim_verify_digest.argtypes = [ctypes.c_char_p] * 3
    for odd in (False, True):
        q = ref.lift_x(0, odd)
        for _ in range(4):
            a, b = rng.randrange(1, N), rng.randrange(1, N)
            R = ref.mul2(a, ref.G, b, q)
            r = R[0] % N
            s = r * pow(b, -1, N) % N
            e = a * s % N
            assert r and s and ref.verify_ints(q, r, s, e)
            pub, sig = ref.pub_bytes(q), ref.sig_bytes(r, s)
            assert shim.ecdsa_p256_shim_verify_digest(pub, sig, be(e)) == 1
            assert shim.ecdsa_p256_shim_verify_digest(pub, ref.sig_bytes(r, N - s), be(e)) == 1  # the high-s twin
            assert shim.ecdsa_p256_shim_verify_digest(pub, ref.sig_bytes(r, s + 1), be(e)) == 0
            assert shim.ecdsa_p256_shim_verify_digest(pub, sig, be(e ^ 1)) == (1 if ref.verify_ints(q, r, s, e ^ 1) else 0)
            assert shim.ecdsa_p256_shim_verify_digest(ref.pub_bytes(ref.neg(q)), sig, be(e)) == (
                1 if ref.verify_ints(ref.neg(q), r, s, e) else 0)


def test_rejected_montgomery_reduction_sketch(shim):
    """tools/isa/p256_mont_sketch.h, whose instruction count DESIGN.md section 27.2 quotes, computes what it says."""
    rng = random.Random(0x3056)
    ops = edge_operands(rng, P, 64)
    out = ctypes.create_string_buffer(32)
    rinv = pow(1 << 256, -1, P)
    for a, b in [(a, b) for a in ops[:45] for b in ops[:45]] + [(rng.randrange(1 << 256), rng.randrange(1 << 256))
                                                                for _ in range(500)]:
        assert shim.ecdsa_p256_shim_fe_op(9, be(a), be(b), out) == 0
        assert int.from_bytes(out.raw, "big") == a * b * rinv % P, (hex(a), hex(b))


def test_point_formulas_on_equal_opposite_and_infinite_operands(shim):
    rng = random.Random(0x6E256)
    out = ctypes.create_string_buffer(64)
    pts = [ref.mul(rng.randrange(1, N), ref.G) for _ in range(6)] + [ref.G, ref.lift_x(0), ref.lift_x(0, True)]

    def run(mode, a, b):
        za, zb = be(rng.randrange(1, P)), be(rng.randrange(1, P))
        ab = ref.pub_bytes(a) if a else bytes(64)
        bb = ref.pub_bytes(b) if b else bytes(64)
        rc = shim.ecdsa_p256_shim_ge_op(mode, ab, a is None, za, bb, b is None, zb, out)
        assert rc in (0, 1)
        return None if rc else (int.from_bytes(out.raw[:32], "big"), int.from_bytes(out.raw[32:], "big"))

    for a in pts + [None]:
        assert run(2, a, None) == ref.add(a, a)  # doubling, infinity included
        for b in pts + [a, ref.neg(a), None]:
            assert run(0, a, b) == ref.add(a, b), (a, b)
            if b is not None:
                assert run(1, a, b) == ref.add(a, b), (a, b)


def test_key_records(shim, golden):
    rec = (ctypes.c_uint32 * 256)()
    usable = [ref.pub_bytes(ref.G), ref.pub_bytes(ref.lift_x(0)), ref.pub_bytes(ref.lift_x(0, True)),
              ref.pub_bytes(ref.mul(0xC0FFEE, ref.G))]
    for kb in usable:
        assert shim.ecdsa_p256_shim_key(kb, rec) == 1
        q = (int.from_bytes(kb[:32], "big"), int.from_bytes(kb[32:], "big"))
        for k in range(1, 16):
            m = ref.mul(k, q)
            x = sum(rec[(k - 1) * 16 + i] << (32 * i) for i in range(8))
            y = sum(rec[(k - 1) * 16 + 8 + i] << (32 * i) for i in range(8))
            assert (x, y) == m, k
        assert list(rec[240:]) == [1] + [0] * 15
    keys = [bytes.fromhex(k) for k in golden["keys"]]
    refused = {v["key"] for v in golden["vectors"] if v["cls"].startswith("key_") and v["cls"] != "key_x_zero"}
    assert len(refused) >= 7
    for i, kb in enumerate(keys):
        ok = shim.ecdsa_p256_shim_key(kb, rec)
        assert ok == (0 if i in refused else 1), i
        if i in refused:
            assert not any(rec)


def test_golden_vectors(shim, golden):
    keys = [bytes.fromhex(k) for k in golden["keys"]]
    by_class = {}
    for i, v in enumerate(golden["vectors"]):
        msg = bytes.fromhex(v["msg"])
        got = shim.ecdsa_p256_shim_verify(keys[v["key"]], bytes.fromhex(v["sig"]), msg, len(msg))
        if got != v["ok"]:
            by_class.setdefault(v["cls"], []).append(i)
    assert not by_class, by_class
    classes = {v["cls"] for v in golden["vectors"]}
    assert {"rx_above_n", "rx_above_n_unreduced", "field_edge", "key_x_zero", "rfc6979_a25", "closing_doubling",
            "closing_infinity", "window_collision", "key_x_plus_p"} <= classes


def test_sanitizer_program():
    """The same source as a stand-alone program under ASan + UBSan (never loaded into python)."""
    r = subprocess.run([os.path.join(HERE, "cpp", "ecdsa_p256_shim_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
