"""The ECDSA secp256k1 lane code (concord-bft_amd/csrc/ecdsa_verify.h with fe_secp256k1.h,
sc_secp256k1.h, ge_secp256k1.h: what the gfx950 kernels run per lane) built for the host
(tests/cpp/libecdsa_shim.so, the same source), against tests/ecdsa_ref.py and the OpenSSL-pinned
golden vectors; the generator's restatement against the fixture; and the same source once as a
stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import ecdsa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "cpp", "libecdsa_shim.so")
SAN = os.path.join(ROOT, "tests", "cpp", "ecdsa_shim_san")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ecdsa_vectors.json")
P, N = ref.P, ref.N
FULL = (1 << 256) - 1


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SHIM), "tests/cpp/libecdsa_shim.so not built (make ecdsa_shim)"
    return ctypes.CDLL(SHIM)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


def edge_operands(rng, mod):
    """Operands near 0, mod - 1 and 2^256 - 1 (reduced into [0, mod) by the caller where needed)."""
    edges = [0, 1, 2, 3, mod - 1, mod - 2, mod - 3, FULL, FULL - 1, FULL - mod, (1 << 255), (1 << 128) - 1, 1 << 32,
             977, mod >> 1]
    return edges + [rng.getrandbits(256) for _ in range(8)]


def test_fixture_matches_restatement(golden):
    """Every OpenSSL verdict of the fixture is what ecdsa_ref gives, and every class is present."""
    classes = set()
    for v in golden["vectors"]:
        key = bytes.fromhex(golden["keys"][v["key"]])
        assert ref.verify(key, bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) == bool(v["ok"]), v["cls"]
        classes.add(v["cls"])
    need = {"valid", "high_s_twin", "flip_r", "flip_s", "flip_msg", "flip_key_index", "r_zero", "s_zero", "r_eq_n",
            "s_eq_n", "r_above_n", "s_above_n", "r_plus_n", "s_plus_n", "key_off_curve", "key_zero", "key_x_eq_p",
            "key_y_eq_p", "rx_above_n", "rx_above_n_unreduced", "chosen_u1", "chosen_u2", "closing_doubling",
            "closing_infinity", "window_collision"}
    assert need <= classes, need - classes
    lens = {len(v["msg"]) // 2 for v in golden["vectors"] if v["cls"] == "valid"}
    assert {0, 1, 55, 56, 63, 64, 119, 120, 256, 4096} <= lens
    by = {}
    for v in golden["vectors"]:
        by.setdefault(v["cls"], set()).add(v["ok"])
    assert by["valid"] == {1} and by["high_s_twin"] == {1} and by["rx_above_n"] == {1}
    assert by["closing_doubling"] == {1} and by["window_collision"] == {1}
    assert by["closing_infinity"] == {0} and by["rx_above_n_unreduced"] == {0} and by["r_plus_n"] == {0}


def test_restatement_jacobian_law_matches_affine_law():
    rng = random.Random(0x1AC)
    for _ in range(12):
        k, pt = rng.randrange(N), ref.mul_affine(rng.randrange(1, N), ref.G)
        assert ref.mul(k, pt) == ref.mul_affine(k, pt)
    for k in (0, 1, 2, N - 1, N, N + 1):
        assert ref.mul(k, ref.G) == ref.mul_affine(k, ref.G)
    q = ref.mul(5, ref.G)
    assert ref.mul2(5, ref.G, N - 1, q) is ref.INF
    assert ref.mul2(5, ref.G, 1, q) == ref.mul_affine(10, ref.G)


def test_lane_code_on_fixture(lib, golden):
    bad = []
    for i, v in enumerate(golden["vectors"]):
        key, sig, msg = bytes.fromhex(golden["keys"][v["key"]]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])
        got = lib.ecdsa_shim_verify(key, sig, msg, ctypes.c_uint32(len(msg)))
        if got != v["ok"]:
            bad.append((i, v["cls"], got))
    assert not bad, bad[:10]


def test_field_operations(lib):
    """2,000 random and edge operations in GF(p) against Python integers."""
    rng = random.Random(0xFE256)
    out = (ctypes.c_uint8 * 32)()
    ops = {0: lambda a, b: (a + b) % P, 1: lambda a, b: (a - b) % P, 2: lambda a, b: a * b % P,
           3: lambda a, b: a * a % P, 4: lambda a, b: pow(a, -1, P) if a else 0, 5: lambda a, b: -a % P}
    pool = edge_operands(rng, P)
    done = 0
    while done < 2000:
        a, b = rng.choice(pool), rng.choice(pool)
        if rng.random() < 0.5:
            a, b = rng.getrandbits(256), rng.getrandbits(256)
        # op 6 takes unreduced operands (the 512-bit reduction on its own)
        assert lib.ecdsa_shim_fe_op(6, be(a), be(b), out) == 0
        assert int.from_bytes(bytes(out), "big") == a * b % P, (hex(a), hex(b))
        a, b = a % P, b % P
        op = rng.randrange(6)
        assert lib.ecdsa_shim_fe_op(op, be(a), be(b), out) == 0
        assert int.from_bytes(bytes(out), "big") == ops[op](a, b), (op, hex(a), hex(b))
        done += 2
    # an operand that is not below p is refused by the reduced-operand entries
    assert lib.ecdsa_shim_fe_op(0, be(P), be(1), out) == -1
    assert lib.ecdsa_shim_fe_op(0, be(1), be(FULL), out) == -1


def test_scalar_operations(lib):
    """2,000 random and edge operations mod n against Python integers."""
    rng = random.Random(0x5C256)
    out = (ctypes.c_uint8 * 32)()
    pool = edge_operands(rng, N)
    for i in range(1000):
        a, b = rng.choice(pool), rng.choice(pool)
        if i % 2:
            a, b = rng.getrandbits(256), rng.getrandbits(256)
        assert lib.ecdsa_shim_sc_op(0, be(a), be(b), out) == 0
        assert int.from_bytes(bytes(out), "big") == a * b % N, (hex(a), hex(b))
        assert lib.ecdsa_shim_sc_op(2, be(a), be(b), out) == 0
        assert int.from_bytes(bytes(out), "big") == a % N
        assert lib.ecdsa_shim_sc_op(3, be(a), be(b), out) == (1 if a < N else 0)
        a %= N
        assert lib.ecdsa_shim_sc_op(1, be(a), be(b), out) == 0
        assert int.from_bytes(bytes(out), "big") == (pow(a, -1, N) if a else 0), hex(a)
    assert lib.ecdsa_shim_sc_op(1, be(N), be(0), out) == -1


def _ge(lib, mode, a, za, b, zb):
    out = (ctypes.c_uint8 * 64)()
    rc = lib.ecdsa_shim_ge_op(mode, ref.pub_bytes(a) if a else bytes(64), 0 if a else 1, be(za),
                              ref.pub_bytes(b) if b else bytes(64), 0 if b else 1, be(zb), out)
    assert rc in (0, 1), rc
    if rc == 1:
        return ref.INF
    o = bytes(out)
    return (int.from_bytes(o[:32], "big"), int.from_bytes(o[32:], "big"))


def test_point_operations_with_equal_opposite_and_infinite_operands(lib):
    rng = random.Random(0x6E256)
    pts = [ref.mul(rng.randrange(1, N), ref.G) for _ in range(6)] + [ref.G, ref.mul(2, ref.G)]
    for a in pts:
        za, zb = rng.randrange(1, P), rng.randrange(1, P)
        assert _ge(lib, 2, a, za, None, 1) == ref.add(a, a)
        for b in [a, ref.neg(a), pts[0], pts[3], ref.add(a, a), None]:
            assert _ge(lib, 0, a, za, b, zb) == ref.add(a, b)      # full addition
            assert _ge(lib, 0, b, zb, a, za) == ref.add(a, b)
            if b is not None:
                assert _ge(lib, 1, a, za, b, 1) == ref.add(a, b)   # mixed addition
                assert _ge(lib, 1, None, 1, b, 1) == b              # infinity + b
    assert _ge(lib, 0, None, 1, None, 1) is ref.INF
    assert _ge(lib, 2, None, 1, None, 1) is ref.INF


def test_key_records(lib):
    """The window table of a usable key is [Q, 2 Q, ..., 15 Q] in affine form; unusable keys are marked."""
    rec = (ctypes.c_uint32 * 256)()
    q = ref.mul(0xC0FFEE, ref.G)
    assert lib.ecdsa_shim_key(ref.pub_bytes(q), rec) == 1
    for k in range(1, 16):
        words = rec[16 * (k - 1): 16 * k]
        x = sum(w << (32 * i) for i, w in enumerate(words[:8]))
        y = sum(w << (32 * i) for i, w in enumerate(words[8:]))
        assert (x, y) == ref.mul(k, q), k
    for bad in [bytes(64), be(q[0]) + be((q[1] + 1) % P), be(P) + be(q[1]), be(q[0]) + be(P), b"\xff" * 64]:
        assert lib.ecdsa_shim_key(bad, rec) == 0
        assert not any(rec)


def test_sha256_front_end(lib):
    rng = random.Random(0x5A256)
    out = (ctypes.c_uint8 * 32)()
    for length in list(range(0, 200)) + [255, 256, 257, 4095, 4096]:
        m = rng.randbytes(length)
        lib.ecdsa_shim_sha256(m, ctypes.c_uint32(length), out)
        assert bytes(out) == hashlib.sha256(m).digest(), length


def test_random_signatures_against_restatement(lib):
    rng = random.Random(0xEC0)
    for i in range(40):
        d = rng.randrange(1, N)
        q = ref.pub_bytes(ref.mul(d, ref.G))
        m = rng.randbytes(rng.randrange(0, 150))
        r, s = ref.sign(d, m, rng.randrange(1, N))
        cases = [(q, ref.sig_bytes(r, s), m), (q, ref.sig_bytes(r, N - s), m), (q, ref.sig_bytes(s, r), m),
                 (q, ref.sig_bytes(r, s), m + b"x")]
        for key, sig, msg in cases:
            assert lib.ecdsa_shim_verify(key, sig, msg, ctypes.c_uint32(len(msg))) == ref.verify(key, sig, msg)


def test_stand_alone_sanitizer_run():
    assert os.path.exists(SAN), "tests/cpp/ecdsa_shim_san not built (make ecdsa_shim)"
    p = subprocess.run([SAN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "as expected" in p.stdout
