"""The ECDSA P-256 signing lane code (concord-bft_amd/csrc/ecdsa_p256_sign.h: what the gfx950 kernels
run per lane) and the DER writer (csrc/ecdsa_der.h) built for the host
(tests/cpp/libecdsa_p256_sign_shim.so, the same source), byte for byte against tests/p256_sign_ref.py,
Python integers and the golden vectors; and the same source once as a stand-alone program under
AddressSanitizer + UBSan."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import p256_ref as ref
import p256_sign_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "cpp", "libecdsa_p256_sign_shim.so")
SAN = os.path.join(ROOT, "tests", "cpp", "ecdsa_p256_sign_shim_san")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ecdsa_p256_sign_vectors.json")
K1_GOLDEN = os.path.join(ROOT, "tests", "golden", "ecdsa_sign_vectors.json")
P, N, B = ref.P, ref.N, ref.B
FULL = (1 << 256) - 1
EIGHTS = int("8" * 64, 16)


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


def word_patterns(mod: int):
    """Values below mod with an all-ones or an all-zeros 32-bit word at each position."""
    base = 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    out = []
    for pos in range(8):
        m = 0xFFFFFFFF << (32 * pos)
        out += [(base | m) % mod, (base & ~m) % mod, m % mod, (FULL & ~m) % mod]
    return out


def operands(mod: int, rng, count: int):
    ops = [0, 1, 2, mod - 1, mod - 2, FULL % mod, (1 << 255) % mod, (1 << 128) - 1, 1 << 32, mod >> 1] + word_patterns(mod)
    ops += [(v + d) % mod for v in (0, mod - 1, FULL) for d in range(-8, 9)]
    return ops + [rng.randrange(mod) for _ in range(count)]


def edge_nonces():
    """The scalars that drive the comb's recoding to its corners (k + 0x88..8 = nibbles + 2^256 carry), unreduced."""
    ks = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255]
    for j in range(64):
        ks += [16**j, 16**j - 1, 8 * 16**j]
    ks.append((0 - EIGHTS) % (1 << 256))  # every digit -8 (k + 0x88..8 = 2^256: the carry alone)
    ks.append(int("F" * 64, 16) - EIGHTS)  # every digit 7
    ks.append(N - EIGHTS)
    for j in (0, 1, 31, 62, 63):  # all digits 0 but one: +7, and -8 under the 2^256 carry
        ks += [7 * 16**j, (1 << 256) - 8 * 16**j]
    return ks


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SHIM), "tests/cpp/libecdsa_p256_sign_shim.so not built (make ecdsa_p256_sign_shim)"
    so = ctypes.CDLL(SHIM)
    so.ecdsa_p256_sign_shim_nonce_skip.restype = ctypes.c_uint32
    return so


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["vectors"]


def test_fixture_is_the_restatement_and_covers_the_edges(golden):
    assert os.path.getsize(GOLDEN) <= os.path.getsize(K1_GOLDEN)
    assert 150 <= len(golden) <= 250
    lens = {len(v["msg"]) // 2 for v in golden}
    assert {0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 256, 4096} <= lens
    xs = {int(v["x"], 16) for v in golden}
    assert {1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255, 16**63, 16**63 - 1, EIGHTS % N} <= xs
    for v in golden[::9] + golden[-2:]:
        k, r, s = sref.sign_digest(int(v["x"], 16), hashlib.sha256(bytes.fromhex(v["msg"])).digest())
        assert (f"{k:064x}", ref.sig_bytes(r, s).hex()) == (v["k"], v["sig"])
        assert ref.verify(sref.public_key(int(v["x"], 16)), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]))
    # RFC 6979 A.2.5, SHA-256: "sample" and "test"
    rfc = {bytes.fromhex(v["msg"]): v for v in golden[-2:]}
    assert rfc[b"sample"]["sig"].upper() == ("EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"
                                             "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8")
    assert rfc[b"test"]["sig"].upper() == ("F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367"
                                           "019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083")


def test_lane_code_on_fixture(lib, golden):
    out = (ctypes.c_uint8 * 64)()
    kout = (ctypes.c_uint8 * 32)()
    for i, v in enumerate(golden):
        msg = bytes.fromhex(v["msg"])
        assert lib.ecdsa_p256_sign_shim_sign(bytes.fromhex(v["x"]), msg, ctypes.c_uint32(len(msg)), out) == 1
        assert bytes(out).hex() == v["sig"], i
        assert lib.ecdsa_p256_sign_shim_nonce_skip(bytes.fromhex(v["x"]), hashlib.sha256(msg).digest(), ctypes.c_uint32(0),
                                                   kout) == 0
        assert bytes(kout).hex() == v["k"], i


def test_chosen_digests(lib):
    """Digests no message reaches: e >= n exercises bits2octets and the reduction of e."""
    rng = random.Random(0xD16E58)
    out = (ctypes.c_uint8 * 64)()
    for h in [0, 1, N - 1, N, N + 1, FULL, FULL - 1, (1 << 255), N + (1 << 100)] + [N + rng.randrange(FULL - N) for _ in range(4)]:
        for x in (1, N - 1, rng.randrange(1, N)):
            _, r, s = sref.sign_digest(x, be(h))
            assert lib.ecdsa_p256_sign_shim_sign_digest(be(x), be(h), out) == 1
            assert bytes(out) == ref.sig_bytes(r, s), (hex(h), hex(x))


def test_b_times_a(lib):
    rng = random.Random(0xB)
    out = (ctypes.c_uint8 * 32)()
    for a in operands(P, rng, 300):
        lib.ecdsa_p256_sign_shim_mulb(be(a), out)
        assert int.from_bytes(bytes(out), "big") == B * a % P, hex(a)


def test_constant_time_inversions(lib):
    rng = random.Random(0x1A8)
    out = (ctypes.c_uint8 * 32)()
    for which, mod in ((0, P), (1, N)):
        for a in operands(mod, rng, 400):
            lib.ecdsa_p256_sign_shim_inv(which, be(a), out)
            assert int.from_bytes(bytes(out), "big") == (pow(a, -1, mod) if a else 0), (which, hex(a))


def madd(lib, p3, q):
    out = (ctypes.c_uint8 * 96)()
    lib.ecdsa_p256_sign_shim_madd(b"".join(be(v) for v in p3), be(q[0]) + be(q[1]), out)
    o = bytes(out)
    return tuple(int.from_bytes(o[32 * i:32 * i + 32], "big") for i in range(3))


def proj_to_aff(t):
    if t[2] == 0:
        return ref.INF
    zi = pow(t[2], -1, P)
    return (t[0] * zi % P, t[1] * zi % P)


def test_complete_addition(lib):
    rng = random.Random(0xADD)
    pts = [ref.mul(rng.randrange(1, N), ref.G) for _ in range(40)] + [ref.G, ref.mul(N - 1, ref.G)]
    for i, q in enumerate(pts):
        # P = infinity (0 : 1 : 0), and with another Y
        assert proj_to_aff(madd(lib, (0, 1, 0), q)) == q
        assert proj_to_aff(madd(lib, (0, rng.randrange(1, P), 0), q)) == q
        for z in (1, P - 1, rng.randrange(1, P)):
            # P = Q
            assert proj_to_aff(madd(lib, (q[0] * z % P, q[1] * z % P, z), q)) == ref.add(q, q)
            # P = -Q: infinity, Z3 = 0 and Y3 != 0
            got = madd(lib, (q[0] * z % P, (P - q[1]) * z % P, z), q)
            assert got[2] == 0 and got[0] == 0 and got[1] != 0
            # random P with random Z
            p = pts[(i + 7) % len(pts)]
            assert proj_to_aff(madd(lib, (p[0] * z % P, p[1] * z % P, z), q)) == ref.add(p, q)


def test_comb_on_any_256_bit_scalar(lib):
    """k G for scalars up to 2^256 - 1 (the carry position), 0 and n (infinity)."""
    out = (ctypes.c_uint8 * 64)()
    for k in edge_nonces() + [FULL, FULL - 1, N + 1, (1 << 256) - EIGHTS - 1]:
        if k % N == 0:
            continue
        assert lib.ecdsa_p256_sign_shim_comb(be(k), out) == 0
        assert bytes(out) == ref.pub_bytes(ref.mul(k % N, ref.G)), hex(k)
    for k in (0, N):
        assert lib.ecdsa_p256_sign_shim_comb(be(k), out) == 1
        assert bytes(out) == bytes(64)


def test_comb_table_entries(lib):
    nwords = lib.ecdsa_p256_sign_shim_table_words()
    assert nwords == 64 * 8 * 16 + 16 and nwords * 4 == 32832
    tbl = (ctypes.c_uint32 * nwords)()
    lib.ecdsa_p256_sign_shim_table(tbl)

    def entry(w):
        return (sum(tbl[w + i] << (32 * i) for i in range(8)), sum(tbl[w + 8 + i] << (32 * i) for i in range(8)))

    base = ref.G
    for j in range(64):
        acc = base
        for e in range(1, 9):
            assert entry((j * 8 + e - 1) * 16) == acc, (j, e)
            acc = ref.add(acc, base)
        for _ in range(4):
            base = ref.add(base, base)
    assert entry(64 * 8 * 16) == base == ref.mul((1 << 256) % N, ref.G)


def test_x_mod_n(lib):
    out = (ctypes.c_uint8 * 32)()
    for x in (0, N - 1, N, N + 1, P - 1, 1, (N + P) // 2):
        lib.ecdsa_p256_sign_shim_x_mod_n(be(x), out)
        assert int.from_bytes(bytes(out), "big") == x % N, hex(x)


def test_sign_with_chosen_nonces(lib):
    rng = random.Random(0xC0FFEF)
    out = (ctypes.c_uint8 * 64)()
    for i, k in enumerate(k % N for k in edge_nonces() if k % N):
        x, e = (rng.randrange(1, N), rng.randrange(N)) if i % 3 else (N - 1, N - 1)
        want = sref.sign_with_k(x, e, k)
        got = lib.ecdsa_p256_sign_shim_sign_with_k(be(x), be(e), be(k), out)
        assert got == (1 if want else 0), hex(k)
        if want:
            assert bytes(out) == ref.sig_bytes(*want), hex(k)


def test_s_zero_reports_next_candidate_and_the_lane_takes_it(lib):
    """A digest chosen so that e + r x = 0 under the first nonce: sign_with_k reports s = 0, and the lane routine
    returns the signature under the next candidate, as the restatement does with that candidate refused."""
    rng = random.Random(0x51)
    out = (ctypes.c_uint8 * 64)()
    kout = (ctypes.c_uint8 * 32)()
    for _ in range(3):
        x, k = rng.randrange(1, N), rng.randrange(1, N)
        r = ref.mul(k, ref.G)[0] % N
        assert lib.ecdsa_p256_sign_shim_sign_with_k(be(x), be(-r * x % N), be(k), out) == 0
        assert bytes(out)[:32] == be(r) and bytes(out)[32:] == bytes(32)
        assert lib.ecdsa_p256_sign_shim_sign_with_k(be(x), be((1 - r * x) % N), be(k), out) == 1
    # The nonce is a function of the digest, so no digest reaches e + r x = 0 through a message.  The lane routine
    # takes the reduced digest apart from the one that seeds the generator: with e = -r x under the first nonce
    # it must pass on to the next candidate.
    for _ in range(12):
        x, h = rng.randrange(1, N), be(rng.getrandbits(256))
        k0 = sref.nonce(x, h)
        e = -(ref.mul(k0, ref.G)[0] % N) * x % N
        k1, r1, s1 = sref.sign_digest(x, h, e=e)
        assert k1 != k0 and (r1, s1) == sref.sign_with_k(x, e, k1)
        assert lib.ecdsa_p256_sign_shim_nonce_skip(be(x), h, ctypes.c_uint32(1), kout) >= 1
        assert int.from_bytes(bytes(kout), "big") == k1
        lib.ecdsa_p256_sign_shim_sign_digest_e(be(x), h, be(e), out)
        assert bytes(out) == ref.sig_bytes(r1, s1)


def test_unusable_keys(lib):
    out = (ctypes.c_uint8 * 64)()
    rec = (ctypes.c_uint32 * 32)()
    for x in (0, N, N + 1, FULL):
        assert lib.ecdsa_p256_sign_shim_sign(be(x), b"abc", ctypes.c_uint32(3), out) == 0
        assert bytes(out) == bytes(64)
        lib.ecdsa_p256_sign_shim_signer(be(x), rec)
        assert not any(rec)
    lib.ecdsa_p256_sign_shim_signer(be(N - 1), rec)
    words = list(rec)
    assert words[24] == 1 and not any(words[25:])
    q = ref.mul(N - 1, ref.G)
    assert sum(w << (32 * i) for i, w in enumerate(words[0:8])) == N - 1
    assert sum(w << (32 * i) for i, w in enumerate(words[8:16])) == q[0]
    assert sum(w << (32 * i) for i, w in enumerate(words[16:24])) == q[1]


def test_rs_to_der(lib):
    rng = random.Random(0xDE4)
    edge = [1, (1 << 255) - 1, 1 << 255, N - 1, 0x7F, 0x80, 0xFF, 0x100, (1 << 248) - 1, 1 << 247, 0]
    pairs = [(r, s) for r in edge for s in edge] + [(rng.randrange(1, N), rng.randrange(1, N)) for _ in range(200)]
    pairs += [(rng.getrandbits(8 * rng.randrange(1, 33)), rng.getrandbits(8 * rng.randrange(1, 33))) for _ in range(200)]
    der = (ctypes.c_uint8 * 80)()
    back = (ctypes.c_uint8 * 64)()
    for r, s in pairs:
        n = lib.ecdsa_p256_sign_shim_rs_to_der(be(r) + be(s), der)
        want = ref.der_encode(r, s)
        assert bytes(der)[:n] == want, (hex(r), hex(s))
        assert ref.der_to_rs(want) == be(r) + be(s)
        assert lib.ecdsa_p256_sign_shim_der_to_rs(want, ctypes.c_uint32(len(want)), back) == 1
        assert bytes(back) == be(r) + be(s)


def test_stand_alone_sanitizer_run():
    assert os.path.exists(SAN), "tests/cpp/ecdsa_p256_sign_shim_san not built (make ecdsa_p256_sign_shim)"
    p = subprocess.run([SAN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "as expected" in p.stdout
