#!/usr/bin/env python3
"""Generates tests/golden/ecdsa_p256_vectors.json: ECDSA P-256 (prime256v1) / SHA-256 verification
vectors whose verdicts are OpenSSL's (ECDSA_do_verify through ctypes: 1 is accept, anything else, the
-1 of an infinite R included, is reject; a key EC_KEY_set_public_key_affine_coordinates refuses
rejects everything).  Asserts that tests/p256_ref.py agrees on every vector.  Deterministic.

    python3 tests/golden/gen_ecdsa_p256_vectors.py

File: {"keys": [hex of X || Y], "vectors": [{"cls", "key", "sig" (hex r || s), "msg" (hex), "ok"}]}.

The classes are those of gen_ecdsa_vectors.py, and:
  key_x_zero            the keys (0, +-sqrt(b)), which are on P-256 and usable (rejects only: an accepted
                        signature under them needs their discrete logarithm)
  rx_above_n[_unreduced] x(R) in [n, p): p - n < 2^127, so r = x - n is small and only a chosen R
                        reaches the second arm of the closing test
  field_edge            R whose x has a 32-bit word of all ones or all zeros at each of the eight
                        positions, and R = k G with x or y having such a word.  A word of a random
                        coordinate is all ones or all zeros with probability 2^-31, so the bounded
                        search over k G finds none (it is run and its count printed); the x of
                        the first kind is written down and lifted to the curve instead, and the
                        key recovered from it.
  rfc6979_a25           the two SHA-256 signatures of RFC 6979 A.2.5, recomputed from its key and
                        nonces
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import p256_ref as ref  # noqa: E402

N, P, G = ref.N, ref.P, ref.G
NID_X9_62_PRIME256V1 = 415

_c = ctypes.CDLL(ctypes.util.find_library("crypto"))
_vp = ctypes.c_void_p
for name, res, args in [
    ("EC_KEY_new_by_curve_name", _vp, [ctypes.c_int]),
    ("EC_KEY_free", None, [_vp]),
    ("EC_KEY_set_public_key_affine_coordinates", ctypes.c_int, [_vp, _vp, _vp]),
    ("BN_bin2bn", _vp, [ctypes.c_char_p, ctypes.c_int, _vp]),
    ("BN_free", None, [_vp]),
    ("ECDSA_SIG_new", _vp, []),
    ("ECDSA_SIG_free", None, [_vp]),
    ("ECDSA_SIG_set0", ctypes.c_int, [_vp, _vp, _vp]),
    ("ECDSA_do_verify", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, _vp, _vp]),
    ("ECDSA_verify", ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, _vp]),
    ("ERR_clear_error", None, []),
]:
    fn = getattr(_c, name)
    fn.restype, fn.argtypes = res, args


def _bn(b: bytes):
    return _c.BN_bin2bn(b, len(b), None)


def _load_key(pub64: bytes):
    key = _c.EC_KEY_new_by_curve_name(NID_X9_62_PRIME256V1)
    assert key
    x, y = _bn(pub64[:32]), _bn(pub64[32:])
    loaded = _c.EC_KEY_set_public_key_affine_coordinates(key, x, y)
    _c.BN_free(x)
    _c.BN_free(y)
    return key, loaded == 1


def openssl_verdict(pub64: bytes, sig64: bytes, msg: bytes) -> int:
    """1 iff OpenSSL loads the key and ECDSA_do_verify returns 1."""
    key, loaded = _load_key(pub64)
    ok = 0
    if loaded:
        sig = _c.ECDSA_SIG_new()
        assert _c.ECDSA_SIG_set0(sig, _bn(sig64[:32]), _bn(sig64[32:])) == 1  # sig owns r, s
        ok = 1 if _c.ECDSA_do_verify(hashlib.sha256(msg).digest(), 32, sig, key) == 1 else 0
        _c.ECDSA_SIG_free(sig)
    _c.EC_KEY_free(key)
    _c.ERR_clear_error()
    return ok


def openssl_der_verdict(pub64: bytes, der: bytes, msg: bytes) -> int:
    """1 iff OpenSSL loads the key and ECDSA_verify (the DER entry point) returns 1."""
    key, loaded = _load_key(pub64)
    ok = 0
    if loaded:
        ok = 1 if _c.ECDSA_verify(0, hashlib.sha256(msg).digest(), 32, der, len(der), key) == 1 else 0
    _c.EC_KEY_free(key)
    _c.ERR_clear_error()
    return ok


def zero_run_scalars():
    """Scalars with 64-bit runs of zero bits at each of the four 64-bit positions."""
    full = (1 << 256) - 1
    out = []
    for pos in range(4):
        v = (0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95 & full)
        v &= ~(((1 << 64) - 1) << (64 * pos))
        out.append(v % N)
    return out


def edge_words(v: int):
    """[(position, 'ones' | 'zeros')] for the 32-bit words of v that are all ones or all zeros."""
    out = []
    for i in range(8):
        w = (v >> (32 * i)) & 0xFFFFFFFF
        if w == 0xFFFFFFFF:
            out.append((i, "ones"))
        elif w == 0:
            out.append((i, "zeros"))
    return out


def check_restatement():
    """The restatement's Jacobian arithmetic against its own affine law, before anything is built on it."""
    rng = random.Random(7)
    for _ in range(4):
        k = rng.randrange(1, N)
        assert ref.mul(k, G) == ref.mul_affine(k, G)
    assert ref.mul(N, G) is ref.INF and ref.mul(N - 1, G) == ref.neg(G)


def main():
    check_restatement()
    rng = random.Random(0x9256)
    keys, key_index, vectors = [], {}, []

    def key_id(pub64: bytes) -> int:
        if pub64 not in key_index:
            key_index[pub64] = len(keys)
            keys.append(pub64)
        return key_index[pub64]

    def emit(cls: str, pub64: bytes, sig64: bytes, msg: bytes, want=None):
        ok = openssl_verdict(pub64, sig64, msg)
        mine = 1 if ref.verify(pub64, sig64, msg) else 0
        assert ok == mine, f"{cls}: OpenSSL {ok}, p256_ref {mine}"
        if want is not None:
            assert ok == want, f"{cls}: expected {want}, OpenSSL says {ok}"
        vectors.append({"cls": cls, "key": key_id(pub64), "sig": sig64.hex(), "msg": msg.hex(), "ok": ok})

    def rand_scalar():
        return rng.randrange(1, N)

    privs = [rand_scalar() for _ in range(4)]
    pubs = [ref.pub_bytes(ref.mul(d, G)) for d in privs]

    def signed(ki: int, msg: bytes):
        while True:
            rs = ref.sign(privs[ki], msg, rand_scalar())
            if rs:
                return rs

    # valid signatures over the SHA-256 padding boundaries, their high-s twins, single-bit damage
    for length in (0, 1, 55, 56, 63, 64, 119, 120, 256, 4096):
        for ki in range(3 if length < 4096 else 1):
            msg = rng.randbytes(length)
            r, s = signed(ki, msg)
            emit("valid", pubs[ki], ref.sig_bytes(r, s), msg, 1)
            emit("high_s_twin", pubs[ki], ref.sig_bytes(r, N - s), msg, 1)
            if ki == 0:
                emit("flip_r", pubs[ki], ref.sig_bytes(r ^ (1 << rng.randrange(256)), s), msg)
                emit("flip_s", pubs[ki], ref.sig_bytes(r, s ^ (1 << rng.randrange(256))), msg)
                bad = bytearray(msg) if msg else bytearray(b"\0")
                bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
                emit("flip_msg", pubs[ki], ref.sig_bytes(r, s), bytes(bad), 0)
                emit("flip_key_index", pubs[ki + 1], ref.sig_bytes(r, s), msg, 0)

    # r, s out of range
    msg = b"range checks"
    r, s = signed(0, msg)
    full = (1 << 256) - 1
    for cls, rr, ss in [("r_zero", 0, s), ("s_zero", r, 0), ("r_eq_n", N, s), ("s_eq_n", r, N),
                        ("r_above_n", N + 1, s), ("s_above_n", r, N + 1), ("r_max", full, s), ("s_max", r, full),
                        ("r_s_zero", 0, 0)]:
        emit(cls, pubs[0], ref.sig_bytes(rr, ss), msg, 0)

    # small s and small r by key recovery, then s + n and r + n written in their place
    for i in range(4):
        msg = b"small s %d" % i
        e = ref.digest_int(msg)
        R = ref.mul(rand_scalar(), G)
        r, s = R[0] % N, rng.randrange(1, 1 << 100)
        q = ref.pub_bytes(ref.recover_key(R, r, s, e))
        emit("small_s", q, ref.sig_bytes(r, s), msg, 1)
        emit("s_plus_n", q, ref.sig_bytes(r, s + N), msg, 0)
    x, found = 1, 0
    while found < 4:
        R = ref.lift_x(x, odd=bool(found & 1))
        x += 1
        if R is None:
            continue
        msg = b"small r %d" % found
        e, r, s = ref.digest_int(msg), R[0], rand_scalar()
        q = ref.pub_bytes(ref.recover_key(R, r, s, e))
        emit("small_r", q, ref.sig_bytes(r, s), msg, 1)
        emit("r_plus_n", q, ref.sig_bytes(r + N, s), msg, 0)
        found += 1

    # unusable keys: every signature under them is rejected (OpenSSL refuses the key)
    msg = b"unusable keys"
    r, s = signed(0, msg)
    qx, qy = ref.mul(privs[0], G)
    bad_keys = [("key_off_curve", qx.to_bytes(32, "big") + ((qy + 1) % P).to_bytes(32, "big")),
                ("key_off_curve", ((qx + 1) % P).to_bytes(32, "big") + qy.to_bytes(32, "big")),
                ("key_zero", bytes(64)),
                ("key_x_eq_p", P.to_bytes(32, "big") + qy.to_bytes(32, "big")),
                ("key_y_eq_p", qx.to_bytes(32, "big") + P.to_bytes(32, "big")),
                ("key_max", b"\xff" * 64)]
    # a valid point whose x is small enough that x + p fits 256 bits: the unreduced form is refused
    xs = 1
    while ref.lift_x(xs) is None:
        xs += 1
    small_pt = ref.lift_x(xs)
    assert small_pt[0] + P < 1 << 256
    bad_keys.append(("key_x_plus_p", (small_pt[0] + P).to_bytes(32, "big") + small_pt[1].to_bytes(32, "big")))
    for cls, kb in bad_keys:
        emit(cls, kb, ref.sig_bytes(r, s), msg, 0)
        emit(cls, kb, ref.sig_bytes(1, 1), b"", 0)

    # the keys with x = 0: (0, +-sqrt(b)) is on this curve and OpenSSL loads it.  An accepted signature
    # under it needs its discrete logarithm (e is a SHA-256 output, not ours to choose), so the vectors
    # here are rejects under a usable key; tests/test_ecdsa_p256_cpu.py
    # (test_accept_under_the_keys_with_x_zero_for_a_chosen_digest) runs the accepting case on the lane code
    # with a chosen e against the restatement.
    for odd in (False, True):
        Q0 = ref.lift_x(0, odd)
        assert Q0 is not None and Q0[0] == 0
        key, loaded = _load_key(ref.pub_bytes(Q0))
        _c.EC_KEY_free(key)
        assert loaded, "OpenSSL refuses (0, sqrt(b))"
        for i in range(2):
            msg = b"key x zero %d %d" % (odd, i)
            a, b = rand_scalar(), rand_scalar()
            R = ref.mul2(a, G, b, Q0)
            r = R[0] % N
            emit("key_x_zero", ref.pub_bytes(Q0), ref.sig_bytes(r, r * pow(b, -1, N) % N), msg, 0)

    # x(R) in [n, p): r = x - n verifies, the unreduced x written as r is rejected
    x, found = N + 2, 0
    while found < 6:
        R = ref.lift_x(x, odd=bool(found & 1))
        x += 1
        if R is None:
            continue
        assert N <= R[0] < P
        msg = b"x(R) above n %d" % found
        e, r, s = ref.digest_int(msg), R[0] - N, rand_scalar()
        q = ref.pub_bytes(ref.recover_key(R, r, s, e))
        emit("rx_above_n", q, ref.sig_bytes(r, s), msg, 1)
        emit("rx_above_n_unreduced", q, ref.sig_bytes(R[0], s), msg, 0)
        found += 1

    # field_edge: R = k G over a bounded range of k with an all-ones or all-zeros word in x or y ...
    k0 = rng.randrange(1, N - (1 << 20))
    Rj, hits = ref.mul(k0, G), 0
    for i in range(4096):
        for coord in Rj:
            if edge_words(coord):
                hits += 1
                msg = b"field edge search %d" % i
                rs = ref.sign(privs[0], msg, k0 + i)
                emit("field_edge", pubs[0], ref.sig_bytes(*rs), msg, 1)
                break
        Rj = ref.add(Rj, G)
    print(f"field_edge: the search over 4096 consecutive k G found {hits} (expected 0: 2^-31 a word)")
    # ... and R with such a word written into x at every position, lifted to the curve
    for pos in range(8):
        for kind in ("ones", "zeros"):
            while True:
                x = rng.randrange(1 << 256)
                x &= ~(0xFFFFFFFF << (32 * pos))
                if kind == "ones":
                    x |= 0xFFFFFFFF << (32 * pos)
                    if pos == 7:
                        x &= ~(0xFFFFFFFF << 192)  # below p = ffffffff 00000001 00000000 ..
                R = ref.lift_x(x, odd=bool(rng.randrange(2))) if x < P else None
                if R is not None and (pos, kind) in edge_words(R[0]):
                    break
            msg = b"field edge %d %s" % (pos, kind.encode())
            e, r, s = ref.digest_int(msg), R[0] % N, rand_scalar()
            q = ref.pub_bytes(ref.recover_key(R, r, s, e))
            emit("field_edge", q, ref.sig_bytes(r, s), msg, 1)
    assert {(p_, k_) for p_ in range(8) for k_ in ("ones", "zeros")} <= {
        w for v in vectors if v["cls"] == "field_edge" for w in [(int(bytes.fromhex(v["msg"]).split()[2]),
                                                                   bytes.fromhex(v["msg"]).split()[3].decode())]
        if not bytes.fromhex(v["msg"]).startswith(b"field edge search")}

    # chosen u1 (then chosen u2): zero digits, first digits, the top bit, negation
    chosen = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255] + zero_run_scalars()
    for which in ("u1", "u2"):
        for i, u in enumerate(chosen):
            msg = b"chosen %s %d" % (which.encode(), i)
            e = ref.digest_int(msg) % N
            while True:
                k = rand_scalar()
                R = ref.mul(k, G)
                r = R[0] % N
                if which == "u1":
                    u1, s = u, e * pow(u, -1, N) % N
                    u2 = r * u1 * pow(e, -1, N) % N
                else:
                    u2, s = u, r * pow(u, -1, N) % N
                    u1 = e * u2 * pow(r, -1, N) % N
                T = ref.add(R, ref.neg(ref.mul(u1, G)))
                if r and s and T is not ref.INF:
                    break
            q = ref.pub_bytes(ref.mul(pow(u2, -1, N), T))
            emit("chosen_" + which, q, ref.sig_bytes(r, s), msg, 1)

    # u1 G = u2 Q (R = 2 u1 G, accept) and u1 G = -u2 Q (R = infinity, reject)
    for i in range(4):
        msg = b"closing doubling %d" % i
        e = ref.digest_int(msg) % N
        t = rand_scalar()
        T = ref.mul(t, G)
        R = ref.add(T, T)
        r = R[0] % N
        s = e * pow(t, -1, N) % N
        u2 = r * t * pow(e, -1, N) % N
        q = ref.mul(t * pow(u2, -1, N) % N, G)
        emit("closing_doubling", ref.pub_bytes(q), ref.sig_bytes(r, s), msg, 1)
        msg = b"closing infinity %d" % i
        e = ref.digest_int(msg) % N
        r = ref.mul(rand_scalar(), G)[0] % N
        s = e * pow(t, -1, N) % N
        u2 = r * t * pow(e, -1, N) % N
        q = ref.neg(ref.mul(t * pow(u2, -1, N) % N, G))
        emit("closing_infinity", ref.pub_bytes(q), ref.sig_bytes(r, s), msg, 0)

    # keys that are small multiples of G, signed until the top 4-bit windows of u1 and u2 hold the
    # same digit: a windowed double-scalar multiplication then adds d G to d G (Q = G) or to -d G
    # (Q = -G) at its first step
    for c in (1, N - 1, 2, N - 2, 3):
        q = ref.pub_bytes(ref.mul(c, G))
        for i in range(3):
            tries = 0
            while True:
                msg = b"window collision %d %d %d" % (c % 7, i, tries)
                tries += 1
                rs = ref.sign(c, msg, rand_scalar())
                if not rs:
                    continue
                r, s = rs
                w = pow(s, -1, N)
                u1, u2 = ref.digest_int(msg) * w % N, r * w % N
                if (u1 >> 252) == (u2 >> 252) and (u1 >> 252):
                    break
            emit("window_collision", q, ref.sig_bytes(r, s), msg, 1)

    # RFC 6979 A.2.5 (P-256, SHA-256): the key and the nonces are the anchors of
    # gen_ecdsa_sign_vectors.py; the signatures are recomputed here and are the RFC's
    x = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    U = ref.mul(x, G)
    assert U[0] == 0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6
    for msg, k, want_r, want_s in (
            (b"sample", 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
             0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
             0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8),
            (b"test", 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0,
             0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
             0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083)):
        r, s = ref.sign(x, msg, k)
        assert (r, s) == (want_r, want_s), msg
        emit("rfc6979_a25", ref.pub_bytes(U), ref.sig_bytes(r, s), msg, 1)

    out = {"keys": [k.hex() for k in keys], "vectors": vectors}
    path = os.path.join(HERE, "ecdsa_p256_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    classes = {}
    for v in vectors:
        classes[v["cls"]] = classes.get(v["cls"], 0) + 1
    print(f"{len(vectors)} vectors, {len(keys)} keys, {os.path.getsize(path)} bytes")
    print(classes)


if __name__ == "__main__":
    main()
