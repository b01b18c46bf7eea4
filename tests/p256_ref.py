"""ECDSA P-256 (secp256r1, prime256v1) / SHA-256 verification restated on Python integers (the
semantics of cbft_ecdsa_load_keys_curve(CBFT_CURVE_P256) in include/cbft_hipcrypto.h, pinned to
OpenSSL 3.0.2 ECDSA_do_verify by tests/golden/ecdsa_p256_vectors.json), with the point arithmetic,
signing and key recovery the vector generator and the tests build their cases from.  The curve is
y^2 = x^3 - 3 x + b over GF(p), p = 2^256 - 2^224 + 2^192 + 2^96 - 1."""
import hashlib

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
A = P - 3
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
GX = 0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296
GY = 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5
G = (GX, GY)
INF = None  # the point at infinity


def on_curve(pt) -> bool:
    if pt is INF:
        return False
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - x * x * x + 3 * x - B) % P == 0


def neg(pt):
    return INF if pt is INF else (pt[0], (-pt[1]) % P)


def add(a, b):
    """The affine group law."""
    if a is INF:
        return b
    if b is INF:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return INF
        lam = (3 * a[0] * a[0] - 3) * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def mul_affine(k: int, pt):
    """k pt by double-and-add on the affine law above (slow: one inversion per step)."""
    k %= N
    acc = INF
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


# The same law on Jacobian triples (x = X / Z^2, y = Y / Z^3, Z = 0 for infinity): one inversion
# per scalar multiplication.  tests/test_ecdsa_p256_cpu.py checks it against mul_affine.
_JINF = (1, 1, 0)


def _jdbl(a):
    x, y, z = a
    if z == 0:
        return _JINF
    yy, zz = y * y % P, z * z % P
    s = 4 * x * yy % P
    m = 3 * (x - zz) * (x + zz) % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * yy * yy) % P, 2 * y * z % P)


def _jadd(a, b):
    if a[2] == 0:
        return b
    if b[2] == 0:
        return a
    z1z1, z2z2 = a[2] * a[2] % P, b[2] * b[2] % P
    u1, u2 = a[0] * z2z2 % P, b[0] * z1z1 % P
    s1, s2 = a[1] * b[2] * z2z2 % P, b[1] * a[2] * z1z1 % P
    if u1 == u2:
        return _jdbl(a) if s1 == s2 else _JINF
    h, r = (u2 - u1) % P, (s2 - s1) % P
    hh = h * h % P
    hhh, v = h * hh % P, u1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - s1 * hhh) % P, a[2] * b[2] * h % P)


def _to_jac(pt):
    return _JINF if pt is INF else (pt[0], pt[1], 1)


def _from_jac(a):
    if a[2] == 0:
        return INF
    zi = pow(a[2], -1, P)
    return (a[0] * zi * zi % P, a[1] * zi * zi * zi % P)


def mul2(k1: int, p1, k2: int, p2):
    """k1 p1 + k2 p2 (one joint double-and-add)."""
    k1, k2 = k1 % N, k2 % N
    j1, j2 = _to_jac(p1), _to_jac(p2)
    j12 = _jadd(j1, j2)
    acc = _JINF
    for i in range(max(k1.bit_length(), k2.bit_length()) - 1, -1, -1):
        acc = _jdbl(acc)
        b1, b2 = (k1 >> i) & 1, (k2 >> i) & 1
        if b1 or b2:
            acc = _jadd(acc, j12 if b1 and b2 else (j1 if b1 else j2))
    return _from_jac(acc)


def mul(k: int, pt):
    return mul2(k, pt, 0, INF)


def lift_x(x: int, odd: bool = False):
    """The curve point with this x (0 <= x < P) and the given parity of y, or None."""
    if not 0 <= x < P:
        return None
    rhs = (x * x * x - 3 * x + B) % P
    y = pow(rhs, (P + 1) // 4, P)
    if (y * y - rhs) % P:
        return None
    if (y & 1) != odd:
        y = P - y
    return (x, y)


def digest_int(msg: bytes) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


def pub_bytes(pt) -> bytes:
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def sig_bytes(r: int, s: int) -> bytes:
    """r || s as 32-byte big-endian integers (values up to 2^256 - 1 are representable)."""
    return r.to_bytes(32, "big") + s.to_bytes(32, "big")


def verify_ints(pub, r: int, s: int, e: int) -> bool:
    """pub: (X, Y) integers as they stand on the ABI (any 256-bit values)."""
    if not on_curve(pub):
        return False
    if not (1 <= r < N and 1 <= s < N):
        return False
    w = pow(s, -1, N)
    u1, u2 = e * w % N, r * w % N
    R = mul2(u1, G, u2, pub)
    if R is INF:
        return False
    return R[0] % N == r


def verify(pub64: bytes, sig64: bytes, msg: bytes) -> bool:
    if len(pub64) != 64 or len(sig64) != 64:
        return False
    pub = (int.from_bytes(pub64[:32], "big"), int.from_bytes(pub64[32:], "big"))
    r, s = int.from_bytes(sig64[:32], "big"), int.from_bytes(sig64[32:], "big")
    return verify_ints(pub, r, s, digest_int(msg))


def sign(d: int, msg: bytes, k: int):
    """(r, s) with the given nonce; None when r or s comes out 0."""
    R = mul(k, G)
    r = R[0] % N
    s = pow(k, -1, N) * (digest_int(msg) + r * d) % N
    return (r, s) if r and s else None


def recover_key(R, r: int, s: int, e: int):
    """Q = r^-1 (s R - e G): the key under which (r, s) verifies e with u1 G + u2 Q = R."""
    ri = pow(r, -1, N)
    return mul(ri, add(mul(s, R), neg(mul(e, G))))


def der_to_rs(der: bytes, order_bytes: int = 32):
    """Strict DER SEQUENCE { INTEGER r, INTEGER s } -> r || s (each order_bytes wide), or None:
    the restatement of csrc/ecdsa_der.h."""

    def length(b, i):  # -> (length, next index) or None; minimal definite form only
        if i >= len(b):
            return None
        l0 = b[i]
        if l0 < 0x80:
            return l0, i + 1
        nb = l0 & 0x7F
        if nb == 0 or nb > 4 or i + 1 + nb > len(b) or b[i + 1] == 0:
            return None
        v = int.from_bytes(b[i + 1:i + 1 + nb], "big")
        if v < 0x80:
            return None
        return v, i + 1 + nb

    def integer(b, i):
        if i >= len(b) or b[i] != 0x02:
            return None
        got = length(b, i + 1)
        if got is None:
            return None
        ln, i = got
        if ln == 0 or i + ln > len(b):
            return None
        body = b[i:i + ln]
        if body[0] & 0x80:
            return None  # negative
        if ln > 1 and body[0] == 0 and not body[1] & 0x80:
            return None  # superfluous leading zero
        v = int.from_bytes(body, "big")
        if v >> (8 * order_bytes):
            return None
        return v, i + ln

    if len(der) < 2 or der[0] != 0x30:
        return None
    got = length(der, 1)
    if got is None:
        return None
    ln, i = got
    if i + ln != len(der):
        return None
    a = integer(der, i)
    if a is None:
        return None
    r, i = a
    a = integer(der, i)
    if a is None:
        return None
    s, i = a
    if i != len(der):
        return None
    return r.to_bytes(order_bytes, "big") + s.to_bytes(order_bytes, "big")


def der_encode(r: int, s: int) -> bytes:
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 8) // 8), "big")
        return b"\x02" + ln(len(b)) + b

    def ln(n):
        if n < 0x80:
            return bytes([n])
        b = n.to_bytes((n.bit_length() + 7) // 8, "big")
        return bytes([0x80 | len(b)]) + b

    body = integer(r) + integer(s)
    return b"\x30" + ln(len(body)) + body
