"""Operand sets and exact-integer references for the Ed25519 lane code (csrc/fe25519.h with the
generated fe25519_asm*.h, sc25519.h, ge25519.h), used by tests/test_fe25519_lane_gpu.py (the compiled
code on gfx950, through tests/hip/fe25519_selftest.hip) and checked by tests/test_fe25519_cases_cpu.py.

Pure Python; the only project module imported is oracle/ed25519_ref.py.  Every reference is a Python
integer computation: val(a) val(b) mod p, pow(x, p - 2, p) with 0 -> 0, pow(x, (p - 5) // 8, p),
x % L, and ed25519_ref.decode_point / point_add / encode_point.

The limb bounds of fe25519.h are written down once (BOUND) and serve both to generate operands and to
check outputs:
  reduced  every limb < 2^29 + 2^17
  lazy     every limb < 2^30 + 2^18
  sublazy  limb i < 2^29 + 2^17 + SUB65P[i]   (fe_sub_lazy: reduced - reduced + 65p, no carry pass)
  wide     every limb < 2^32 - 8              (what fe_carry, hence fe_to_words, accepts)

Every set is shuffled with a fixed seed, so neighbouring lanes hold different classes, and its length
is never a multiple of 64, so the last block of a launch is partly idle.

sc_reduce512: closing_subtractions(x) counts how often the Barrett estimate (mu = floor(2^512 / L), as
the header has it) leaves L to subtract.  On the edge family of sc_reduce_cases() 267 cases need 0 and
526 need 1.  A search over 200,000 random 512-bit values found none that needs 2, and none exists: the
estimate falls short of x / L by less than (2^512 / L + 2^288 frac(2^512 / L)) / 2^288 < 1
(test_fe25519_cases_cpu.py evaluates that bound exactly), so the quotient is short by at most 1.
"""
import os
import random
import sys
from collections import namedtuple

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ed25519_ref as E  # noqa: E402

P = E.P
L = E.L
MASK = 2**29 - 1
REDUCED = 2**29 + 2**17
LAZY = 2 * REDUCED
SUB65P = [2**30 - 1235] + [2**30 - 2] * 7 + [2**29 + 2**23 - 2]   # fe_sub_lazy's digits of 65p
SUB256P = [2**31 - 4864] + [2**31 - 4] * 8                          # fe_sub / fe_neg's digits of 256p
WIDE = 2**32 - 8
BOUND = {"reduced": [REDUCED] * 9, "lazy": [LAZY] * 9, "sublazy": [REDUCED + m for m in SUB65P], "wide": [WIDE] * 9}
MU = 2**512 // L
ZERO = [0] * 9

# operands: a tuple of limb vectors (or word integers); cls: the declared class of each; kind: the family
Case = namedtuple("Case", "kind cls operands extra", defaults=(None,))


def value(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def limbs29(x):
    """The radix-2^29 digits of 0 <= x < 2^261."""
    assert 0 <= x < 2**261
    return [(x >> (29 * i)) & MASK for i in range(9)]


def in_class(limbs, cls):
    return len(limbs) == 9 and all(0 <= x < b for x, b in zip(limbs, BOUND[cls]))


def top(cls):
    return [b - 1 for b in BOUND[cls]]


def redundant(x, cls, rng):
    """A random limb vector of class cls whose value is == x (mod p): random slack below the bound in
    every limb, plus the 29-bit digits of the difference shifted by a random multiple of p."""
    b = BOUND[cls]
    r = [rng.randrange(b[i] - MASK) for i in range(9)]
    c = limbs29((x - value(r)) % P + rng.randrange(64) * P)
    out = [ci + ri for ci, ri in zip(c, r)]
    assert in_class(out, cls) and value(out) % P == x % P
    return out


def words(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---- the header's limb-exact functions, restated (their outputs are inputs of other cases) ----
def model_carry(l):
    l = list(l)
    for i in range(8):
        l[i + 1] += l[i] >> 29
        l[i] &= MASK
    c = l[8] >> 29
    l[8] &= MASK
    l[0] += c * 1216
    return l


def model_sub(a, b):
    return model_carry([x + m - y for x, m, y in zip(a, SUB256P, b)])


def model_sub_lazy(a, b):
    return [x + m - y for x, m, y in zip(a, SUB65P, b)]


def _finish(cases, seed):
    cases = list(cases)
    random.Random(seed).shuffle(cases)
    if len(cases) % 64 == 0:
        cases.append(cases[0])
    return cases


def _draw(cls, rng):
    b = BOUND[cls]
    return [rng.choice((0, b[i] - 1, b[i] - 2, 2**29 - 1, 2**29)) for i in range(9)]


def _uniform(cls, rng):
    return [rng.randrange(x) for x in BOUND[cls]]


# ---- field products -------------------------------------------------------------------------
PAIRS_MUL = [(a, b) for a in ("reduced", "lazy") for b in ("reduced", "lazy")]
# fold32: (reduced | lazy | sublazy) x (reduced | lazy), and lazy x sublazy; never sublazy x sublazy
PAIRS_FOLD = [(a, b) for a in ("reduced", "lazy", "sublazy") for b in ("reduced", "lazy")] + [("lazy", "sublazy")]


def _pair_cases(ca, cb, rng, n_set=60, n_canon=30, n_uniform=60):
    A, B = top(ca), top(cb)
    yield Case("max", (ca, cb), (A, B))
    yield Case("zero", (ca, cb), (ZERO, B))
    yield Case("zero", (ca, cb), (A, ZERO))
    yield Case("zero", (ca, cb), (ZERO, ZERO))
    for i in range(9):
        for j in range(9):
            yield Case("onehot", (ca, cb), ([A[k] if k == i else 0 for k in range(9)],
                                            [B[k] if k == j else 0 for k in range(9)]))
    for _ in range(n_set):
        yield Case("set", (ca, cb), (_draw(ca, rng), _draw(cb, rng)))
    for _ in range(n_canon):
        yield Case("canonical", (ca, cb), (limbs29(rng.randrange(P)), limbs29(rng.randrange(P))))
    for _ in range(n_uniform):
        yield Case("uniform", (ca, cb), (_uniform(ca, rng), _uniform(cb, rng)))


def _mul_groups(fold):
    rng = random.Random(0xF01D if fold else 0x3A1)
    return [list(_pair_cases(ca, cb, rng)) for ca, cb in (PAIRS_FOLD if fold else PAIRS_MUL)]


def mul_cases(fold=False):
    """Operand pairs of fe_mul<*> (fold = False) or of the fold32 multiply (fold = True)."""
    return _finish([c for g in _mul_groups(fold) for c in g], 1)


def mul2_cases(fold=False):
    """Pairs of cases for the two-product forms: the second slot holds the next class pair's case,
    so the two slots of one statement carry operands of different classes."""
    groups = _mul_groups(fold)
    slot0 = [c for g in groups for c in g]
    slot1 = [c for g in groups[1:] + groups[:1] for c in g]
    assert all(x.cls != y.cls for x, y in zip(slot0, slot1))
    return _finish(zip(slot0, slot1), 2)


def sq_cases():
    rng = random.Random(0x5C)
    out = []
    for cls in ("reduced", "lazy"):
        A = top(cls)
        out += [Case("max", (cls,), (A,)), Case("zero", (cls,), (ZERO,))]
        for i in range(9):
            for j in range(i, 9):  # one limb, or two (the doubled cross terms)
                out.append(Case("onehot", (cls,), ([A[k] if k in (i, j) else 0 for k in range(9)],)))
        out += [Case("set", (cls,), (_draw(cls, rng),)) for _ in range(80)]
        out += [Case("canonical", (cls,), (limbs29(rng.randrange(P)),)) for _ in range(40)]
        out += [Case("uniform", (cls,), (_uniform(cls, rng),)) for _ in range(80)]
    return _finish(out, 3)


SMALL = (0, 1, 2, 19, 1216, 2**15, 2**16 - 1)


def mul_small_cases():
    rng = random.Random(0x51)
    out = []
    for cls in ("reduced", "lazy"):
        for s in SMALL:
            out += [Case("max", (cls,), (top(cls),), s), Case("zero", (cls,), (ZERO,), s)]
            out += [Case("onehot", (cls,), ([top(cls)[k] if k == i else 0 for k in range(9)],), s) for i in range(9)]
            out += [Case("set", (cls,), (_draw(cls, rng),), s) for _ in range(12)]
            out += [Case("canonical", (cls,), (limbs29(rng.randrange(P)),), s) for _ in range(6)]
            out += [Case("uniform", (cls,), (_uniform(cls, rng),), s) for _ in range(12)]
    return _finish(out, 4)


def addsub_cases(pairs=PAIRS_MUL):
    """fe_add / fe_sub / fe_neg (which reads the first operand only); pairs = [("reduced", "reduced")]
    for fe_sub_lazy."""
    rng = random.Random(0xAD5 + len(pairs))
    out = []
    for ca, cb in pairs:
        A, B = top(ca), top(cb)
        out += [Case("max", (ca, cb), (A, B)), Case("zero", (ca, cb), (ZERO, B)), Case("zero", (ca, cb), (A, ZERO)),
                Case("zero", (ca, cb), (ZERO, ZERO))]
        for i in range(9):  # the largest borrow and the largest sum, one limb at a time
            hot_a, hot_b = [A[k] if k == i else 0 for k in range(9)], [B[k] if k == i else 0 for k in range(9)]
            out += [Case("onehot", (ca, cb), (hot_a, ZERO)), Case("onehot", (ca, cb), (ZERO, hot_b)),
                    Case("onehot", (ca, cb), (hot_a, hot_b))]
        out += [Case("set", (ca, cb), (_draw(ca, rng), _draw(cb, rng))) for _ in range(60)]
        out += [Case("canonical", (ca, cb), (limbs29(rng.randrange(P)), limbs29(rng.randrange(P)))) for _ in range(30)]
        out += [Case("uniform", (ca, cb), (_uniform(ca, rng), _uniform(cb, rng))) for _ in range(60)]
        if ca == cb:
            for _ in range(20):  # a - a
                a = _uniform(ca, rng)
                out.append(Case("equal", (ca, cb), (a, list(a))))
    return _finish(out, 5)


def sub_lazy_cases():
    return addsub_cases([("reduced", "reduced")])


def carry_cases():
    rng = random.Random(0xCA)
    A = top("wide")
    out = [Case("max", ("wide",), (A,)), Case("zero", ("wide",), (ZERO,))]
    out += [Case("onehot", ("wide",), ([A[k] if k == i else 0 for k in range(9)],)) for i in range(9)]
    out += [Case("onehot", ("wide",), ([A[k] if k != i else 0 for k in range(9)],)) for i in range(9)]
    for _ in range(150):
        out.append(Case("set", ("wide",), ([rng.choice((0, WIDE - 1, WIDE - 2, 2**29 - 1, 2**29, 2**32 - 2**29))
                                            for _ in range(9)],)))
    out += [Case("uniform", ("wide",), (_uniform("wide", rng),)) for _ in range(150)]
    for cls in ("reduced", "lazy", "sublazy"):
        out += [Case("max", (cls,), (top(cls),))] + [Case("uniform", (cls,), (_uniform(cls, rng),)) for _ in range(30)]
    return _finish(out, 6)


# ---- canonicalisation -----------------------------------------------------------------------
CANON_VALUES = [0, 1, 18, 19, 20, P - 1, P, P + 1, P + 18, P + 19, 2 * P - 1, 2 * P, 2**255 - 1, 2**255, 64 * P, 65 * P]


def canon_cases():
    """Inputs of fe_to_words / fe_iszero / fe_isnegative: the values around 0, p, 2p, 2^255, 64p and 65p
    written with 29-bit digits where they fit (65p with fe_sub_lazy's digits), the same residues as
    redundant limb vectors of every class, differences of equal values through fe_sub and fe_sub_lazy
    (representations of 0 as the product meets them), every class at its bound, and random limbs."""
    rng = random.Random(0xCA909)
    out = []
    for x in CANON_VALUES:
        out.append(Case("exact", ("wide",), (limbs29(x) if x < 2**261 else list(SUB65P),)))
        assert value(out[-1].operands[0]) == x
        for cls in ("reduced", "lazy", "sublazy", "wide"):
            out += [Case("redundant", (cls,), (redundant(x, cls, rng),)) for _ in range(6)]
    for cls in ("reduced", "lazy"):
        for _ in range(25):  # a - a', a' == a: zero through fe_sub, from the same and from another limb vector
            a = _uniform(cls, rng)
            out.append(Case("sub", ("reduced",), (model_sub(a, a),)))
            out.append(Case("sub", ("reduced",), (model_sub(a, redundant(value(a), cls, rng)),)))
    for _ in range(25):
        a = _uniform("reduced", rng)
        out.append(Case("sub_lazy", ("sublazy",), (model_sub_lazy(a, a),)))
        out.append(Case("sub_lazy", ("sublazy",), (model_sub_lazy(a, redundant(value(a), "reduced", rng)),)))
    for cls in ("reduced", "lazy", "sublazy", "wide"):
        out.append(Case("max", (cls,), (top(cls),)))
        out += [Case("set", (cls,), (_draw(cls, rng),)) for _ in range(40)]
        out += [Case("uniform", (cls,), (_uniform(cls, rng),)) for _ in range(60)]
    out += [Case("canonical", ("reduced",), (limbs29(rng.randrange(P)),)) for _ in range(60)]
    return _finish(out, 7)


def from_words_cases():
    """256-bit integers for fe_from_words: the expected limbs are the 29-bit digits of the low 255 bits."""
    rng = random.Random(0xF0)
    xs = [0, P - 1] + list(range(P, 2**255)) + [1, 2**255 - 20]
    xs += [x | 2**255 for x in xs] + [2**256 - 1]
    xs += [1 << k for k in range(256)] + [(2**256 - 1) ^ (1 << k) for k in range(0, 256, 3)]
    xs += [rng.getrandbits(256) for _ in range(200)]
    return _finish(xs, 8)


def inv_cases(wave=False):
    """Inputs of fe_invert / fe_invert_var / fe_pow22523: at most 256 for the one-wave-per-value form."""
    rng = random.Random(0x1A7 + wave)
    vals = [0, 1, 2, P - 1, P - 2, E.SQRT_M1] + [pow(2, k, P) for k in list(range(0, 255, 4 if wave else 2)) + [255, 256, 260]]
    out = [Case("canonical", ("reduced",), (limbs29(x),)) for x in vals]
    out += [Case("redundant", ("lazy",), (redundant(x, "lazy", rng),)) for x in (vals[:40] if wave else vals)]
    if not wave:
        out += [Case("redundant", ("reduced",), (redundant(x, "reduced", rng),)) for x in vals]
    n = 40 if wave else 100
    out += [Case("canonical", ("reduced",), (limbs29(rng.randrange(P)),)) for _ in range(n)]
    out += [Case("uniform", ("lazy",), (_uniform("lazy", rng),)) for _ in range(n)]
    out += [Case("max", (cls,), (top(cls),)) for cls in ("reduced", "lazy")]
    assert not wave or len(out) <= 256
    return _finish(out, 9)


# ---- scalars --------------------------------------------------------------------------------
def sc_canon_cases():
    rng = random.Random(0x5CA)
    xs = [0, L - 1, L, L + 1, 2**252, 2**256 - 1]
    for i in range(8):  # L with word i one up and one down (words 4..6 of L are 0: one down borrows from word 7)
        xs += [L + (1 << (32 * i)), L - (1 << (32 * i))]
    xs += [rng.getrandbits(256) for _ in range(60)]
    xs += [rng.randrange(L) for _ in range(60)]
    xs +=[L + rng.getrandbits(k) for k in range(1, 250, 5)] + [L - 1 - rng.getrandbits(k) for k in range(1, 250, 5)]
    return _finish([x for x in xs if 0 <= x < 2**256], 10)


def closing_subtractions(x):
    """How many times sc_reduce512's closing loop must subtract L: x - q3 L over L, with the Barrett
    estimate q3 = floor(floor(x / 2^224) mu / 2^288) of the header."""
    q3 = ((x >> 224) * MU) >> 288
    t = x - q3 * L
    assert 0 <= t
    return t // L


def sc_reduce_edge_cases():
    xs = [0, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2**512 - 1, 2**512 - L, (2**512 // L) * L, (2**512 // L) * L - 1]
    for k in range(0, 260, 3):
        for q in (2**k - 1, 2**k, 2**k + 1):
            xs += [q * L + r for r in (0, 1, L - 1)]
    assert all(x < 2**512 for x in xs)
    return xs


def sc_reduce_cases():
    rng = random.Random(0x5C512)
    xs = sc_reduce_edge_cases() + [rng.getrandbits(512) for _ in range(300)]
    xs += [rng.getrandbits(k) for k in range(1, 512, 4)]
    return _finish(xs, 11)


# ---- decoding -------------------------------------------------------------------------------
def root_kind(y):
    """'direct' if the (p + 3) / 8 power is already the root, 'sqrtm1' if it needs the factor sqrt(-1),
    None if y is off the curve (ed25519_ref._recover_x's steps)."""
    y %= P
    u, v = (y * y - 1) % P, (E.D * y * y + 1) % P
    x = (u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P)) % P
    vxx = v * x * x % P
    return "direct" if vxx == u else "sqrtm1" if vxx == (-u) % P else None


def decode_cases():
    """(kind, 256-bit encoding) for ge_frombytes / ge_frombytes_row."""
    rng = random.Random(0xDEC0DE)
    out = []
    for y in (0, 1, 2, P - 1):
        out += [("small_y", y | (s << 255)) for s in (0, 1)]
    for y in range(P, 2**255):  # every non-canonical y, decoding or not
        out += [("noncanonical", y | (s << 255)) for s in (0, 1)]
    out += [("x0_sign1", 1 | (1 << 255)), ("x0_sign1", (P - 1) | (1 << 255))]
    for pt in E.small_order_points():
        e = int.from_bytes(E.encode_point(pt), "little")
        out += [("small_order", e), ("small_order", e ^ (1 << 255))]
    out.append(("base", int.from_bytes(E.encode_point(E.B), "little")))
    want = {"direct": 40, "sqrtm1": 40, None: 40}
    while any(want.values()):
        y = rng.randrange(P)
        k = root_kind(y)
        if want[k]:
            want[k] -= 1
            out.append((k or "off_curve", y | (rng.getrandbits(1) << 255)))
    out += [("random", rng.getrandbits(256)) for _ in range(120)]
    return _finish(out, 12)


# ---- points ---------------------------------------------------------------------------------
PointCase = namedtuple("PointCase", "kind p q neg expected")  # p, q: 4 limb vectors X Y Z T; expected: 32 bytes


def _affine(pt):
    x, y, z, _ = pt
    zi = pow(z, P - 2, P)
    return x * zi % P, y * zi % P


def _projective(pt, z, rng, z_limbs=None):
    """pt with Z scaled to z, each coordinate a random reduced limb vector."""
    x, y = _affine(pt)
    return [redundant(x * z % P, "reduced", rng), redundant(y * z % P, "reduced", rng),
            z_limbs or redundant(z, "reduced", rng), redundant(x * y * z % P, "reduced", rng)]


def _point_sets(rng):
    small = E.small_order_points()
    order = {k: next(p for p in small if E.point_order_small(p) == k) for k in (2, 4, 8)}
    rnd = [E.scalar_mult(rng.randrange(1, L), E.B) for _ in range(4)]
    ps = [("identity", E.IDENTITY), ("base", E.B)] + [("random", r) for r in rnd[:3]] + [("small_order", s) for s in small]
    return ps, order, rnd[3]


def add_cases(z_is_one):
    """P + (neg ? -Q : Q) for ge_p3_to_cached -> ge_cached_cneg -> ge_add -> ge_p1p1_to_p3 -> ge_tobytes.
    z_is_one: Q is given with Z = 1 (limbs 1, 0, ...), else with a random Z != 1; P's Z is always random."""
    rng = random.Random(0xADD + z_is_one)
    ps, order, other = _point_sets(rng)
    out = []
    for pk, p in ps:
        qs = [("same", p), ("negated", E.point_neg(p)), ("identity", E.IDENTITY), ("order2", order[2]),
              ("order4", order[4]), ("order8", order[8]), ("random", other)]
        for qk, q in qs:
            for neg in (0, 1):
                for _ in range(2):
                    zp, zq = rng.randrange(2, P), rng.randrange(2, P)
                    pl = _projective(p, zp, rng)
                    ql = _projective(q, 1, rng, [1] + [0] * 8) if z_is_one else _projective(q, zq, rng)
                    want = E.encode_point(E.point_add(p, E.point_neg(q) if neg else q))
                    out.append(PointCase(f"{pk}+{qk}", pl, ql, neg, want))
    return _finish(out, 13)


def dbl_cases():
    """2P for ge_dbl -> ge_p1p1_to_p3 (X, Y, Z read; Z reduced or lazy)."""
    rng = random.Random(0xDB1)
    ps, _, other = _point_sets(rng)
    ps += [("random", other)] + [("random", E.scalar_mult(rng.randrange(1, L), E.B)) for _ in range(12)]
    out = []
    for pk, p in ps:
        for zcls in ("reduced", "lazy", "one"):
            z = 1 if zcls == "one" else rng.randrange(2, P)
            zl = [1] + [0] * 8 if zcls == "one" else redundant(z, zcls, rng)
            out.append(PointCase(f"{pk}/z {zcls}", _projective(p, z, rng, zl), None, 0, E.encode_point(E.point_add(p, p))))
    return _finish(out, 14)
