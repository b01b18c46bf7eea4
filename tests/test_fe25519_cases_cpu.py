"""The operand sets of tests/fe25519_cases.py (what tests/test_fe25519_lane_gpu.py feeds the compiled
Ed25519 lane code) are what they claim to be: every operand inside the bound of its declared class,
every class pair of the operation table present, the edge families present, and the fold32 set able
to tell a wrong closing step from the right one -- which random canonical operands are not."""
import os
import random
from fractions import Fraction

import ed25519_ref as E
import fe25519_cases as C
from test_generated_asm_fold import Machine, _macro, _value

P = C.P


def _all_field_cases():
    yield "mul", C.mul_cases(False)
    yield "mulf", C.mul_cases(True)
    yield "mul2", [c for pair in C.mul2_cases(False) for c in pair]
    yield "mulf2", [c for pair in C.mul2_cases(True) for c in pair]
    yield "sq", C.sq_cases()
    yield "mul_small", C.mul_small_cases()
    yield "addsub", C.addsub_cases()
    yield "sub_lazy", C.sub_lazy_cases()
    yield "carry", C.carry_cases()
    yield "canon", C.canon_cases()
    yield "inv", C.inv_cases(False)
    yield "inv_wave", C.inv_cases(True)


def test_bounds_are_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "concord-bft_amd", "csrc", "fe25519.h")) as f:
        hdr = f.read()
    for m in C.SUB65P:
        assert f"0x{m:08x}u" in hdr
    assert C.value(C.SUB65P) == 65 * P and C.value(C.SUB256P) == 256 * P
    assert "every limb < 2^29 + 2^17" in hdr and "every limb < 2^30 + 2^18" in hdr
    assert C.REDUCED == 2**29 + 2**17 and C.LAZY == 2**30 + 2**18
    assert C.BOUND["sublazy"] == [C.REDUCED + m for m in C.SUB65P]


def test_every_operand_is_inside_its_declared_class():
    for name, cases in _all_field_cases():
        assert len(cases) % 64 != 0 or name in ("mul2", "mulf2"), name  # (those two are flattened pairs here)
        for c in cases:
            assert len(c.cls) == len(c.operands), name
            for cls, limbs in zip(c.cls, c.operands):
                assert C.in_class(limbs, cls), (name, c.kind, cls, [hex(x) for x in limbs])
    for name, n in (("mul2", len(C.mul2_cases(False))), ("mulf2", len(C.mul2_cases(True)))):
        assert n % 64 != 0, name
    for z1 in (False, True):
        for c in C.add_cases(z1):
            assert all(C.in_class(l, "reduced") for l in c.p + c.q)
            assert not z1 or c.q[2] == [1] + [0] * 8
    for c in C.dbl_cases():
        assert all(C.in_class(l, "reduced") for l in (c.p[0], c.p[1])) and C.in_class(c.p[2], "lazy")


def test_every_class_pair_of_the_table_occurs():
    rl = {"reduced", "lazy"}
    assert {c.cls for c in C.mul_cases(False)} == {(a, b) for a in rl for b in rl}
    fold = {(a, b) for a in rl | {"sublazy"} for b in rl} | {("lazy", "sublazy")}
    assert {c.cls for c in C.mul_cases(True)} == fold and ("sublazy", "sublazy") not in fold
    for f, want in ((False, {(a, b) for a in rl for b in rl}), (True, fold)):
        pairs = C.mul2_cases(f)
        assert {c0.cls for c0, _ in pairs} == want and {c1.cls for _, c1 in pairs} == want
        assert all(c0.cls != c1.cls for c0, c1 in pairs)  # two classes in one statement
    # each pair has its extreme, its zeros, all 81 one-hot positions and each random family
    for f in (False, True):
        by = {}
        for c in C.mul_cases(f):
            by.setdefault(c.cls, []).append(c)
        for cls, cs in by.items():
            kinds = [c.kind for c in cs]
            assert kinds.count("onehot") >= 81 and kinds.count("max") >= 1 and kinds.count("zero") >= 3
            assert {"set", "canonical", "uniform"} <= set(kinds)
            hot = {(next(i for i, x in enumerate(c.operands[0]) if x), next(j for j, x in enumerate(c.operands[1]) if x))
                   for c in cs if c.kind == "onehot"}
            assert len(hot) == 81
            assert any(c.operands == (C.top(cls[0]), C.top(cls[1])) for c in cs)
    assert {c.cls for c in C.sq_cases()} == {("reduced",), ("lazy",)}
    assert {(c.cls, c.extra) for c in C.mul_small_cases()} == {((k,), s) for k in rl for s in C.SMALL}
    assert {c.cls for c in C.addsub_cases()} == {(a, b) for a in rl for b in rl}
    assert {c.cls for c in C.sub_lazy_cases()} == {("reduced", "reduced")}
    assert {c.cls for c in C.inv_cases(False)} == {("reduced",), ("lazy",)} == {c.cls for c in C.inv_cases(True)}
    assert len(C.inv_cases(True)) <= 256
    assert any(c.operands[0] == C.top("wide") for c in C.carry_cases())


def test_canonicalisation_set():
    cases = C.canon_cases()
    assert {c.cls for c in cases} == {("reduced",), ("lazy",), ("sublazy",), ("wide",)}
    zeros = {tuple(c.operands[0]) for c in cases if C.value(c.operands[0]) % P == 0}
    assert len(zeros) >= 3
    assert tuple(C.SUB65P) in zeros and tuple([0] * 9) in zeros  # 65p in fe_sub_lazy's digits, and 0 itself
    vals = {C.value(c.operands[0]) for c in cases if c.kind == "exact"}
    assert vals == set(C.CANON_VALUES)
    for x in C.CANON_VALUES:  # every listed residue in every class
        for cls in ("reduced", "lazy", "sublazy", "wide"):
            assert any(c.kind == "redundant" and c.cls == (cls,) and C.value(c.operands[0]) % P == x % P for c in cases)
    for cls in ("reduced", "lazy", "sublazy", "wide"):
        assert any(c.operands[0] == C.top(cls) for c in cases)
    assert {"sub", "sub_lazy"} <= {c.kind for c in cases}
    assert all(C.value(c.operands[0]) % P == 0 for c in cases if c.kind in ("sub", "sub_lazy"))


def test_from_words_and_inversion_sets():
    xs = set(C.from_words_cases())
    assert {0, P - 1, 2**255 - 1, 2**256 - 1, 2**255} <= xs and set(range(P, 2**255)) <= xs
    assert {x | 2**255 for x in range(P, 2**255)} <= xs
    for wave in (False, True):
        vals = {C.value(c.operands[0]) % P for c in C.inv_cases(wave)}
        assert {0, 1, 2, P - 1, P - 2, E.SQRT_M1} <= vals
        assert any(C.value(c.operands[0]) % P == 0 and c.cls == ("lazy",) and any(c.operands[0]) for c in C.inv_cases(wave))


def test_decode_set():
    cases = C.decode_cases()
    encs = {e for _, e in cases}
    for y in (1, P - 1):  # x = 0 with both sign bits
        assert y in encs and (y | 1 << 255) in encs
        assert E.decode_point(int.to_bytes(y | 1 << 255, 32, "little"))[0] == 0
    for y in list(range(P, 2**255)) + [0, 2]:
        assert y in encs and (y | 1 << 255) in encs
    kinds = [k for k, _ in cases]
    assert kinds.count("direct") >= 40 and kinds.count("sqrtm1") >= 40 and kinds.count("off_curve") >= 40
    for k, e in cases:
        ok = E.decode_point(int.to_bytes(e, 32, "little")) is not None
        if k in ("direct", "sqrtm1", "small_order", "base", "x0_sign1"):
            assert ok
        if k == "off_curve":
            assert not ok
        if k in ("direct", "sqrtm1"):
            assert C.root_kind(e & (2**255 - 1)) == k
    assert sum(E.decode_point(int.to_bytes(e, 32, "little")) is not None for k, e in cases if k == "noncanonical") > 0
    small = {int.from_bytes(E.encode_point(p), "little") for p in E.small_order_points()}
    assert len(small) == 8 and small <= encs


def test_scalar_sets():
    L = C.L
    xs = set(C.sc_canon_cases())
    assert {0, L - 1, L, L + 1, 2**252, 2**256 - 1} <= xs
    for i in range(8):
        assert L + (1 << 32 * i) in xs and L - (1 << 32 * i) in xs
    assert C.MU == int.from_bytes(bytes.fromhex(  # kScMu of sc25519.h, most significant word first
        "0000000f" "ffffffff" "ffffffff" "ffffffff" "ffffffeb" "2106215d" "086329a7" "ed9ce5a3" "0a2c131b"), "big")
    edge = C.sc_reduce_edge_cases()
    need = [C.closing_subtractions(x) for x in edge]
    assert (len(edge), need.count(0), need.count(1), need.count(2)) == (793, 267, 526, 0)
    assert set(edge) <= set(C.sc_reduce_cases())
    assert {C.closing_subtractions(x) for x in C.sc_reduce_cases()} == {0, 1}
    # no input needs 2: the estimate is short of x / L by less than this, which is below 1
    short = (Fraction(2**512, L) + (2**288 - 1) * (Fraction(2**512, L) - C.MU)) / 2**288
    assert short < 1
    rng = random.Random(512)
    assert all(C.closing_subtractions(rng.getrandbits(512)) <= 1 for _ in range(20000))


# ---- the fold32 set against two wrong closing steps ------------------------------------------
def _fold_asm(a, b):
    named = {f"a{i}": a[i] for i in range(9)}
    named.update({f"b{i}": b[i] for i in range(9)})
    named.update(k1216=1216, k9728=9728)
    m = Machine(named)
    m.run(_FOLD_TEXT)
    return [m.named[f"o{i}"] for i in range(9)], m.read("v[20:21]")


def _closing(o, acc, k=1216, high=True):
    """fe_fold32_final; k = 1215 and high = False are the two mutants."""
    w = (acc & 0xFFFFFFFF) * k + o[0]
    o = list(o)
    o[0] = w & C.MASK
    o[1] += (w >> 29) + ((acc >> 32) * 9728 if high else 0)
    return o


_FOLD_TEXT = _macro("CBFT_FE_MULF_ASM")


def _caught(pairs):
    """How many operand pairs expose each mutant (and none may fail the true closing step)."""
    no_high = wrong_k = 0
    for a, b in pairs:
        o, acc = _fold_asm(a, b)
        want = C.value(a) * C.value(b) % P
        assert _value(_closing(o, acc)) % P == want
        no_high += _value(_closing(o, acc, high=False)) % P != want
        wrong_k += _value(_closing(o, acc, k=1215)) % P != want
    return no_high, wrong_k


def test_fold32_set_is_sensitive_to_the_closing_step():
    """Dropping the high-word term of fe_fold32_final, or folding by 1215 for 1216, must give a wrong
    product on the fold32 set.  The contrast: of 3,000 random canonical operand pairs none notices the
    dropped high word (its carry's high word is 0 for them), which is all an end-to-end vector reaches."""
    cases = C.mul_cases(True)
    no_high, wrong_k = _caught(c.operands for c in cases)
    rng = random.Random(3000)
    r_no_high, r_wrong_k = _caught((C.limbs29(rng.randrange(P)), C.limbs29(rng.randrange(P))) for _ in range(3000))
    print(f"fold32 set ({len(cases)} pairs): {no_high} notice the dropped high word, {wrong_k} notice 1215; "
          f"3000 random canonical pairs: {r_no_high} and {r_wrong_k}")
    assert no_high > 0 and wrong_k > 0
    assert r_no_high == 0  # recorded contrast: canonical operands never reach that path
    # every all-limbs-at-bound pair notices both
    for c in cases:
        if c.kind == "max":
            assert _caught([c.operands]) == (1, 1), c.cls
