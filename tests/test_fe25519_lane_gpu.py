"""The Ed25519 lane code (csrc/fe25519.h with the generated fe25519_asm*.h, sc25519.h, ge25519.h) as
compiled for gfx950, one function per launch through the test-only harness
tests/hip/libfe25519_selftest.so, on the operand sets of tests/fe25519_cases.py: operands at the
bounds the headers state, in every class and aliasing form a function accepts.  Every result must
equal the Python-integer reference exactly, every output limb must lie inside the bound the header
states for that function, and no lane may leave its output unwritten."""
import ctypes
import os

import numpy as np
import pytest

import ed25519_ref as E
import fe25519_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip", "libfe25519_selftest.so")
P = C.P
SENTINEL = 0xA5A5A5A5
# the harness's operation numbers (tests/hip/fe25519_selftest.hip, enum ST_*)
OPS = ("mul_c mul_nc mulf mul2 mulf2 sq_c sq_nc mul_small add sub neg sub_lazy carry canon from_words invert_c "
       "invert_nc invert_var pow_c pow_nc sc_canon sc_reduce frombytes ge_dbl ge_add invert_var_wave "
       "frombytes_row").split()
OP = {name: i for i, name in enumerate(OPS)}
_lib = None


def _library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            pytest.fail("tests/hip/libfe25519_selftest.so not built (make selftest)")
        _lib = ctypes.CDLL(LIB)
    return _lib


def run(op, rows, variant=0):
    """rows: n cases of IN words each -> an (n, OUT) array of what each lane wrote."""
    lib = _library()
    wi, wo, nv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.fe25519_selftest_words(OP[op], ctypes.byref(wi), ctypes.byref(wo), ctypes.byref(nv))
    inp = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
    n = inp.shape[0]
    assert inp.shape == (n, wi.value) and 0 <= variant < nv.value, (op, inp.shape, wi.value, nv.value)
    out = np.zeros((n, wo.value), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.fe25519_selftest(OP[op], variant, ptr(inp), ptr(out), n)
    assert rc == 0, f"{op}/{variant}: HIP error {rc}"
    blank = np.nonzero((out == SENTINEL).all(axis=1))[0]
    assert blank.size == 0, f"{op}/{variant}: lanes {blank[:10]} of {n} wrote nothing"
    return out.astype(object)  # Python integers from here on


def hexl(limbs):
    return "[" + " ".join(f"{int(x):x}" for x in limbs) + "]"


class Report:
    """Collects mismatches; the first ten are printed with the operation, the classes and the operands."""

    def __init__(self, op):
        self.op, self.bad = op, []

    def check(self, ok, what, cls, operands, got):
        if not ok:
            self.bad.append(f"{self.op}: {what}; classes {cls}; operands {' '.join(hexl(o) for o in operands)}; "
                            f"got {hexl(got)}")

    def limbs(self, got, want_value, cls, operands, tight=False):
        """got == want_value (mod p), and reduced: every limb < 2^29 + 2^17; tight (the multiply family's
        outputs): only limb 1 may pass 2^29, by the wrap of the closing carry."""
        self.check(C.value(got) % P == want_value % P, "wrong value", cls, operands, got)
        self.check(C.in_class(got, "reduced"), "limb out of the reduced bound", cls, operands, got)
        if tight:
            self.check(all(x <= C.MASK for k, x in enumerate(got) if k != 1), "limb past 2^29", cls, operands, got)

    def done(self):
        for line in self.bad[:10]:
            print(line)
        assert not self.bad, f"{self.op}: {len(self.bad)} wrong results (first ten above)"


# ---- field products -------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mul_c", "mul_nc", "mulf"])
def test_fe_mul(op):
    """fe_mul<true>, fe_mul<false>, fe_mulf_oneasm: r fresh, r is a, r is b, a is b."""
    cases = C.mul_cases(fold=op == "mulf")
    rows = [c.operands[0] + c.operands[1] for c in cases]
    for variant in range(4):
        rep = Report(f"{op} form {variant}")
        for c, got in zip(cases, run(op, rows, variant)):
            a, b = c.operands
            # a is b: the square of the first operand; fold32 takes sub-lazy against reduced or lazy only
            if variant == 3 and c.cls[0] == "sublazy":
                continue
            rep.limbs(got, C.value(a) * C.value(a if variant == 3 else b), c.cls, c.operands, tight=True)
        rep.done()


@pytest.mark.parametrize("op", ["mul2", "mulf2"])
def test_fe_mul2(op):
    """fe_mul2_oneasm, fe_mulf2_oneasm: fresh results; r0 is a1 and r1 is b0; r0 is a0 and r1 is a1.  The two
    products of a statement have different operand classes."""
    pairs = C.mul2_cases(fold=op == "mulf2")
    rows = [c0.operands[0] + c0.operands[1] + c1.operands[0] + c1.operands[1] for c0, c1 in pairs]
    for variant in range(3):
        rep = Report(f"{op} form {variant}")
        for (c0, c1), got in zip(pairs, run(op, rows, variant)):
            ops = c0.operands + c1.operands
            cls = c0.cls + c1.cls
            rep.limbs(got[:9], C.value(c0.operands[0]) * C.value(c0.operands[1]), cls, ops, tight=True)
            rep.limbs(got[9:], C.value(c1.operands[0]) * C.value(c1.operands[1]), cls, ops, tight=True)
        rep.done()


@pytest.mark.parametrize("op", ["sq_c", "sq_nc"])
def test_fe_sq(op):
    cases = C.sq_cases()
    rows = [c.operands[0] for c in cases]
    for variant in range(2):
        rep = Report(f"{op} form {variant}")
        for c, got in zip(cases, run(op, rows, variant)):
            rep.limbs(got, C.value(c.operands[0]) ** 2, c.cls, c.operands, tight=True)
        rep.done()


def test_fe_mul_small():
    cases = C.mul_small_cases()
    rows = [c.operands[0] + [c.extra] for c in cases]
    for variant in range(2):
        rep = Report(f"mul_small form {variant}")
        for c, got in zip(cases, run("mul_small", rows, variant)):
            rep.limbs(got, C.value(c.operands[0]) * c.extra, c.cls + (c.extra,), c.operands, tight=True)
        rep.done()


# ---- additions, subtractions, carry ----------------------------------------------------------
def test_fe_add_sub_neg():
    """fe_add: the limb-wise sum, nothing else.  fe_sub, fe_neg: the value, reduced."""
    cases = C.addsub_cases()
    rows = [c.operands[0] + c.operands[1] for c in cases]
    for variant in range(2):
        rep = Report(f"add form {variant}")
        for c, got in zip(cases, run("add", rows, variant)):
            a, b = c.operands
            rep.check(list(got) == [x + y for x, y in zip(a, b)], "not the limb-wise sum", c.cls, c.operands, got)
        rep.done()
        rep = Report(f"sub form {variant}")
        for c, got in zip(cases, run("sub", rows, variant)):
            a, b = c.operands
            rep.limbs(got, C.value(a) - C.value(b), c.cls, c.operands)
            rep.check(list(got) == C.model_sub(a, b), "not a + 256p - b, carried once", c.cls, c.operands, got)
        rep.done()
        rep = Report(f"neg form {variant}")
        for c, got in zip(cases, run("neg", [c.operands[0] for c in cases], variant)):
            rep.limbs(got, -C.value(c.operands[0]), c.cls[:1], c.operands[:1])
        rep.done()


def test_fe_sub_lazy():
    """reduced - reduced: limb i = a_i + digit i of 65p - b_i exactly (no wrap), below reduced + that digit."""
    cases = C.sub_lazy_cases()
    rows = [c.operands[0] + c.operands[1] for c in cases]
    for variant in range(2):
        rep = Report(f"sub_lazy form {variant}")
        for c, got in zip(cases, run("sub_lazy", rows, variant)):
            a, b = c.operands
            rep.check(C.value(got) % P == (C.value(a) - C.value(b)) % P, "wrong value", c.cls, c.operands, got)
            rep.check(C.in_class(got, "sublazy"), "limb out of the sub-lazy bound", c.cls, c.operands, got)
            rep.check(list(got) == C.model_sub_lazy(a, b), "not a + 65p - b by limbs", c.cls, c.operands, got)
        rep.done()


def test_fe_carry():
    cases = C.carry_cases()
    rep = Report("carry")
    for c, got in zip(cases, run("carry", [c.operands[0] for c in cases])):
        rep.limbs(got, C.value(c.operands[0]), c.cls, c.operands)
        rep.check(list(got) == C.model_carry(c.operands[0]), "not one carry pass", c.cls, c.operands, got)
    rep.done()


# ---- canonical form -------------------------------------------------------------------------
def test_fe_to_words_iszero_isnegative():
    cases = C.canon_cases()
    rep = Report("to_words / iszero / isnegative")
    for c, got in zip(cases, run("canon", [c.operands[0] for c in cases])):
        x = C.value(c.operands[0]) % P
        rep.check(C.from_words(got[:8]) == x, f"fe_to_words != {x:x} ({c.kind})", c.cls, c.operands, got[:8])
        rep.check(got[8] == (1 if x == 0 else 0), f"fe_iszero of {x:x} ({c.kind})", c.cls, c.operands, got[8:9])
        rep.check(got[9] == (x & 1), f"fe_isnegative of {x:x} ({c.kind})", c.cls, c.operands, got[9:10])
    rep.done()


def test_fe_from_words():
    """The low 255 bits exactly, as 29-bit digits: not reduced mod p."""
    xs = C.from_words_cases()
    rep = Report("from_words")
    for x, got in zip(xs, run("from_words", [C.words(x, 8) for x in xs])):
        rep.check(list(got) == C.limbs29(x & (2**255 - 1)), "not the low 255 bits", ("words",), [C.words(x, 8)], got)
    rep.done()


# ---- inversion and the square-root power ------------------------------------------------------
@pytest.mark.parametrize("op", ["invert_c", "invert_nc", "invert_var", "pow_c", "pow_nc"])
def test_fe_invert_pow22523(op):
    cases = C.inv_cases()
    rep = Report(op)
    e = (P - 5) // 8 if op.startswith("pow") else P - 2  # pow(0, p - 2, p) == 0: 0 -> 0
    for c, got in zip(cases, run(op, [c.operands[0] for c in cases])):
        want = pow(C.value(c.operands[0]) % P, e, P)
        rep.limbs(got, want, c.cls, c.operands, tight=True)
        if op == "invert_var":  # through fe_from_words: the canonical digits
            rep.check(list(got) == C.limbs29(want), "not canonical", c.cls, c.operands, got)
    rep.done()


def test_fe_invert_var_wave():
    """fe_invert_var<true>: a full wave per value, every lane the same input and the same, canonical, result."""
    cases = C.inv_cases(wave=True)
    rep = Report("invert_var_wave")
    for c, got in zip(cases, run("invert_var_wave", [c.operands[0] for c in cases])):
        want = C.limbs29(pow(C.value(c.operands[0]) % P, P - 2, P))
        lanes = [list(got[9 * k:9 * k + 9]) for k in range(64)]
        rep.check(all(l == lanes[0] for l in lanes), "lanes differ", c.cls, c.operands, sum(lanes[:2], []))
        rep.check(lanes[0] == want, "wrong inverse", c.cls, c.operands, lanes[0])
    rep.done()


# ---- scalars --------------------------------------------------------------------------------
def test_sc_is_canonical():
    xs = C.sc_canon_cases()
    rep = Report("sc_is_canonical")
    for x, got in zip(xs, run("sc_canon", [C.words(x, 8) for x in xs])):
        rep.check(got[0] == (1 if x < C.L else 0), "wrong verdict", ("words",), [C.words(x, 8)], got)
    rep.done()


def test_sc_reduce512():
    xs = C.sc_reduce_cases()
    rep = Report("sc_reduce512")
    for x, got in zip(xs, run("sc_reduce", [C.words(x, 16) for x in xs])):
        rep.check(C.from_words(got) == x % C.L, f"closing subtractions needed: {C.closing_subtractions(x)}", ("words",),
                  [C.words(x, 16)], got)
    rep.done()


# ---- decoding -------------------------------------------------------------------------------
def test_ge_frombytes_and_row():
    """ge_frombytes and ge_frombytes_row<false> against ed25519_ref.decode_point and each other: the ok flag
    always; X, Y (mod p) and T == XY when ok; all 16 lanes of a row the same."""
    cases = C.decode_cases()
    rows = [C.words(e, 8) for _, e in cases]
    lane, row = run("frombytes", rows), run("frombytes_row", rows)
    rep = Report("frombytes")
    for (kind, e), w, g, r in zip(cases, rows, lane, row):
        pt = E.decode_point(int.to_bytes(e, 32, "little"))
        lanes = [list(r[19 * k:19 * k + 19]) for k in range(16)]
        rep.check(all(l == lanes[0] for l in lanes), f"row lanes differ ({kind})", ("words",), [w], sum(lanes[:2], []))
        r = lanes[0]
        rep.check(g[0] == (pt is not None), f"ge_frombytes ok flag ({kind})", ("words",), [w], g[:1])
        rep.check(r[0] == (pt is not None), f"ge_frombytes_row ok flag ({kind})", ("words",), [w], r[:1])
        y_limbs = C.limbs29(e & (2**255 - 1))
        rep.check(list(g[10:19]) == y_limbs and r[10:19] == y_limbs, f"Y is not the low 255 bits ({kind})", ("words",), [w],
                  g[10:19])
        if pt is None:
            continue
        X, Y, T = g[1:10], g[10:19], g[19:28]
        rep.limbs(X, pt[0], (kind,), [w])
        rep.limbs(r[1:10], pt[0], (kind + " (row)",), [w])
        rep.check(C.value(Y) % P == pt[1], f"wrong y ({kind})", ("words",), [w], Y)
        rep.limbs(T, pt[0] * pt[1], (kind + " T",), [w], tight=True)
    rep.done()


# ---- point arithmetic -----------------------------------------------------------------------
def _check_p3(rep, c, got):
    X, Y, Z, T = (list(got[9 * k:9 * k + 9]) for k in range(4))
    ops = c.p + (c.q or [])
    for name, l in zip("XYZT", (X, Y, Z, T)):
        rep.check(C.in_class(l, "reduced") and all(x <= C.MASK for k, x in enumerate(l) if k != 1),
                  f"{name} limb out of bound ({c.kind})", ("neg", c.neg), ops, l)
    x, y, z, t = (C.value(l) % P for l in (X, Y, Z, T))
    rep.check(z != 0 and E.encode_point((x, y, z, t)) == c.expected, f"wrong point ({c.kind})", ("neg", c.neg), ops, X + Y + Z)
    rep.check(t * z % P == x * y % P, f"T Z != X Y ({c.kind})", ("neg", c.neg), ops, T)
    rep.check(int.to_bytes(C.from_words(got[36:44]), 32, "little") == c.expected,
              f"ge_tobytes != {c.expected.hex()} ({c.kind})", ("neg", c.neg), ops, got[36:44])


def test_ge_dbl():
    cases = C.dbl_cases()
    rep = Report("ge_dbl")
    for c, got in zip(cases, run("ge_dbl", [c.p[0] + c.p[1] + c.p[2] for c in cases])):
        _check_p3(rep, c, got)
    rep.done()


@pytest.mark.parametrize("z_is_one", [0, 1])
def test_ge_add(z_is_one):
    cases = C.add_cases(z_is_one)
    rep = Report(f"ge_add zIsOne={z_is_one}")
    for c, got in zip(cases, run("ge_add", [sum(c.p, []) + sum(c.q, []) + [c.neg] for c in cases], z_is_one)):
        _check_p3(rep, c, got)
    rep.done()
