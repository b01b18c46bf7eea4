"""The fold32 field multiply (concord-bft_amd/csrc/fe25519_asm_fold32.h, tools/gen/fe25519_asm.py fold32):
the committed header is the generator's output, and the emitted text, run by a small exact-integer
interpreter, never overflows a 64-bit accumulator, returns a * b mod 2^255 - 19 and leaves every limb
"reduced", for random operands and for the extreme operands of the pair ladder's bound table
(fe25519.h: reduced < 2^29 + 2^17, lazy = 2 reduced, sub-lazy = reduced + the digits of 65p)."""
import random
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "concord-bft_amd" / "csrc"
P = 2**255 - 19
MASK = 2**29 - 1
REDUCED = 2**29 + 2**17          # exclusive bound of every limb of a reduced element
LAZY = 2 * REDUCED               # sum of two reduced
SUB65P = [2**30 - 1235] + [2**30 - 2] * 7 + [2**29 + 2**23 - 2]  # fe_sub_lazy's multiple of p, by digit
SUBLAZY = [REDUCED + m for m in SUB65P]  # reduced + 65p - reduced, exclusive per-limb bound


def _header_text():
    return (CSRC / "fe25519_asm_fold32.h").read_text()


def _macro(name):
    m = re.search(r'#define %s "([^"]*)"' % name, _header_text())
    assert m, name
    return m.group(1).split("\\n\\t")


def test_fold_header_is_generator_output():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen" / "fe25519_asm.py"), "fold32"], check=True,
                         capture_output=True, text=True).stdout
    assert out == _header_text()


def test_generated_headers_are_all_current():
    """Every generated fe25519_asm*.h under csrc comes from a generator mode (no stale header)."""
    modes = {"fe25519_asm.h": [], "fe25519_asm_multi.h": ["multi"], "fe25519_asm_fold32.h": ["fold32"]}
    assert {p.name for p in CSRC.glob("fe25519_asm*.h")} == set(modes)
    for name, argv in modes.items():
        out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen" / "fe25519_asm.py"), *argv], check=True,
                             capture_output=True, text=True).stdout
        assert out == (CSRC / name).read_text(), name


def test_sub65p_is_a_multiple_of_p_above_reduced():
    assert sum(m << (29 * i) for i, m in enumerate(SUB65P)) == 65 * P
    assert all(m >= REDUCED for m in SUB65P)  # no limb of a - b + 65p underflows for reduced b
    hdr = (CSRC / "fe25519.h").read_text()
    for m in SUB65P:
        assert f"0x{m:08x}u" in hdr  # fe_sub_lazy adds exactly these digits


# ---- the interpreter: v_mad_u64_u32, v_and_b32, v_lshrrev_b64, v_mov_b32 over exact integers ----
PAIR = re.compile(r"^v\[(\d+):(\d+)\]$")


class Machine:
    def __init__(self, named):
        self.v = {}            # physical VGPRs, 32 bits each
        self.named = dict(named)  # %[name] operands, 32 bits each
        self.peak = 0          # largest 64-bit intermediate seen

    def read(self, s):
        if s.startswith("%["):
            return self.named[s[2:-1]]
        if s.startswith("0x"):
            return int(s, 16)
        if s.isdigit():
            return int(s)
        m = PAIR.match(s)
        if m:
            lo, hi = int(m.group(1)), int(m.group(2))
            assert hi == lo + 1 and lo % 2 == 0, s  # gfx950 wants even-aligned 64-bit pairs
            return self.v[lo] | (self.v[hi] << 32)
        assert re.match(r"^v\d+$", s), s
        return self.v[int(s[1:])]  # a pair's half: v<2n> low, v<2n+1> high

    def write(self, s, val):
        m = PAIR.match(s)
        if m:
            assert 0 <= val < 2**64, (s, val)
            self.peak = max(self.peak, val)
            self.v[int(m.group(1))], self.v[int(m.group(2))] = val & 0xFFFFFFFF, val >> 32
        elif s.startswith("%["):
            assert 0 <= val < 2**32
            self.named[s[2:-1]] = val
        else:
            assert 0 <= val < 2**32
            self.v[int(s[1:])] = val

    def run(self, lines):
        for l in lines:
            op, rest = l.split(None, 1)
            a = [x.strip() for x in re.split(r",\s*(?![^\[]*\])", rest)]
            if op == "v_mad_u64_u32":
                dst, cc, x, y, z = a
                assert cc == "%[cc]"
                for s in (x, y):
                    assert not PAIR.match(s), l  # 32-bit factors
                self.write(dst, self.read(x) * self.read(y) + self.read(z))  # write asserts < 2^64
            elif op == "v_and_b32":
                self.write(a[0], self.read(a[1]) & self.read(a[2]))
            elif op == "v_lshrrev_b64":
                self.write(a[0], self.read(a[2]) >> self.read(a[1]))
            elif op == "v_mov_b32":
                self.write(a[0], self.read(a[1]))
            else:
                raise AssertionError(f"unknown instruction {l}")


def _value(limbs):
    return sum(x << (29 * i) for i, x in enumerate(limbs))


def _final(o, acc):
    """fe_fold32_final: the carry out of column 8 (weight 2^261 == 1216) wraps by words, the low
    word * 1216 into limbs 0 and 1, the high word (weight 2^293 == 9728 * 2^29) into limb 1."""
    assert acc < 2**35
    w = (acc & 0xFFFFFFFF) * 1216 + o[0]
    o = list(o)
    o[0] = w & MASK
    o[1] += (w >> 29) + (acc >> 32) * 9728
    return o


def _run_single(a, b):
    named = {f"a{i}": a[i] for i in range(9)}
    named.update({f"b{i}": b[i] for i in range(9)})
    named.update(k1216=1216, k9728=9728)
    m = Machine(named)
    m.run(_macro("CBFT_FE_MULF_ASM"))
    return _final([m.named[f"o{i}"] for i in range(9)], m.read("v[20:21]")), m.peak


def _check(a, b):
    o, peak = _run_single(a, b)
    assert _value(o) % P == (_value(a) * _value(b)) % P
    assert all(x < REDUCED for x in o), o
    return peak


def _extremes():
    """The operand bounds of every product of the pair ladder's addition step (the bound table in
    fe25519.h / DESIGN): the worst is sub-lazy x lazy (T' = t.X * t.Y)."""
    red, lazy = [REDUCED - 1] * 9, [LAZY - 1] * 9
    sub = [s - 1 for s in SUBLAZY]
    return {"lazy*reduced": (lazy, red), "sublazy*reduced": (sub, red), "reduced*reduced": (red, red),
            "sublazy*lazy": (sub, lazy), "lazy*sublazy": (lazy, sub), "lazy*lazy": (lazy, lazy)}


@pytest.mark.parametrize("name", sorted(_extremes()))
def test_fold_multiply_extreme_operands(name):
    a, b = _extremes()[name]
    peak = _check(a, b)
    assert peak < 2**64
    zero = [0] * 9
    _check(zero, b)
    _check(a, zero)
    _check(zero, zero)
    for i in range(9):  # one-hot limbs at their maximum, every pair of positions
        for j in range(9):
            _check([a[k] if k == i else 0 for k in range(9)], [b[k] if k == j else 0 for k in range(9)])


def test_fold_multiply_random_operands():
    rng = random.Random(25519)
    sub = SUBLAZY
    for _ in range(200):
        kind = rng.randrange(3)
        a = [rng.randrange(sub[i]) if kind == 0 else rng.randrange(LAZY) if kind == 1 else rng.randrange(2**29)
             for i in range(9)]
        b = [rng.randrange(LAZY) for _ in range(9)]
        _check(a, b)


def _count(lines):
    mads = [l for l in lines if l.startswith("v_mad_u64_u32")]
    f1216 = [l for l in mads if "%[k1216]" in l]
    f9728 = [l for l in mads if "%[k9728]" in l]
    ands = [l for l in lines if l.startswith("v_and_b32")]
    shifts = [l for l in lines if l.startswith("v_lshrrev_b64")]
    return len(mads) - len(f1216) - len(f9728), len(f1216), len(f9728), len(ands), len(shifts), len(lines)


def test_fold_text_shape():
    # 81 products, 8 + 8 fold mads, one digit split per LOW column only, no move: 115 instructions
    assert _count(_macro("CBFT_FE_MULF_ASM")) == (81, 8, 8, 9, 9, 115)


def test_fold_multi_text_is_two_interleaved_products():
    """fe_mulf2_oneasm: two copies of the single form (product 0 in the single form's registers,
    product 1 in its own accumulator and H pairs), every (a_i, b_j) once each, the streams alternating;
    and the interleaved text computes both products."""
    lines = _macro("CBFT_FE_MULF2_ASM")
    single = _macro("CBFT_FE_MULF_ASM")
    assert len(lines) == 2 * len(single)

    def rename(l, p):  # the single form's line as product p's
        l = re.sub(r"%\[([abo])(\d)\]", lambda m: f"%[{m.group(1)}{p}_{m.group(2)}]", l)
        return re.sub(r"v(\[?)(\d+)(?::(\d+)\])?", lambda m: _shift_reg(m, p), l)

    def _shift_reg(m, p):
        r = int(m.group(2))
        r = r + 2 * p if r < 24 else r + 16 * p
        return f"v[{r}:{r + 1}]" if m.group(1) else f"v{r}"

    for p in (0, 1):
        want = [rename(l, p) for l in single]
        accs = {"v[%d:%d]" % (20 + 2 * p, 21 + 2 * p)} | {"v[%d:%d]" % (b, b + 1) for b in range(24 + 16 * p, 40 + 16 * p, 2)}
        mine = [l for l in lines if (l.split()[1].rstrip(",") in accs) or
                (l.startswith("v_and_b32") and l.endswith(f"v{20 + 2 * p}"))]
        assert sorted(mine) == sorted(want)
        pairs = set()
        for l in mine:
            mm = re.match(r"v_mad_u64_u32 v\[\d+:\d+\], %\[cc\], %\[a{0}_(\d)\], %\[b{0}_(\d)\]".format(p), l)
            if mm:
                pairs.add((int(mm.group(1)), int(mm.group(2))))
        assert pairs == {(i, j) for i in range(9) for j in range(9)}
    mad_dsts = [l.split(",")[0].split()[-1] for l in lines if l.startswith("v_mad_u64_u32")]
    owner = lambda d: 0 if int(d[2:d.index(":")]) in (20, *range(24, 40)) else 1
    assert all(owner(x) != owner(y) for x, y in zip(mad_dsts, mad_dsts[1:]))
    # and it computes: two different extreme products at once
    ex = _extremes()
    (a0, b0), (a1, b1) = ex["sublazy*lazy"], ex["lazy*reduced"]
    named = {"k1216": 1216, "k9728": 9728}
    for p, (a, b) in enumerate(((a0, b0), (a1, b1))):
        named.update({f"a{p}_{i}": a[i] for i in range(9)})
        named.update({f"b{p}_{i}": b[i] for i in range(9)})
    m = Machine(named)
    m.run(lines)
    for p, (a, b) in enumerate(((a0, b0), (a1, b1))):
        o = _final([m.named[f"o{p}_{i}"] for i in range(9)], m.read(f"v[{20 + 2 * p}:{21 + 2 * p}]"))
        assert _value(o) % P == (_value(a) * _value(b)) % P
        assert all(x < REDUCED for x in o)
