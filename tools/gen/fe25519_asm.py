#!/usr/bin/env python3
"""Generate the one-statement GF(2^255-19) multiply / square texts (radix 2^29 x 9, column sums of
fe25519.h's fe_mul / fe_sq, same mads in the same order).

  python3 tools/gen/fe25519_asm.py        > concord-bft_amd/csrc/fe25519_asm.h
  python3 tools/gen/fe25519_asm.py multi  > concord-bft_amd/csrc/fe25519_asm_multi.h
  python3 tools/gen/fe25519_asm.py fold32 > concord-bft_amd/csrc/fe25519_asm_fold32.h

Why one statement: the compiler cannot see inside inline asm, so it puts an s_nop between an asm
statement and any instruction right after it that reads the statement's results; the
column-per-statement form pays that at each of the 17 columns.  The accumulator lives in the
fixed pair v[20:21] so the text can name its low half for the digit split.

`multi`: N independent products in ONE statement, their instruction streams interleaved column by
column (product p's accumulator in v[20+2p : 21+2p]): the same mads and splits as N single
products, but every mad, digit split and carry shift of product p is followed by the next
product's independent one instead of by its own dependent successor, so a wave always has an
independent instruction ready.  Emitted as C++ wrappers fe_mul{N}_oneasm(r0, a0, b0, ...) for
N in MULTI: the pair ladder uses N = 2 (N = 3 and 4 measured slower, tools/probes/r06_ab2.sh)."""
import sys

MULTI = (2,)


def products(k, sq):
    lo = 0 if k < 9 else k - 8
    hi = k if k < 9 else 8
    if not sq:
        return [(f"a{i}", f"b{k - i}") for i in range(lo, hi + 1)]
    out = []
    i = lo
    while 2 * i < k:
        out.append((f"d{i}", f"a{k - i}"))  # d = 2a
        i += 1
    if k % 2 == 0:
        out.append((f"a{k // 2}", f"a{k // 2}"))
    return out


def steps(sq):
    """The single product's instruction sequence as abstract steps:
    ("mad", x, y, first) | ("split", digit) | ("movtop",)."""
    out = []
    for k in range(9, 17):  # high columns -> h0..h7 and the top h8 (weight 2^261 == 1216)
        out += [("mad", x, y, k == 9 and n == 0) for n, (x, y) in enumerate(products(k, sq))]
        out.append(("split", f"h{k - 9}"))
    out.append(("movtop",))
    for k in range(9):  # low columns, each chain led by its fold term h_k * 1216
        out.append(("mad", f"h{k}", "k1216", k == 0))
        out += [("mad", x, y, False) for x, y in products(k, sq)]
        out.append(("split", f"o{k}"))
    return out


def render(step, p=None):
    """asm line(s) of one step; p = None: the single form's operand names, else product p's."""
    acc = "v[20:21]" if p is None else f"v[{20 + 2 * p}:{21 + 2 * p}]"
    lo = "v20" if p is None else f"v{20 + 2 * p}"
    nm = (lambda s: s) if p is None else (lambda s: s if s == "k1216" else f"{s[0]}{p}_{s[1:]}")
    if step[0] == "mad":
        _, x, y, first = step
        return [f"v_mad_u64_u32 {acc}, %[cc], %[{nm(x)}], %[{nm(y)}], {'0' if first else acc}"]
    if step[0] == "split":
        return [f"v_and_b32 %[{nm(step[1])}], 0x1fffffff, {lo}", f"v_lshrrev_b64 {acc}, 29, {acc}"]
    return [f"v_mov_b32 %[{nm('h8')}], {lo}"]


def text(sq):
    lines = []
    for st in steps(sq):
        lines += render(st)
    return "\\n\\t".join(lines)


def multi_text(n):
    """n products interleaved step by step (every product has the same step sequence)."""
    seq = steps(False)
    lines = []
    for st in seq:
        if st[0] == "split":  # all digit ands first, then the shifts: each shift is then n - 1
            ands = [render(st, p)[0] for p in range(n)]  # instructions away from its product's and
            shifts = [render(st, p)[1] for p in range(n)]
            lines += ands + shifts
        else:
            for p in range(n):
                lines += render(st, p)
    return "\\n\\t".join(lines)


def multi_wrapper(n):
    args = ", ".join(f"fe& r{p}, const fe& a{p}, const fe& b{p}" for p in range(n))
    outs = ["[cc] \"=s\"(cc)"]
    for p in range(n):
        outs.append(f"\"=&{{v[{20 + 2 * p}:{21 + 2 * p}]}}\"(acc{p})")
        outs += [f"[o{p}_{k}] \"=&v\"(o{p}.v[{k}])" for k in range(9)]
        outs += [f"[h{p}_{k}] \"=&v\"(h{p}[{k}])" for k in range(9)]
    ins = []
    for p in range(n):
        ins += [f"[a{p}_{k}] \"v\"(a{p}.v[{k}])" for k in range(9)]
        ins += [f"[b{p}_{k}] \"v\"(b{p}.v[{k}])" for k in range(9)]
    ins.append("[k1216] \"v\"(1216u)")
    decl = "  fe " + ", ".join(f"o{p}" for p in range(n)) + ";\n"
    decl += "  uint32_t " + ", ".join(f"h{p}[9]" for p in range(n)) + ";\n"
    decl += "  uint64_t cc, " + ", ".join(f"acc{p}" for p in range(n)) + ";\n"
    body = f"  asm(CBFT_FE_MUL{n}_ASM\n      : " + ",\n        ".join(outs) + "\n      : " + ",\n        ".join(ins) + ");\n"
    fin = "".join(f"  fe_oneasm_final(r{p}, o{p}, acc{p});\n" for p in range(n))
    return (f"// r_p = a_p * b_p for p < {n} (any r_p may alias any input)\n"
            f"FE_INLINE void fe_mul{n}_oneasm({args}) {{\n{decl}{body}{fin}}}\n")


# ---- fold32: the multiply with the high columns folded on dword boundaries ----------------------
# Every high column k = 9..16 accumulates into its own 64-bit pair H_(k-9) (no carry between them, no
# digit split); the pair's register halves then enter the low columns directly:
#   lo32(H_j) * 1216 -> column j        (2^(261 + 29 j) == 1216 * 2^(29 j))
#   hi32(H_j) * 9728 -> column j + 1    (2^32 = 8 * 2^29, 8 * 1216 = 9728)
# 81 + 16 mads, 9 + 9 split instructions, no move: 115 instructions against 125.  The pairs are
# pinned (single form: accumulator v[20:21], H_j in v[24+2j : 25+2j]; product p of the interleaved
# form: accumulator v[20+2p : 21+2p], H_j in v[24+16p+2j : 25+16p+2j]) so the text can name the halves.
FOLD_MULTI = (2,)


def fold_regs(p):
    """(accumulator pair base, [H_j pair bases]) of product p (p = None: the single form = product 0)."""
    p = p or 0
    return 20 + 2 * p, [24 + 16 * p + 2 * j for j in range(8)]


def fold_steps():
    """("mad", dst, x, y, first) with dst "acc" or "H<j>" | ("split", digit); x / y are operand names,
    "H<j>.lo" / "H<j>.hi" for a pair's halves, "k1216" / "k9728" for the fold constants."""
    out = []
    for k in range(9, 17):
        out += [("mad", f"H{k - 9}", x, y, n == 0) for n, (x, y) in enumerate(products(k, False))]
    for k in range(9):
        if k < 8:
            out.append(("mad", "acc", f"H{k}.lo", "k1216", k == 0))
        if k > 0:
            out.append(("mad", "acc", f"H{k - 1}.hi", "k9728", False))
        out += [("mad", "acc", x, y, False) for x, y in products(k, False)]
        out.append(("split", f"o{k}"))
    return out


def fold_render(step, p=None):
    accb, hb = fold_regs(p)

    def pair(name):
        b = accb if name == "acc" else hb[int(name[1])]
        return f"v[{b}:{b + 1}]"

    def src(s):
        if s[0] == "H":
            return f"v{hb[int(s[1])] + (s.endswith('.hi'))}"
        if s[0] == "k" or p is None:
            return f"%[{s}]"
        return f"%[{s[0]}{p}_{s[1:]}]"

    if step[0] == "mad":
        _, dst, x, y, first = step
        return [f"v_mad_u64_u32 {pair(dst)}, %[cc], {src(x)}, {src(y)}, {'0' if first else pair(dst)}"]
    return [f"v_and_b32 {src(step[1])}, 0x1fffffff, v{accb}", f"v_lshrrev_b64 {pair('acc')}, 29, {pair('acc')}"]


def fold_text(n=None):
    """n = None: the single form; else n products interleaved step by step like multi_text."""
    lines = []
    for st in fold_steps():
        if n is None:
            lines += fold_render(st)
        elif st[0] == "split":
            lines += [fold_render(st, p)[0] for p in range(n)] + [fold_render(st, p)[1] for p in range(n)]
        else:
            for p in range(n):
                lines += fold_render(st, p)
    return "\\n\\t".join(lines)


def fold_wrapper(n):
    """n = None: fe_mulf_oneasm(r, a, b); else fe_mulf{n}_oneasm(r0, a0, b0, ...)."""
    ps = [None] if n is None else list(range(n))
    sfx = (lambda p: "" if p is None else str(p))
    nm = (lambda p, s, k: f"{s}{k}" if p is None else f"{s}{p}_{k}")
    args = ", ".join(f"fe& r{sfx(p)}, const fe& a{sfx(p)}, const fe& b{sfx(p)}" for p in ps)
    outs, ins, clob = ["[cc] \"=s\"(cc)"], [], []
    for p in ps:
        accb, hb = fold_regs(p)
        outs.append(f"\"=&{{v[{accb}:{accb + 1}]}}\"(acc{sfx(p)})")
        outs += [f"[{nm(p, 'o', k)}] \"=&v\"(o{sfx(p)}.v[{k}])" for k in range(9)]
        ins += [f"[{nm(p, 'a', k)}] \"v\"(a{sfx(p)}.v[{k}])" for k in range(9)]
        ins += [f"[{nm(p, 'b', k)}] \"v\"(b{sfx(p)}.v[{k}])" for k in range(9)]
        clob += [f"\"v{b + h}\"" for b in hb for h in (0, 1)]
    ins += ["[k1216] \"s\"(1216u)", "[k9728] \"s\"(9728u)"]
    decl = "  fe " + ", ".join(f"o{sfx(p)}" for p in ps) + ";\n"
    decl += "  uint64_t cc, " + ", ".join(f"acc{sfx(p)}" for p in ps) + ";\n"
    macro = "CBFT_FE_MULF_ASM" if n is None else f"CBFT_FE_MULF{n}_ASM"
    clob_lines = [", ".join(clob[i:i + 16]) for i in range(0, len(clob), 16)]
    body = (f"  asm({macro}\n      : " + ",\n        ".join(outs) + "\n      : " + ",\n        ".join(ins) +
            "\n      : " + ",\n        ".join(clob_lines) + ");\n")
    fin = "".join(f"  fe_fold32_final(r{sfx(p)}, o{sfx(p)}, acc{sfx(p)});\n" for p in ps)
    what = "r = a * b (r may alias a or b)" if n is None else f"r_p = a_p * b_p for p < {n} (any r_p may alias any input)"
    name = "fe_mulf_oneasm" if n is None else f"fe_mulf{n}_oneasm"
    return f"// {what}\nFE_INLINE void {name}({args}) {{\n{decl}{body}{fin}}}\n"


if len(sys.argv) > 1 and sys.argv[1] == "fold32":
    print("// Generated by tools/gen/fe25519_asm.py fold32 -- do not edit.")
    print("// Included by fe25519.h after fe, FE_INLINE and fe_fold32_final.")
    print("#pragma once")
    print(f'#define CBFT_FE_MULF_ASM "{fold_text()}"')
    for n in FOLD_MULTI:
        print(f'#define CBFT_FE_MULF{n}_ASM "{fold_text(n)}"')
    print(fold_wrapper(None))
    for n in FOLD_MULTI:
        print(fold_wrapper(n))
elif len(sys.argv) > 1 and sys.argv[1] == "multi":
    print("// Generated by tools/gen/fe25519_asm.py multi -- do not edit.")
    print("// Included by fe25519.h after fe, FE_INLINE and fe_oneasm_final.")
    print("#pragma once")
    for n in MULTI:
        print(f'#define CBFT_FE_MUL{n}_ASM "{multi_text(n)}"')
    for n in MULTI:
        print(multi_wrapper(n))
else:
    print("// Generated by tools/gen/fe25519_asm.py -- do not edit.")
    print("#pragma once")
    print(f'#define CBFT_FE_MUL_ASM "{text(False)}"')
    print(f'#define CBFT_FE_SQ_ASM "{text(True)}"')
