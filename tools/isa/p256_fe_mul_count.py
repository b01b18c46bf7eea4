#!/usr/bin/env python3
"""Counts, per kernel of an assembly listing (hipcc -S --cuda-device-only), the vector instructions and the
v_mad_u64_u32 among them: the figures of DESIGN.md section 27.2 for tools/isa/p256_fe_mul_probe.hip.

    python3 tools/isa/p256_fe_mul_count.py tools/isa/p256_fe_mul_probe.s
"""
import re
import sys


def count(text):
    parts = re.split(r"^(_Z\w+):\s*(?:;.*)?$", text, flags=re.M)
    out = {}
    for i in range(1, len(parts), 2):
        body = parts[i + 1].split("s_endpgm")[0]
        out[parts[i]] = (len(re.findall(r"^\s+v_", body, re.M)), len(re.findall(r"v_mad_u64_u32", body)))
    return out


if __name__ == "__main__":
    for name, (v, mad) in count(open(sys.argv[1]).read()).items():
        print(f"{name}: {v} vector instructions, {mad} v_mad_u64_u32 ({100 * mad / max(v, 1):.1f} %)")
