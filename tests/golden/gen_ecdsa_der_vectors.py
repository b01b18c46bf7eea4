#!/usr/bin/env python3
"""Generates tests/golden/ecdsa_der_vectors.json: DER-encoded ECDSA P-256 signatures, canonical and damaged,
each with OpenSSL's ECDSA_verify verdict (the entry point that takes DER; 1 is accept, anything else is
reject).  Asserts that tests/p256_ref.py (der_to_rs, then verify) agrees on every vector.  Deterministic.

    python3 tests/golden/gen_ecdsa_der_vectors.py

File: {"vectors": [{"cls", "key" (hex X || Y), "msg" (hex), "der" (hex), "canonical" (0 | 1), "ok"}]}.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import p256_ref as ref  # noqa: E402
from gen_ecdsa_p256_vectors import openssl_der_verdict  # noqa: E402

N, G = ref.N, ref.G


def der_int(body: bytes) -> bytes:
    return b"\x02" + bytes([len(body)]) + body


def minimal(v: int) -> bytes:
    return v.to_bytes(max(1, (v.bit_length() + 8) // 8), "big")


def seq(body: bytes) -> bytes:
    return b"\x30" + bytes([len(body)]) + body


def main():
    rng = random.Random(0xDE256)
    vectors = []
    d = rng.randrange(1, N)
    pub = ref.pub_bytes(ref.mul(d, G))

    def emit(cls, der, msg, canonical=0, want=None):
        ok = openssl_der_verdict(pub, der, msg)
        rs = ref.der_to_rs(der, 32)
        mine = 1 if rs is not None and ref.verify(pub, rs, msg) else 0
        assert ok == mine, f"{cls}: OpenSSL {ok}, restatement {mine}"
        if want is not None:
            assert ok == want, f"{cls}: expected {want}, OpenSSL says {ok}"
        if canonical:
            assert der == ref.der_encode(int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big"))
        vectors.append({"cls": cls, "key": pub.hex(), "msg": msg.hex(), "der": der.hex(), "canonical": canonical,
                        "ok": ok})

    def sign_where(pred, tag):
        i = 0
        while True:
            msg = b"der %s %d" % (tag, i)
            i += 1
            rs = ref.sign(d, msg, rng.randrange(1, N))
            if rs and pred(*rs):
                return msg, rs

    # canonical encodings: r, s with and without the sign byte, and short ones
    for tag, pred in ((b"hi hi", lambda r, s: r >> 255 and s >> 255), (b"lo lo", lambda r, s: not r >> 255 and not s >> 255),
                      (b"hi lo", lambda r, s: r >> 255 and not s >> 255), (b"lo hi", lambda r, s: not r >> 255 and s >> 255),
                      (b"short r", lambda r, s: r < 1 << 248), (b"short s", lambda r, s: s < 1 << 248)):
        for _ in range(2):
            msg, (r, s) = sign_where(pred, tag)
            emit("canonical", ref.der_encode(r, s), msg, 1, 1)
            emit("canonical_wrong_msg", ref.der_encode(r, s), msg + b"!", 1, 0)
            emit("canonical_high_s", ref.der_encode(r, N - s), msg, 1, 1)

    msg, (r, s) = sign_where(lambda r, s: r >> 255 and not s >> 255, b"damage")
    good = ref.der_encode(r, s)
    rb, sb = minimal(r), minimal(s)
    body = der_int(rb) + der_int(sb)
    assert seq(body) == good and openssl_der_verdict(pub, good, msg) == 1
    emit("trailing_byte", good + b"\x00", msg, 0, 0)
    emit("trailing_byte_inside", seq(body + b"\x00"), msg, 0, 0)
    emit("long_form_seq_length", b"\x30\x81" + bytes([len(body)]) + body, msg, 0, 0)
    emit("long_form_int_length", seq(b"\x02\x81" + bytes([len(rb)]) + rb + der_int(sb)), msg, 0, 0)
    emit("indefinite_length", b"\x30\x80" + body + b"\x00\x00", msg, 0, 0)
    emit("superfluous_zero_r", seq(der_int(b"\x00" + rb) + der_int(sb)), msg, 0, 0)
    emit("superfluous_zero_s", seq(der_int(rb) + der_int(b"\x00" + sb)), msg, 0, 0)
    emit("missing_zero_negative_r", seq(der_int(rb[1:]) + der_int(sb)), msg, 0, 0)
    emit("empty_integer_r", seq(der_int(b"") + der_int(sb)), msg, 0, 0)
    emit("empty_integer_s", seq(der_int(rb) + der_int(b"")), msg, 0, 0)
    emit("r_33_bytes", seq(der_int(minimal(r + (1 << 256))) + der_int(sb)), msg, 0, 0)
    emit("r_plus_n_33_bytes", seq(der_int(minimal(r + N)) + der_int(sb)), msg, 0, 0)
    emit("wrong_outer_tag", b"\x31" + good[1:], msg, 0, 0)
    emit("wrong_integer_tag", seq(b"\x03" + der_int(rb)[1:] + der_int(sb)), msg, 0, 0)
    for cut in (1, 2, 3, len(good) // 2, len(good) - 1):
        emit("truncated", good[:cut], msg, 0, 0)
    emit("empty", b"", msg, 0, 0)
    emit("nested_junk", seq(seq(body)), msg, 0, 0)
    emit("nested_junk", seq(der_int(rb) + seq(der_int(sb))), msg, 0, 0)
    emit("three_integers", seq(body + der_int(b"\x01")), msg, 0, 0)
    emit("one_integer", seq(der_int(rb)), msg, 0, 0)
    emit("seq_length_short", b"\x30" + bytes([len(body) - 1]) + body, msg, 0, 0)
    emit("seq_length_long", b"\x30" + bytes([len(body) + 1]) + body, msg, 0, 0)
    emit("r_zero", ref.der_encode(0, s), msg, 1, 0)
    emit("s_zero", ref.der_encode(r, 0), msg, 1, 0)
    emit("r_eq_n", ref.der_encode(N, s), msg, 1, 0)

    path = os.path.join(HERE, "ecdsa_der_vectors.json")
    with open(path, "w") as f:
        json.dump({"vectors": vectors}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(vectors)} vectors, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
