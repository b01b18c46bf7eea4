"""Runs the C++ host-side test of concord::hip::HipP256PrivateKey (PRIVATE_KEY:secp256r1:<hex scalar>, DER
signatures with RFC 6979 nonces): constructor refusals, sign() against the host OpenSSL and HipP256PublicKey,
signBatch() against the sign() loop, serialize() and the counters.  --no-gpu keeps every batch under the GPU
minimum; that mode also runs as a stand-alone ASan + UBSan program with the host sources compiled in."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_ecdsa_p256_sign_host")


def _run(binary, *args):
    if not os.path.exists(binary):
        pytest.fail(os.path.relpath(binary, ROOT) + " not built (make host)")
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=300)


def test_cpp_ecdsa_p256_sign_host_under_the_minimum():
    r = _run(BIN, "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed under the GPU minimum" in r.stdout


def test_cpp_ecdsa_p256_sign_host_under_the_minimum_sanitized():
    r = _run(BIN + "_san", "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed under the GPU minimum" in r.stdout


@pytest.mark.gpu
def test_cpp_ecdsa_p256_sign_host():
    r = _run(BIN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed\n" in r.stdout
