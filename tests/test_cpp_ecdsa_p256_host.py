"""Runs the C++ host-side test of the P-256 plugin layer: concord::hip::HipECDSAVerifier on prime256v1 keys
from hex DER and PEM and concord::hip::HipP256PublicKey from PUBLIC_KEY:secp256r1:<hex point> with DER
signatures, both against the host OpenSSL.  --no-gpu keeps every item under the GPU minimum; that mode also
runs as a stand-alone ASan + UBSan program with the host sources compiled in."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_ecdsa_p256_host")


def _run(binary, *args):
    if not os.path.exists(binary):
        pytest.fail(os.path.relpath(binary, ROOT) + " not built (make host)")
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=300)


def test_cpp_ecdsa_p256_host_under_the_minimum():
    r = _run(BIN, "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed under the GPU minimum" in r.stdout


def test_cpp_ecdsa_p256_host_under_the_minimum_sanitized():
    r = _run(BIN + "_san", "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed under the GPU minimum" in r.stdout


@pytest.mark.gpu
def test_cpp_ecdsa_p256_host():
    r = _run(BIN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed\n" in r.stdout
