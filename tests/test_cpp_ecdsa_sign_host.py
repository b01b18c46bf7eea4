"""Runs the C++ host-side test of concord::hip::HipECDSASigner (keys from hex DER and PEM, sign()
against signBatch() on the GPU and on the host path, every signature accepted by HipECDSAVerifier and
OpenSSL, a secp384r1 key on the host path, the ecdsaSignStats() counters; parsing, sign() and the host
path without the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_ecdsa_sign_host")


def _run(*args):
    if not os.path.exists(BIN):
        pytest.fail("tests/cpp/test_ecdsa_sign_host not built (make host)")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


def test_cpp_ecdsa_sign_host_gpu_free_parts():
    r = _run("--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_ecdsa_sign_host():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
