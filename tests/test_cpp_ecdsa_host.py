"""Runs the C++ host-side test of concord::hip::HipECDSAVerifier (keys from hex DER and PEM, verify()
and verifyBatch() against the host OpenSSL, wrong-length signatures, a secp384r1 key on the host
path; key parsing, the host path and the length rule without the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_ecdsa_host")


def _run(*args):
    if not os.path.exists(BIN):
        pytest.fail("tests/cpp/test_ecdsa_host not built (make host)")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


def test_cpp_ecdsa_host_gpu_free_parts():
    r = _run("--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_ecdsa_host():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
