"""Runs the C++ host-side tests of batched RSA signing in the plugin layer (HipRSASigner::signBatch,
HipSigManager::signBatch with an RSA own key, signPreProcessReplyHashes, the host fall-back on a
GPU failure, a 3,072-bit key on the host only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_rsa_sign_host")


@pytest.mark.gpu
def test_cpp_rsa_sign_host():
    if not os.path.exists(BIN):
        pytest.fail("tests/cpp/test_rsa_sign_host not built (make host)")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
