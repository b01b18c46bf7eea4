"""Runs the C++ host-side tests of batched signing in the plugin layer (EdDSASigner::signBatch,
HipSigManager::signBatch, signPreProcessReplyHashes, the host fall-back on a GPU failure)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_sign_host")


@pytest.mark.gpu
def test_cpp_sign_host():
    if not os.path.exists(BIN):
        pytest.fail("tests/cpp/test_sign_host not built (make host)")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
