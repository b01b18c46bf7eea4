"""Runs the C++ host-side test of BLS key generation in the plugin layer (BLS::Hip::BlsThresholdKeygen,
BlsMultisigKeygen and BlsThresholdFactory: random signers that sign, accumulate and verify; injected
coefficients against cbft_bls_keygen_threshold below, at and above the crossover; newKeyPair; and, without
the GPU, the sampling bounds, the key encodings and the crossover setting, also in a stand-alone build
under ASan + UBSan)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_bls_keygen_host")
SAN = os.path.join(ROOT, "tests", "cpp", "test_bls_keygen_san")


def _run(binary, *args, env=None):
    if not os.path.exists(binary):
        pytest.fail(f"{os.path.relpath(binary, ROOT)} not built (make host)")
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=300, env=env)


def test_cpp_bls_keygen_host_gpu_free_parts():
    r = _run(BIN, "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


def test_cpp_bls_keygen_host_crossover_override():
    r = _run(BIN, "--no-gpu", env=dict(os.environ, CBFT_BLS_KEYGEN_BATCH_MIN="17"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


def test_cpp_bls_keygen_gpu_free_parts_under_sanitizers():
    r = _run(SAN, "--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_bls_keygen_host():
    r = _run(BIN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
