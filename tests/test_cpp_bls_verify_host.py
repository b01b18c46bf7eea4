"""Runs the C++ host-side test of batched BLS verification in the plugin layer
(BLS::Hip::BlsThresholdVerifier::verifyBatch against verify() and the accumulator's share check, below
and above the crossover; request validation and digest deduplication without the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_bls_verify_host")


def _run(*args, env=None):
    if not os.path.exists(BIN):
        pytest.fail("tests/cpp/test_bls_verify_host not built (make host)")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300, env=env)


def test_cpp_bls_verify_host_gpu_free_parts():
    r = _run("--no-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


def test_cpp_bls_verify_host_crossover_override():
    r = _run("--no-gpu", env=dict(os.environ, CBFT_BLS_VERIFY_BATCH_MIN="17"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all GPU-free checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_bls_verify_host():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
