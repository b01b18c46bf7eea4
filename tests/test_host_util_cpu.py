"""The HIP-free helpers that the host front ends share (concord-bft_amd/csrc/cbft_host_util.h: the
message span with its rebased offsets, the packed input image's layout, the verdict words -> bitmap
copy, the wipe), as a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/host_util_test.cpp; never loaded into python).  The program compares the span helper with
the loop the front ends wrote out before it existed, on empty, zero-length, descending, 2^64-edge,
length-cap and null-blob inputs, each array in a heap buffer of exactly its size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "cpp", "host_util_test")


def test_stand_alone_sanitizer_run():
    assert os.path.exists(PROG), "tests/cpp/host_util_test not built (make host_util_test)"
    p = subprocess.run([PROG], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "span, bitmap, layout, wipe ok" in p.stdout
