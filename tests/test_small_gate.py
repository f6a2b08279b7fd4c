"""The small-call gate and the server slot registry (csrc/small_gate.h) off the GPU.

tests/c_abi/small_gate_check.cpp includes that header alone and makes no HIP call: 36 threads go
through the gate and it asserts the cap, the completion of every pass, first-in first-out
admission and the slot registry.  It is built with ThreadSanitizer and with AddressSanitizer +
UBSan, at the product's cap and at a cap of 1, and each binary is run directly as a plain program.
"""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "c_abi", "small_gate_check.cpp")
CSRC = os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc")
# the runtimes linked statically: the binaries need nothing from the environment they run in
FLAVOURS = {"tsan": ["-fsanitize=thread", "-static-libtsan"],
            "asan_ubsan": ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]}


@pytest.mark.parametrize("cap", [None, 1], ids=["product_cap", "cap_1"])
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_small_gate_check_runs_clean(tmp_path, flavour, cap):
    exe = str(tmp_path / "small_gate_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror",
           *FLAVOURS[flavour], "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe]
    if cap is not None:
        cmd.insert(1, f"-DEEGFX_SMALL_CALLERS={cap}")
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "small_gate_check ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
