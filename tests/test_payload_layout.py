"""The payload exchange's host arithmetic (partisan_amd/csrc/psim_payload.h:
counts to offsets, import bases, byte accounting) as a stand-alone program
under AddressSanitizer and UBSan -- host code only, no device, no library
loaded into Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _cxx():
    for c in ("g++", "c++", "clang++"):
        try:
            if subprocess.run([c, "--version"], capture_output=True).returncode == 0:
                return c
        except OSError:
            pass
    return None


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_payload_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "payload_layout_check")
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "payload_layout_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "payload layout ok" in r.stdout, r.stdout + r.stderr
