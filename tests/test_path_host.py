"""CPU: the host arithmetic of the read paths (csrc/kc_path_host.h: the cut of a text into passes, a
GAF line's path and lengths) in tools/path_host_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a stand-alone program."""
import os
import subprocess

from conftest import PKG


def test_path_host_check_is_clean_under_the_sanitizers():
    p = subprocess.run(["make", "-C", PKG, "bin/path_host_check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([os.path.join(PKG, "bin", "path_host_check")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    assert p.stdout.strip() == "path_host_check: OK"
