"""Pcg64W (csrc/pcg64.hpp: the PCG64 step on four 32-bit words) on the host, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host/pcg64_words_check.cpp is a stand-alone program (its own main, no HIP) that includes the
header's host path and compares it with unsigned __int128 over the case list of tests/pcg64_words_cases.py and three million
random records.  No GPU; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import pcg64_words_cases as pw

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "pcg64_words_check.cpp")


def test_header_against_int128_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build the stand-alone check with")
    exe = str(tmp_path / "pcg64_words_check")
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        for _, state, inc in pw.CASES:
            f.write("{:x} {:x} {:x} {:x}\n".format(state >> 64, state & pw.M64, inc >> 64, inc & pw.M64))
    # the sanitizers' runtimes linked INTO the program: it then runs whatever else the environment loads first
    clang = b"clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout
    static = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror"] + static + [SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = run.stdout.decode()
    assert run.returncode == 0, out
    assert out.startswith("ok: {} cases".format(len(pw.CASES))), out
