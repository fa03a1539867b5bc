"""The rollout's action table of uct_kernel's saturated form (csrc/uct_action_table.hpp: one byte per bucket of the draw's top
twelve bits, kUctActExact where a threshold lies inside the bucket) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/uct_action_table_check.cpp is a stand-alone host program (its own main, no HIP) that fills the table for uniform rows
of 2, 3, 4, 5, 6 and 8 actions, a row with two thresholds inside one bucket, a row with a zero in the middle, a row with trailing
zeros and rows in which one action takes all, and compares it with the restated rule at both ends of every bucket, at every
threshold and its neighbours, at 0 and at 2^64 - 1.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "uct_action_table_check.cpp")


def test_table_against_restated_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build the stand-alone check with")
    exe = str(tmp_path / "uct_action_table_check")
    # the sanitizers' runtimes linked INTO the program: it then runs whatever else the environment loads first
    clang = b"clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout
    static = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror"] + static + [SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = run.stdout.decode()
    assert run.returncode == 0, out
    assert out.startswith("ok:"), out
