"""The two 16-bit transition tables of the LDS-resident UCT forms (csrc/uct_term_table.hpp: bit 15 = terminal[next], or
terminal[s] of the state a record leaves) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/uct_term_table_check.cpp
is a stand-alone host program (its own main, no HIP) that fills both tables for random models with and without terminal flags, a
model of 32 767 states and a model in which every record's bit differs between the tables, compares every record with a
restatement of the two terminal rules, and walks the model to check that the source table's bit is the bit a kernel without it
carries from the previous record.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "uct_term_table_check.cpp")


def test_both_tables_against_restated_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build the stand-alone check with")
    exe = str(tmp_path / "uct_term_table_check")
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
