"""The visited-mask rule of csrc/uct_virgin.hpp (first_child | mask << 24: a child whose bit is clear was never stored and reads as
{0.0, 0, -1}) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/uct_visited_mask_check.cpp is a stand-alone host
program (its own main, no HIP) that runs the word helpers and the export's fill on hand-made trees -- mask 0, the full mask, a
clear bit over garbage memory, -1 words, a first_child of 2^24 - 1 -- and on random ones against a plain restatement.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "uct_visited_mask_check.cpp")


def test_mask_rule_against_restatement_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build the stand-alone check with")
    exe = str(tmp_path / "uct_visited_mask_check")
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
