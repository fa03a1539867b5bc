"""The wave-balance rule of uct_kernel's saturated form (csrc/uct_balance.hpp: the priority a wave runs its next rollout at,
from the progress words of its workgroup) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/uct_balance_rule_check.cpp is a stand-alone host program (its own main, no HIP) with the named cases -- no mates, a
finished mate, a tie, behind, ahead -- and random workgroups of 1, 2, 4, 8 and 16 waves against a restatement.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "uct_balance_rule_check.cpp")


def test_rule_against_restatement_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) to build the stand-alone check with")
    exe = str(tmp_path / "uct_balance_rule_check")
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
