"""The host plan of a stream step (csrc/stream_step.h): which steps of the streaming H-Codec encoder and of a
Transformer stream are legal, which fault and row a refusal names, and what a legal step hands to its kernels.  A stand-alone program
under the host sanitizers, compiled with -fsanitize=address,undefined and run as a program of its own (tools/stream_step_selftest.cpp),
which compares the planner with a naive restatement of its rules."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    name = "stream_step_selftest"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail(f"no host C++ compiler: tools/{name}.cpp cannot be built")
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I",
           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "unified_audio_amd", "csrc"), os.path.join(ROOT, "tools", name + ".cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "stream_step_selftest: ok" in r.stdout
