"""The host check of the length vector of every call with per-row lengths (csrc/row_lengths.h) and its formatter
for the per-clip BiCodec / resample / wav_normalize calls (csrc/clip_lengths.h), each as a stand-alone program under the host sanitizers:
compiled with -fsanitize=address,undefined and run as a program of its own (tools/row_lengths_selftest.cpp,
tools/clip_lengths_selftest.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, ok", [("row_lengths_selftest", "row_lengths_selftest: ok"), ("clip_lengths_selftest", "clip_lengths_selftest ok")])
def test_selftest_is_clean_under_the_host_sanitizers(tmp_path, name, ok):
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
    assert ok in r.stdout
