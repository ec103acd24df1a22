"""The host check behind the 32-bit entries of conv_gemm's source-frame table (csrc/conv_offsets.h): a tile's
entries stay below (ceil(BM / T_out) + 1) * T_in * ldx, which has to be below 2^31.  As a stand-alone program under the host sanitizers,
compiled with -fsanitize=address,undefined and run as a program of its own (tools/conv_offsets_selftest.cpp): the limit itself, one below
and one above it, T_out = 1, T_out > BM, products that leave int64, and the bound against a walk over every tile of small grids."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: tools/conv_offsets_selftest.cpp cannot be built")
    exe = str(tmp_path / "conv_offsets_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I",
           os.path.join(ROOT, "unified_audio_amd", "csrc"), os.path.join(ROOT, "tools", "conv_offsets_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "conv_offsets_selftest: ok" in r.stdout
