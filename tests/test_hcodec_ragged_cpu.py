"""Per-clip lengths of the H-Codec entry points, the parts that need no GPU: the two C-ABI symbols are declared, exported and bound with
matching argument types; the tokenizer's sample -> code-frame arithmetic; the argument checks made on the host."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPE = {"qa_hcodec*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "void*": C.c_void_p,
          "int64_t": C.c_int64, "const int64_t*": None}  # const int64_t*: device codes (void*) or the HOST lengths (POINTER(int64))


def _declaration(name):
    header = open(os.path.join(ROOT, "include", "quarkaudio.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in quarkaudio.h"
    args = []
    for a in m.group(1).split(","):
        a = re.sub(r"/\*.*?\*/", "", a, flags=re.S).split()
        args.append((" ".join(a[:-1]), a[-1]))
    return args


@pytest.mark.parametrize("name", ["qa_hcodec_encode_ragged", "qa_hcodec_decode_ragged"])
def test_ragged_entry_points_are_declared_exported_and_bound(qa_lib, name):
    from unified_audio_amd import _lib

    args = _declaration(name)
    assert hasattr(qa_lib, name)
    res, bound = _lib.SYMBOLS[name]
    assert res is C.c_int and len(bound) == len(args), (len(bound), args)
    for (ctype, arg), got in zip(args, bound):
        if arg == "frames":  # host memory: a typed pointer, so that ctypes refuses a tensor's data_ptr() there
            assert ctype == "const int64_t*" and got is C.POINTER(C.c_int64)
        else:
            assert got is (_CTYPE[ctype] or C.c_void_p), (name, arg, ctype, got)
    names = [a for _, a in args]
    assert names.index("frames") == (4 if "encode" in name else 5) and names[-1] == "stream"


def test_sample_lengths_round_up_to_code_frames():
    from unified_audio_amd import hcodec

    assert hcodec.code_frames([16 * 10 + 7, 16 * 3 + 1, 16, 1], 16) == [11, 4, 1, 1]
    lens = [1, 639, 640, 641, 160000]
    assert hcodec.code_frames(torch.tensor(lens), 640) == [math.ceil(n / 640) for n in lens] == [1, 1, 1, 2, 250]
    for bad in ([0], [-5], [640, 0]):
        with pytest.raises(hcodec._lib.QuarkAudioError) as e:
            hcodec.code_frames(bad, 640)
        assert e.value.status == -1 and f"lengths[{len(bad) - 1}]" in str(e.value)


def test_length_arguments_are_checked_on_the_host():
    from unified_audio_amd import hcodec

    arr = hcodec._frames_arg(torch.tensor([3, 1, 2]), 3)
    assert list(arr) == [3, 1, 2] and C.sizeof(arr) == 24
    assert list(hcodec._frames_arg([7], 1)) == [7]
    for bad, B in (([3, 1], 3), ([1.5, 2], 2), (torch.tensor([1.0, 2.0]), 2), (torch.ones(2, 2, dtype=torch.int64), 2), ([True, 1], 2)):
        with pytest.raises(hcodec._lib.QuarkAudioError) as e:
            hcodec._frames_arg(bad, B)
        assert e.value.status == -1


def test_null_arguments_are_refused_without_a_device(qa_lib):
    fr = (C.c_int64 * 1)(1)
    assert qa_lib.qa_hcodec_encode_ragged(None, None, 1, 640, fr, None, 0, 0, 0, 2, None, None, None) == -1
    assert b"qa_hcodec_encode_ragged" in qa_lib.qa_last_error()
    assert qa_lib.qa_hcodec_decode_ragged(None, None, None, 1, 1, fr, None, None) == -1
    assert b"qa_hcodec_decode_ragged" in qa_lib.qa_last_error()
