"""launch_row_ints (csrc/ew.hip) alone through its test hook qa_debug_row_ints: the one kernel that carries the host
integers of every call with per-row lengths - clip lengths, row counts, positions, offsets - into device memory, ROW_INTS_CHUNK = 256 of
them per launch, by value in the launch arguments.

Counts: 1, one below / at / one above the chunk, 258 (= 3 x 86: the SSL front-end's first two-launch call), two chunks, two chunks and
one.  Everything is an integer copy: every comparison is torch.equal.

    1  dst[:count] is the source; every word in front of and behind it keeps its sentinel
    2  by value: the host source may be overwritten as soon as the call returns
    3  stream order: two uploads to the same array, each followed by a device copy, on one stream
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (1, 255, 256, 257, 258, 512, 513)
HEAD, TAIL = 300, 600  # sentinel words in front of dst and behind dst[count - 1]: more than a chunk on either side
SENTINEL = -0x5A5A5A5B


@pytest.fixture(scope="module")
def upload(qa_lib):
    fn = qa_lib.qa_debug_row_ints
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]

    def call(dst, src):
        """src: a C-contiguous int32 numpy array in host memory; dst: a device int32 tensor (view) of at least src.size words"""
        assert src.dtype == np.int32 and src.flags.c_contiguous and dst.dtype == torch.int32 and dst.is_contiguous()
        st = fn(dst.data_ptr(), src.ctypes.data, src.size, torch.cuda.current_stream().cuda_stream)
        assert st == 0, qa_lib.qa_last_error()

    return call


def _values(count, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-2**31, 2**31, size=count, dtype=np.int64).astype(np.int32)
    v[0], v[-1] = np.int32(2**31 - 1), np.int32(-2**31)  # the ends of the range at the ends of the vector
    return v


def _guarded(dev, count):
    buf = torch.full((HEAD + count + TAIL,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[HEAD:HEAD + count]


@pytest.mark.parametrize("count", COUNTS)
def test_every_word_arrives_and_nothing_else_is_written(upload, gpu_device, count):
    src = _values(count, 100 + count)
    buf, dst = _guarded(gpu_device, count)
    upload(dst, src)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[HEAD:HEAD + count], torch.from_numpy(src))
    assert bool((got[:HEAD] == SENTINEL).all()) and bool((got[HEAD + count:] == SENTINEL).all())


@pytest.mark.parametrize("count", (257, 513))
def test_the_values_travel_by_value(upload, gpu_device, count):
    src = _values(count, 200 + count)
    want = torch.from_numpy(src.copy())
    buf, dst = _guarded(gpu_device, count)
    upload(dst, src)
    src[:] = 7  # directly after the call returns, before any synchronisation
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("count", (257, 513))
def test_uploads_are_ordered_on_their_stream(upload, gpu_device, count):
    a, b = _values(count, 300 + count), _values(count, 400 + count)
    assert not np.array_equal(a, b)
    buf, dst = _guarded(gpu_device, count)
    x, y = torch.empty_like(dst), torch.empty_like(dst)
    upload(dst, a)
    x.copy_(dst)
    upload(dst, b)
    y.copy_(dst)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(a)) and torch.equal(y.cpu(), torch.from_numpy(b))
