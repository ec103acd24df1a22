"""Layout of a pre-split weight image (csrc/split_planes.h plane_byte_offset, exported as qa_weight_plane_offset), pinned against a
plain loop: the image is a sequence of groups of 8 floats; a group is three consecutive 16-byte units - planes h, m, l - of 8 bf16
each, in the order of the floats.  For a weight matrix [N][K] (K % 8 == 0) element (row, k) is float row * K + k, so a row's 16-wide
K chunk is 96 contiguous bytes and a row slice starts on a group."""


def _loop_offsets(n):
    """byte offset of (index, plane) by writing the image out unit by unit"""
    off, pos = {}, 0
    for group in range(n // 8):
        for plane in range(3):
            for j in range(8):
                off[(group * 8 + j, plane)] = pos
                pos += 2
    assert pos == 6 * n
    return off


def test_plane_offset_matches_a_plain_loop(qa_lib):
    n = 8 * 40
    want = _loop_offsets(n)
    for (index, plane), o in want.items():
        assert qa_lib.qa_weight_plane_offset(index, plane) == o, (index, plane)


def test_rows_and_chunks_of_a_weight_matrix(qa_lib):
    N, K = 5, 48
    want = _loop_offsets(N * K)
    for row in range(N):
        for k in range(K):
            for plane in range(3):
                assert qa_lib.qa_weight_plane_offset(row * K + k, plane) == want[(row * K + k, plane)]
        # a row starts on a group, and each of its 16-wide chunks is 96 contiguous bytes: slots (k / 8) of planes h, m, l
        start = qa_lib.qa_weight_plane_offset(row * K, 0)
        assert start == row * K * 6 and start % 48 == 0
        for chunk in range(K // 16):
            lo = qa_lib.qa_weight_plane_offset(row * K + 16 * chunk, 0)
            hi = qa_lib.qa_weight_plane_offset(row * K + 16 * chunk + 15, 2) + 2
            assert (lo, hi) == (start + 96 * chunk, start + 96 * (chunk + 1))


def test_plane_offset_rejects_bad_arguments(qa_lib):
    assert qa_lib.qa_weight_plane_offset(-1, 0) < 0
    assert qa_lib.qa_weight_plane_offset(0, 3) < 0
    assert qa_lib.qa_weight_plane_offset(0, -1) < 0
    assert qa_lib.qa_weight_plane_offset((1 << 40) + 3, 2) == ((1 << 40) // 8) * 48 + 32 + 6
