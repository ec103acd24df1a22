"""conv_gemm's tile cost model (choose_tile in csrc/conv_gemm.hip) through the test hook qa_debug_conv_gemm_tile, which launches nothing
and answers for a weight with a pre-split image, as the recorded sweep ran (launches without one keep the round-4 model):
the fixed rules (narrow N, forced tiles, fall-backs), a legal answer over the M range the H-Codec 1.5 aggregators really see, and the
choice against the recorded per-tile sweep: with the device to itself (share = 1) the chosen tile must be within 3 % - three times
tools/gemm_bench.py's run-to-run noise - of the best tile measured, on every recorded shape."""
import ctypes as C

import pytest

T128x32, T128x64, T128x128, T64x128, T64x64, T256x128 = range(6)  # QA_GEMM_CFG values
MIMI = {"in_proj": (1536, 512), "out_proj": (512, 512), "lin1": (2048, 512), "lin2": (512, 2048)}  # (N, K) at d = 512, ff = 2048

# profiles/r07_gemm_tile_sweep.txt, "final build ... QA_BENCH_PLANES=1": TFLOP/s of 128x64, 128x128, 64x128, 64x64 forced, kernel alone
SWEEP = [
    ("cal.8192x4096x4096", 8192, 4096, 4096, (144.2, 158.9, 137.3, 128.9)),
    ("mimi.in_proj", 9056, 1536, 512, (116.6, 128.8, 127.3, 104.3)),
    ("mimi.out_proj", 9056, 512, 512, (82.7, 65.9, 90.1, 85.4)),
    ("mimi.lin1", 9056, 2048, 512, (125.1, 146.9, 131.8, 111.2)),
    ("mimi.lin2", 9056, 512, 2048, (107.3, 91.2, 118.4, 108.4)),
    ("bt.in_proj", 8000, 3072, 1024, (141.2, 176.0, 149.2, 121.4)),
    ("bt.lin1", 8000, 2048, 1024, (137.4, 166.0, 147.1, 119.8)),
    ("bt.lin2", 8000, 1024, 2048, (140.4, 173.1, 151.0, 120.7)),
    ("agg15.qkv", 9056, 1536, 512, (122.1, 130.5, 129.8, 107.6)),
    ("agg15.half", 4528, 512, 512, (60.0, 62.8, 67.5, 64.8)),
    ("convnext.pw1", 16000, 2304, 768, (139.4, 172.6, 147.7, 117.7)),
    ("convnext.pw2", 16000, 768, 2304, (142.6, 186.4, 154.4, 124.6)),
    ("dec.qkv", 16000, 2304, 768, (140.5, 173.8, 147.9, 120.9)),
    ("dec.w2", 16000, 768, 3072, (148.3, 189.0, 156.1, 126.0)),
    ("enc.lstm_ih", 16000, 2048, 512, (132.5, 161.9, 139.8, 115.1)),
]
SWEEP_TILES = (T128x64, T128x128, T64x128, T64x64)


@pytest.fixture()
def tile(qa_lib, knob):
    fn = qa_lib.qa_debug_conv_gemm_tile
    fn.restype = C.c_int
    fn.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
    for name in ("QA_GEMM_CFG", "QA_GEMM_256", "QA_GEMM_MATH", "QA_GEMM_LINEAR", "QA_GEMM_BK16", "QA_GEMM_BK16_MIN_TILES"):
        knob(name, {"QA_GEMM_CFG": -1, "QA_GEMM_256": 0, "QA_GEMM_MATH": 1, "QA_GEMM_LINEAR": 1, "QA_GEMM_BK16": 1 << 30,
                    "QA_GEMM_BK16_MIN_TILES": 384}[name])  # the defaults, whatever the environment says

    def _tile(M, N, K, ksize=1, linear=1, math_fp32=0, share=1):
        return fn(M, N, K, ksize, linear, math_fp32, share)

    return _tile


def test_narrow_layers_keep_their_fixed_tiles(tile):
    for M in (100, 4000, 5120000):
        for fp32 in (0, 1):
            assert tile(M, 32, 96, ksize=3, linear=0, math_fp32=fp32) == T128x32
            assert tile(M, 16, 64, math_fp32=fp32) == T128x32
            assert tile(M, 64, 128, math_fp32=fp32) == T128x64
            assert tile(M, 48, 64, math_fp32=fp32) == T128x64


def test_forced_tiles_and_fallbacks(tile, knob):
    for cfg in range(5):
        knob("QA_GEMM_CFG", cfg)
        assert tile(9056, 512, 512) == cfg and tile(9056, 512, 1536, ksize=3, linear=0) == cfg
    knob("QA_GEMM_CFG", T128x32)  # the 128 x 32 tile has no BK = 16 instance: 48 input channels take 128 x 64
    assert tile(4000, 768, 48) == T128x64
    knob("QA_GEMM_CFG", T256x128)  # exists for LINEAR layers only
    assert tile(9056, 2048, 512) == T256x128
    assert tile(9056, 2048, 1536, ksize=3, linear=0) == T128x128
    knob("QA_GEMM_LINEAR", 0)
    assert tile(9056, 2048, 512) == T128x128
    knob("QA_GEMM_LINEAR", 1)
    knob("QA_GEMM_CFG", 9)  # names no tile
    assert tile(9056, 2048, 512) == T128x128
    knob("QA_GEMM_CFG", -1)  # QA_GEMM_256 = 0: the cost model never picks the 256-row tile
    assert tile(16000, 2048, 512) != T256x128
    assert tile(0, 512, 512) < 0 and tile(9056, 512, 512, ksize=3) < 0  # bad arguments are refused


def test_every_aggregator_batch_gets_a_tile(tile):
    """G is data dependent: 32 clips of 10 s give M = 32 (250 + G) from about 8032 to 12000."""
    for M in range(8032, 12001, 32):
        for name, (N, K) in MIMI.items():
            for share in (1, 2):
                for fp32 in (0, 1):
                    assert tile(M, N, K, math_fp32=fp32, share=share) in SWEEP_TILES, (M, name, share, fp32)


def test_choice_is_within_3_percent_of_the_best_recorded_tile(tile):
    report, missed = [], []
    for name, M, N, K, tflops in SWEEP:
        cfg = tile(M, N, K)
        assert cfg in SWEEP_TILES, (name, cfg)
        got, best = tflops[SWEEP_TILES.index(cfg)], max(tflops)
        report.append(f"{name}: tile {cfg} at {got} of {best} TFLOP/s ({100.0 * (got / best - 1.0):+.1f} %)")
        if got < 0.97 * best:
            missed.append(report[-1])
    print("\n".join(report))
    assert not missed, missed
