"""bench.py's plain run on the hardware: set-up, warm-up, the timed steps, the --dump-outputs files and one line carrying the headline
and the roofline of those same steps - none of the secondary measurements that only `--full` runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("pcie_inclusive", "roofline_hbm", "unise_lm", "extras", "ssl_frontend", "cpu_baseline", "speedup_vs_cpu_baseline",
             "ranks_seen", "exchange", "configs3_tse", "configs4_hcodec20")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_of_full(qa_lib, gpu_device, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--seconds", "10", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["metric"] == "audio-seconds/sec H-Codec encode+decode @16kHz b=32" and line["unit"] == "audio-seconds/sec"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(4 * 10.0 * 1e3 / line["ms_per_step"], rel=1e-9)
    assert line["roofline"]["achieved"] > 0 and "isolated" not in line["roofline"]
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    wav = np.load(tmp_path / "wav.npy")
    assert wav.shape[0] == 4 and np.isfinite(wav).all()
    assert {f for f in os.listdir(tmp_path)} == {"acoustic_codes.npy", "semantic_codes.npy", "wav.npy"}
