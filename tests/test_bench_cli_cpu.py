"""bench.py's command line: a plain run is the lean one; `--full` (every secondary measurement) is opt-in."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _argv_parse(argv):
    sys.path.insert(0, ROOT)
    import bench

    saved = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = saved


def test_full_is_off_by_default_and_excludes_lean():
    assert _argv_parse([]).full is False and _argv_parse(["--full"]).full is True
    with pytest.raises(SystemExit):
        _argv_parse(["--full", "--lean"])
