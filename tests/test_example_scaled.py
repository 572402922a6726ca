"""examples/train_scaled.py stays runnable and shows what it claims."""

import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_scaled_example_runs():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "train_scaled.py"),
         "--n", "1000", "--d", "32", "--iters", "10"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    m = re.search(r"final loss: raw ([0-9.]+)\s+scaled ([0-9.]+)", out.stdout)
    assert m, out.stdout[-2000:]
    raw, scaled = float(m.group(1)), float(m.group(2))
    assert scaled < raw
    assert "feature_scaling=True" in out.stdout
