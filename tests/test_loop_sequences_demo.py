"""The C++ demo of a node running many sequences (host/loop_sequences_demo.cpp): one RingKeyIndex per sequence, one
dsm_host::search_ringkey_many call per advance, checked inside the demo against per-sequence search_ringkey on twin indexes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_loop_sequences_demo(built):
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "loop_sequences_demo")
    assert os.path.exists(exe)
    out = subprocess.run([exe, "8", "260"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"sequences=8 advances=260 queries=(\d+) candidates=(\d+) mismatches=(\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == 8 * 260 + 26  # sequence 2 marginalises two keyframes every tenth advance
    assert int(m.group(2)) > 20 and int(m.group(3)) == 0
