"""GPU: the C++ adaptor host/TraceNewCoarse.hpp (traceNewCoarse for one sequence and for many) driven by
host/trace_new_coarse_demo.cpp like the loop of FrontEnd.cpp:276-327, two frames in a row: the printed statuses, counts, steps and
the hash of the traced floats against the checker tests/_trace_ref.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _trace_ref as R
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def traced(res):
    """the floats the demo hashes, NaNs made canonical"""
    a = np.concatenate([res[k].reshape(len(res["status"]), -1) for k in ("idepth_min", "idepth_max", "quality", "trace_uv", "trace_interval")],
                       axis=1).astype(np.float32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits.tobytes()


def test_adaptor_one_sequence_many_sequences_and_host_form_equal_the_checker(built, ctx, tmp_path):
    seq = R.sequence()[:2]
    job = seq[0][1]
    n, nh = len(job["host"]), len(job["kt"])
    hosts = np.concatenate([job["krki"].reshape(nh, 9), job["kt"].reshape(nh, 3), job["aff"].reshape(nh, 2)], axis=1).astype(np.float32)
    rec = np.zeros((n, 32), np.float32)
    rec[:, 0], rec[:, 1] = job["host"].astype(np.int32).view(np.float32), job["status"].astype(np.int32).view(np.float32)
    rec[:, 2], rec[:, 3], rec[:, 4] = job["u"], job["v"], job["energy_th"]
    rec[:, 5:9], rec[:, 9:17], rec[:, 17:25] = job["grad_h"], job["color"], job["weights"]
    rec[:, 25], rec[:, 26], rec[:, 27] = job["idepth_min"], job["idepth_max"], job["quality"]
    rec[:, 28:30], rec[:, 30] = job["trace_uv"], job["trace_interval"]
    path = tmp_path / "sequence.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("iiiii", R.W, R.H, len(seq), nh, n))
        f.write(b"".join(np.ascontiguousarray(frame, np.float32).tobytes() for frame, _, _ in seq) + hosts.tobytes() + rec.tobytes())
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "trace_new_coarse_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["n_pts"] == n and len(res["frames"]) == 2
    for got, (_, _, exp) in zip(res["frames"], seq):
        assert got["statuses"] == "".join(str(int(s)) for s in exp["status"])
        assert got["counts"] == exp["counts"].tolist() and got["steps"] == int(exp["steps"].sum())
        assert got["hash"] == f"{fnv1a(traced(exp)):016x}"
    assert seq[1][2]["counts"].tolist() != seq[0][2]["counts"].tolist()  # the second frame started from the state the first left
