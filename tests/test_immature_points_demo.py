"""GPU: the C++ adaptor host/ImmaturePoints.hpp (KeyframeWindow, optimizeImmaturePoints for one window and for many) driven by
host/immature_points_demo.cpp like the loop of FrontEnd.cpp:458-468: the printed statuses, the hash of the idepths and the IN-target
lists against the checker tests/_immature_ref.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _immature_ref as R
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_one_window_many_windows_and_host_form_equal_the_checker(built, ctx, tmp_path):
    job, frames, exp, _ = R.case("not_brightened")
    nf, n = len(frames), len(job["host"])
    pre = np.concatenate([job["pre_R"].reshape(nf * nf, 9), job["pre_t"].reshape(nf * nf, 3), job["pre_aff"].reshape(nf * nf, 2)], axis=1).astype(np.float32)
    rec = np.zeros((n, 22), np.float32)
    rec[:, 0] = job["host"].view(np.float32)
    for k, name in enumerate(("u", "v", "idepth_min", "idepth_max", "energy_th")):
        rec[:, 1 + k] = job[name]
    rec[:, 6:14], rec[:, 14:22] = job["color"], job["weights"]
    path = tmp_path / "window.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("ii", R.W, R.H) + np.array(list(job["cam"]) + list(job["cam_inv"]), np.float32).tobytes())
        f.write(struct.pack("ii", nf, job["min_obs"]) + job["frame_ids"].astype(np.int32).tobytes())
        f.write(b"".join(np.ascontiguousarray(fr, np.float32).tobytes() for fr in frames) + pre.tobytes())
        f.write(struct.pack("i", n) + rec.tobytes())
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "immature_points_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["n_pts"] == n
    assert res["statuses"] == "".join(str(int(s)) for s in exp["status"])
    assert res["idepth_hash"] == f"{fnv1a(exp['idepth'].tobytes()):016x}"
    ids = [int(i) for i in job["frame_ids"]]
    targets, last = [], []
    for i in range(n):
        t = [f for f in range(nf) if exp["res_state"][i, f] == R.IN] if exp["status"][i] == 1 else []
        targets.append([ids[f] for f in t])
        last.append([t.index(nf - 1) if nf - 1 in t else -1, t.index(nf - 2) if nf - 2 in t else -1])
    assert res["in_targets"] == targets and res["last_residuals"] == last
    assert sum(1 for t in targets if len(t) >= 2) >= 20 and sum(1 for a, b in last if a >= 0) >= 20 and sum(1 for a, b in last if b >= 0) >= 20
