"""GPU: the C++ adaptor host/ResidualLinearizer.hpp (linearizeAll for one window and for many) driven by host/linearize_demo.cpp like
the passes of FrontEnd::optimize: the printed states, the hashes of the energies and of the Jacobian rows, the energy sum, the new
threshold, the kept list and the per-point updates against the checker tests/_linearize_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
from _window_files import fnv1a, write_window

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_one_window_many_windows_and_host_form_equal_the_checker(built, ctx, tmp_path):
    job, frames, exp, _ = R.case("scene")
    path = tmp_path / "window.bin"
    write_window(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "linearize_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["n_res"] == len(job["point"])
    assert res["states"] == "".join(str(int(s)) for s in exp["new_state"])
    assert res["energy_hash"] == f"{fnv1a(exp['new_energy_with_outlier'].tobytes(), fnv1a(exp['new_energy'].tobytes())):016x}"
    h = 1469598103934665603
    for r in np.flatnonzero(exp["defined"]):
        h = fnv1a(exp["J"][r].tobytes() + exp["center_projected_to"][r].tobytes() + exp["projected_to"][r].tobytes(), h)
    assert res["row_hash"] == f"{h:016x}"
    assert res["energy_bits"] == f"{np.float64(exp['energy']).view(np.uint64):016x}"
    assert res["threshold_bits"] == f"{np.float32(exp['new_frame_energy_th']).view(np.uint32):08x}"
    assert res["kept"] == [int(r) for r in np.flatnonzero(exp["keep"])]
    good = {}
    for r in np.flatnonzero(exp["keep"].astype(bool) & np.asarray(job["is_new"]).astype(bool)):
        p = int(job["point"][r])
        n, best = good.get(p, (0, np.float32(0.0)))
        good[p] = (n + 1, max(best, exp["rel_bs"][r]))
    assert res["good_points"] == [[p, n, int(np.float32(b).view(np.uint32))] for p, (n, b) in sorted(good.items())]
    assert len(good) >= 10 and sum(1 for n, _ in good.values() if n >= 2) >= 3
