"""GPU: the C++ adaptor host/WindowSolve.hpp (solveWindow for one window, solveWindows for many) driven by host/solve_demo.cpp like a
trial step of FrontEnd::optimize: the hashes of lastX, the points' steps, lastHS, lastbS and the calibration step against the checker
tests/_solve_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
import _solve_ref as SR
from _window_files import fnv1a, write_solve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_one_window_many_windows_and_host_form_equal_the_checker(built, ctx, tmp_path):
    job, frames, exp = SR.case("scene", n_null=7)
    path = tmp_path / "window.bin"
    write_solve(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "solve_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["n_res"] == len(job["point"])
    assert res["x_finite"] == 1 and res["steps_finite"] == 1 and exp["flags"] == 0
    for k in ("x", "step", "last_HS", "last_bS"):
        assert res[k] == f"{fnv1a(np.ascontiguousarray(exp[k]).tobytes()):016x}", k
    assert res["step_c"] == f"{fnv1a((-exp['x'][:4]).tobytes()):016x}"
    assert exp["step"].any() and exp["x0"].tobytes() != exp["x"].tobytes()
