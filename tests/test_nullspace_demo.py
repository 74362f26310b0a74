"""GPU: the C++ adaptor host/WindowNullspace.hpp driven by host/nullspace_demo.cpp like FrontEnd::solveSystem before a solve: one
window, two windows in one call, the device's basis fed to host/WindowSolve.hpp, and the host form, against the checkers
tests/_nullspace_ref.py and tests/_solve_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
import _nullspace_ref as NR
import _solve_ref as SR
from _window_files import fnv1a, write_nullspace

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_one_window_two_windows_solve_and_host_form(built, ctx, tmp_path):
    job, frames, exp = SR.case("scene", n_null=7)
    nf, N = len(job["frame_ids"]), len(exp["x"])
    poses = [NR.make_job(90, nf), NR.make_job(91, nf)]
    path, out_path = tmp_path / "window.bin", tmp_path / "null.bin"
    write_nullspace(path, R.W, R.H, job, frames, poses)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "nullspace_demo")
    out = subprocess.run([exe, str(path), str(out_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["windows_equal"] == 1 and res["host_repeats_device"] == 1 and res["rank"] == [7, 7] and res["flags"] == [0, 0]
    raw = np.fromfile(out_path, np.float64)
    assert len(raw) == 14 * N + 42 * nf
    basis, pinv, blocks = raw[:7 * N].reshape(N, 7), raw[7 * N:14 * N].reshape(7, N), raw[14 * N:].reshape(nf, 42)
    own = NR.nullspace(dict(poses[0], frame_null_in=blocks))  # the checker behind the device's blocks
    assert NR.bits_equal(basis, own["null_basis"]) and NR.bits_equal(pinv, own["null_pinv"])
    sol = SR.solve(dict(job, null_basis=basis, null_pinv=pinv, n_null=7), exp)
    hx = lambda a: f"{fnv1a(np.ascontiguousarray(a).tobytes()):016x}"  # noqa: E731
    assert res["x"] == hx(sol["x"]) and res["x_finite"] == 1 and sol["x0"].tobytes() != sol["x"].tobytes()
    ref = NR.nullspace(poses[0])  # the host form from the poses: the same C library as the checker's
    assert res["host_basis"] == hx(ref["null_basis"]) and res["host_pinv"] == hx(ref["null_pinv"]) and res["host_pre"] == hx(ref["null_x0_pre"])
    assert res["scale_column"] == hx(ref["null_x0_pre"][:, 8])
