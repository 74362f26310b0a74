"""GPU: the C++ adaptor host/WindowHessian.hpp (accumulateWindow for one window, accumulateWindows for many) driven by
host/hessian_demo.cpp like a pass of FrontEnd::optimize: the printed states and active flags and the hashes of H_A, b_A, H_sc, b_sc,
JpJdF and the per-point results against the checker tests/_hessian_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
from _window_files import fnv1a, write_hessian

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_one_window_many_windows_and_host_form_equal_the_checker(built, ctx, tmp_path):
    job, frames, exp = HR.case("scene")
    path = tmp_path / "window.bin"
    write_hessian(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "hessian_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["n_res"] == len(job["point"])
    assert res["states"] == "".join(str(int(s)) for s in exp["new_state"])
    assert res["active"] == "".join(str(int(s)) for s in exp["active"])
    for k in HR.STITCHED:
        assert res[k] == f"{fnv1a(exp[k].tobytes()):016x}", k
    jp = np.where(exp["active"].astype(bool)[:, None], exp["JpJdF"], np.float32(0.0))
    assert res["JpJdF"] == f"{fnv1a(jp.tobytes()):016x}"
    assert res["points"] == f"{fnv1a(exp['idepth_hessian'].tobytes(), fnv1a(exp['bd_sum'].tobytes(), fnv1a(exp['hdi'].tobytes()))):016x}"
    assert res["energy_bits"] == f"{np.float64(exp['energy']).view(np.uint64):016x}"
    assert exp["active"].sum() >= 50
