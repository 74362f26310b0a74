"""GPU: the C++ adaptor host/WindowOptimize.hpp driven by host/optimize_demo.cpp: the loop of FrontEnd::optimize as ONE call for one
window, for two DIFFERENT windows in one call that decide differently, and through the host form, against the checker
tests/_optimize_ref.py as tests/test_step_demo.py compares its loop."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
import _optimize_ref as O
import _step_ref as T
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def test_adaptor_one_window_two_different_windows_and_host_form(built, ctx, tmp_path):
    """The host form's outcome equals the checker's bit for bit (same C library).  On the device each window of the call of two equals
    itself alone bit for bit, the two decide differently, each takes the checker's decisions and ends within n_res x 2^-22 x the
    largest residual energy of the checker's last energy (tests/test_step_demo.py's bound and reasoning)."""
    names = ("scene", "two_frames")
    paths = []
    for name in names:
        job, frames = T.scene(name)
        paths.append(tmp_path / f"{name}.bin")
        T.write_case(paths[-1], R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "optimize_demo")
    out = subprocess.run([exe, str(paths[0]), str(paths[1]), "6"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("\n", res)
    assert res["windows_equal"] == 1 and res["decide_differently"] == 1
    hx = lambda a: f"{fnv1a(np.ascontiguousarray(a).tobytes()):016x}"  # noqa: E731
    for name, tag in zip(names, "ab"):
        job, _, exp = O.expected(name)
        last = float(exp["last_energy"][0]) + float(exp["last_energy"][1])
        want = dict(pattern=exp["pattern"], passes=exp["n_passes"], state=hx(np.asarray(exp["state"], f64)), calib=hx(np.asarray(exp["calib"], f64)),
                    idepth=hx(np.asarray(exp["idepth"], f32)), energy=hx(np.array([last], f64)))
        host = res[f"host_{tag}"]
        assert {k: v for k, v in host.items() if k != "last"} == want and host["last"] == last
        for form in (f"device_{tag}", f"many_{tag}"):
            assert res[form]["pattern"] == exp["pattern"] and res[form]["passes"] == exp["n_passes"]
            bound = len(job["point"]) * 2.0 ** -22 * 2500.0 * 8  # a residual's energy is at most 8 x outlierTHSumComponent = 8 x 2500
            print(f"{form} against checker: last energy differs by {abs(res[form]['last'] - last):.3g} (bound {bound:.3g})")
            assert abs(res[form]["last"] - last) <= bound
    assert res["device_a"]["pattern"] != res["device_b"]["pattern"]
