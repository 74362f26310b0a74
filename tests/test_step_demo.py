"""GPU: the C++ adaptor host/WindowStep.hpp driven by host/step_demo.cpp through the loop of FrontEnd::optimize (lambda 0.1, x 0.25 on
an accepted step, x 100 on a rejected one): one window, two windows in one call per iteration, and the host form, against the same
loop over the checker tests/_step_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
import _step_ref as T
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def optimize_ref(job, frames, max_its):
    """step_demo.cpp's loop over the checker: (pattern, state, calib, idepth, last energy, the energies of every call)"""
    n = len(job["frame_ids"])
    cur = dict(job, fix_linearization=0, frame_step=np.zeros((n, 8)), calib_step=np.zeros(4), idepth_step=np.zeros(len(job["host"]), f32),
               frame_energy_th=np.array(job["frame_energy_th"], f32, copy=True))
    energies = []

    def call(fac, lam):
        res = T.run(dict(cur, stepfac=np.array(fac, f32), **{"lambda": lam}), frames)
        cur["frame_energy_th"] = cur["frame_energy_th"].copy()
        cur["frame_energy_th"][-1] = res["new_frame_energy_th"]
        energies.append(float(res["energy"]) + float(res["energy_m"]))
        return res

    def accept(res):
        cur.update(state_backup=res["state"], calib_backup=res["calib"], idepth_backup=res["idepth"], state_in=res["new_state"],
                   energy_in=res["new_energy"], frame_step=-res["x"][4:].reshape(n, 8), calib_step=-res["x"][:4], idepth_step=res["step"])
        return float(res["energy"]) + float(res["energy_m"])

    zero, one, lam, pattern = [0.0] * 5, [1.0] * 5, 1e-1, ""
    last = accept(call(zero, lam))
    for it in range(max_its):
        res = call(one, lam * 0.25)
        if float(res["energy"]) + float(res["energy_m"]) < last:
            last, lam, pattern = accept(res), lam * 0.25, pattern + "A"
        else:
            lam *= 1e2
            last, pattern = accept(call(zero, lam)), pattern + "R"
        if res["can_break"] and it >= 1:
            break
    return pattern, cur["state_backup"], cur["calib_backup"], cur["idepth_backup"], last, energies


def test_adaptor_loop_one_window_two_windows_and_host_form(built, ctx, tmp_path):
    """The host form's loop equals the checker's bit for bit (same C library).  The device's equals its own two-window run bit for
    bit, takes the same accept / reject decisions as the checker, and ends within n_res x 2^-22 x the largest residual energy of the
    checker's last energy: the device's sincos and exp may differ from the C library's in the last place, which moves a pose by
    parts in 1e15 and can move each residual's float energy by an ulp or two, no more."""
    job, frames = T.scene("scene")
    path = tmp_path / "step.bin"
    T.write_case(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "step_demo")
    out = subprocess.run([exe, str(path), "6"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    pattern, state, calib, idepth, last, energies = optimize_ref(job, frames, 6)
    print("\n", res, pattern, last, energies)
    assert "A" in pattern and len(pattern) >= 2
    assert res["windows_equal"] == 1 and res["n_res"] == len(job["point"])
    assert res["stale_step_refused"] == 2  # non-zero factors before the first accept, and after a reject
    hx = lambda a: f"{fnv1a(np.ascontiguousarray(a).tobytes()):016x}"  # noqa: E731
    want = dict(pattern=pattern, state=hx(np.asarray(state, f64)), calib=hx(np.asarray(calib, f64)), idepth=hx(np.asarray(idepth, f32)),
                energy=hx(np.array([last], f64)))
    assert {k: v for k, v in res["host"].items() if k != "last"} == want and res["host"]["last"] == last
    assert res["device"]["pattern"] == pattern
    bound = len(job["point"]) * 2.0 ** -22 * 2500.0 * 8  # a residual's energy is at most 8 x outlierTHSumComponent = 8 x 2500
    print(f"device against checker: last energy differs by {abs(res['device']['last'] - last):.3g} (bound {bound:.3g}); "
          f"device_equals_host {res['device_equals_host']}")
    assert abs(res["device"]["last"] - last) <= bound
