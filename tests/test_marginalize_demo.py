"""GPU: the C++ adaptor host/WindowMarginalize.hpp driven by host/marginalize_demo.cpp.  The chain of two keyframes -- optimize, the
request filled from the WindowOptimize's committed members, marginalise, the window shrunk, optimize on the returned prior -- through
the device forms and through the host forms, against the checkers' chain (tests/_marginalize_ref.py, keyframe_chain, on
tests/_optimize_ref.py).  And flagPointsForRemoval, marginalizePointsF and marginalizeFrame as ONE call for one window, for two
DIFFERENT windows in one call, and through the host form, against the checker, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import _linearize_ref as R
import _marginalize_ref as MR
import _step_ref as T
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def set_delta(job):
    """what MarginalizeRequest::setDeltaF forms for the demo's state, which stands off its zero state by 0.001 (1 + (7 frame + 3 k) mod 11)"""
    nf = len(job["frame_ids"])
    zero = np.full((nf, 8), 0.25)
    state = zero + 0.001 * np.array([[1 + (7 * i + 3 * k) % 11 for k in range(8)] for i in range(nf)], f64)
    return MR.set_delta(state - zero, np.array([10.001, 10.002, 5.003, 5.004]) - np.array([10.0, 10.0, 5.0, 5.0]), job["ad_host"], job["ad_target"])


def test_adaptor_one_window_two_different_windows_and_host_form(built, ctx, tmp_path):
    """every form's verdicts, returned prior and resInM equal the checker's bit for bit: window A (5 frames, one leaves) alone, A and B
    (9 frames, two leave) in one call, both through the host form; A's prior after the points and its res_toZeroF; setDeltaF"""
    names = ("scene", "nine_frames")
    paths = []
    for name in names:
        job, frames, _ = MR.case(name)
        paths.append(tmp_path / f"{name}.bin")
        MR.write_case(paths[-1], R.W, R.H, job, frames)
    step_job, step_frames = T.scene("scene")
    paths.append(tmp_path / "step_scene.bin")
    T.write_case(paths[-1], R.W, R.H, step_job, step_frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "marginalize_demo")
    out = subprocess.run([exe, str(paths[0]), str(paths[1]), str(paths[2]), "6"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("\n", res)
    assert res["windows_equal"] == 1 and res["device_equals_host"] == 1
    hx = lambda a, h=1469598103934665603: f"{fnv1a(np.ascontiguousarray(a).tobytes(), h):016x}"  # noqa: E731
    for name, tag in zip(names, "ab"):
        exp = MR.case(name)[2]
        want = dict(verdict=hx(exp["verdict"]), HM_out=hx(exp["H_M_out"]), bM_out=hx(exp["b_M_out"]), resInM=exp["n_res_marg"])
        for form in (f"device_{tag}", f"many_{tag}", f"host_{tag}"):
            assert res[form] == want, form
    assert res["device_a"] != res["device_b"]
    job, _, exp = MR.case("scene")
    assert res["points_prior_a"] == hx(exp["b_M_points"], fnv1a(np.ascontiguousarray(exp["H_M_points"]).tobytes()))
    rtz = np.where((exp["active"] == 1)[:, None], exp["res_to_zero"], f32(0.0)).astype(f32)  # the adaptor's room starts as zeros
    assert res["res_to_zero_a"] == hx(rtz)
    dp, cd = set_delta(job)
    assert res["set_delta_a"] == hx(cd, fnv1a(dp.tobytes()))
    # the chain of two keyframes.  The host forms equal the checkers' chain bit for bit (same C library).  The device forms take the
    # same decisions in both optimisations, give the same verdicts and counts, and end within n_res x 2^-22 x 20000 of the checkers'
    # last energy (tests/test_optimize_demo.py's bound and reasoning: a residual's energy is at most 8 x 2500).
    one, _, marg, two, _, fin = MR.keyframe_chain("scene", 6)
    last = float(fin["last_energy"][0]) + float(fin["last_energy"][1])
    assert (marg["verdict"] == MR.MARGINALIZE).sum() >= 5 and (marg["verdict"] == MR.DROP).sum() >= 1 and len(two["frame_ids"]) == 4
    want = dict(first=one["pattern"], second=fin["pattern"], verdict=hx(marg["verdict"]), HM_out=hx(marg["H_M_out"]), bM_out=hx(marg["b_M_out"]),
                resInM=marg["n_res_marg"], kept=len(two["host"]), residuals=len(two["point"]), state=hx(np.asarray(fin["state"], f64)),
                calib=hx(np.asarray(fin["calib"], f64)), idepth=hx(np.asarray(fin["idepth"], f32)), last=last)
    assert res["chain_host"] == want
    dev = res["chain_device"]
    assert all(dev[k] == want[k] for k in ("first", "second", "verdict", "resInM", "kept", "residuals")), (dev, want)
    bound = len(two["point"]) * 2.0 ** -22 * 2500.0 * 8
    print(f"device chain against the checkers': last energy differs by {abs(dev['last'] - last):.3g} (bound {bound:.3g}); "
          f"every hash equal: {dev == want}")
    assert abs(dev["last"] - last) <= bound
