"""GPU: the C++ adaptors host/WindowFinish.hpp and MarginalizeRequest::fromFinished (host/WindowMarginalize.hpp) driven by
host/finish_demo.cpp: the chain of two keyframes as makeKeyFrame runs it -- optimize + finish, shrink(), fromFinished, frame 1
marginalised, the window shrunk, optimize + finish on the returned prior -- through the device forms and through the host forms,
against the checkers' chain (tests/_finish_ref.py, checker_chain)."""
import json
import os
import subprocess

import numpy as np
import pytest

import _finish_ref as F
import _linearize_ref as R
from _window_files import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def hx(a, dtype):
    return f"{fnv1a(np.ascontiguousarray(a, dtype).tobytes()):016x}"


def decisions(fin):
    return dict(keep=hx(fin["keep"], np.uint8), states=hx(fin["new_state"], np.uint8), n_good=hx(fin["n_good_residuals_out"], np.int32),
                last_res=hx(fin["last_res_out"], np.int32), last_state=hx(fin["last_state_out"], np.uint8), dropped=hx(fin["point_dropped"], np.uint8),
                res_index=hx(fin["res_index_out"], np.int32), point_index=hx(fin["point_index_out"], np.int32), residuals=int(fin["n_res_out"]),
                points=int(fin["n_pts_out"]), lost=int(fin["lost"]))


def expected_chain(name="scene", max_iterations=6):
    """what finish_demo prints for a chain, from the checkers' chain"""
    c = F.checker_chain(name, max_iterations)
    marg, loop2, fin2 = c["marg"], c["loop2"], c["fin2"]
    return dict(first=c["loop"]["pattern"], second=loop2["pattern"], one=decisions(c["fin"]), two=decisions(fin2), verdict=hx(marg["verdict"], np.uint8),
                HM_out=hx(marg["H_M_out"], f64), bM_out=hx(marg["b_M_out"], f64), ad_ht_delta=hx(c["fin"]["ad_ht_delta_out"], f32),
                resInM=int(marg["n_res_marg"]), kept=len(c["two"]["host"]), residuals=len(c["two"]["point"]), state=hx(fin2["state_out"], f64),
                state_zero=hx(fin2["state_zero_out"], f64), eval=hx(fin2["world_to_cam_eval_out"], f64), calib=hx(loop2["calib"], f64),
                idepth=hx(loop2["idepth"], f32), last=float(loop2["last_energy"][0]) + float(loop2["last_energy"][1]), energy=float(fin2["energy"]),
                rmse=float(fin2["rmse"]))


def test_the_two_keyframe_chain_through_the_adaptors(built, ctx, tmp_path):
    """The host chain equals the checkers' chain bit for bit (same C library).  The device chain takes the same decisions in both
    finishes and in the marginalisation, and ends within n_res x 2^-22 x 20000 of the checkers' energies (section 20's bound)."""
    job, frames = F.scene("scene")
    path = tmp_path / "finish_scene.bin"
    F.write_case(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "finish_demo")
    out = subprocess.run([exe, str(path), "6"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    want = expected_chain("scene", 6)
    c = F.checker_chain("scene", 6)
    assert (c["fin"]["keep"] == 0).any() and c["fin"]["point_dropped"].any() and (c["marg"]["verdict"] == 1).any() and want["two"]["residuals"] > 0
    host = res["chain_host"]
    assert f32(host.pop("rmse")) == f32(want["rmse"])
    assert host == {k: v for k, v in want.items() if k != "rmse"}, {k: (host[k], want[k]) for k in host if host[k] != want[k]}
    dev = res["chain_device"]
    same = ("first", "second", "one", "two", "verdict", "resInM", "kept", "residuals")
    assert all(dev[k] == want[k] for k in same), {k: (dev[k], want[k]) for k in same if dev[k] != want[k]}
    assert res["decisions_equal"] == 1
    bound = want["residuals"] * 2.0 ** -22 * 2500.0 * 8
    print(f"\ndevice chain against the checkers': last energy differs by {abs(dev['last'] - want['last']):.3g}, the final linearisation's by "
          f"{abs(dev['energy'] - want['energy']):.3g} (bound {bound:.3g})")
    assert abs(dev["last"] - want["last"]) <= bound and abs(dev["energy"] - want["energy"]) <= bound
