"""GPU: the C++ adaptor host/WindowRescale.hpp driven by host/rescale_demo.cpp: a stereo keyframe as makeKeyFrame runs it -- optimize +
finish, shrink(), the rescale call, MarginalizeRequest::fromFinished + applyTo, frame 1 marginalised, the nullspaces -- with the scale
accepted, rejected and disabled, through the device form and through the host form of the call, and without the call."""
import json
import os
import subprocess

import pytest

import _finish_ref as F
import _linearize_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = ("idepth", "eval", "state", "tables", "ad_ht_delta", "verdict", "H_M_out", "b_M_out", "resInM", "null_basis", "null_pinv", "rank")


def test_a_stereo_keyframe_through_the_adaptors(built, ctx, tmp_path):
    job, frames = F.scene("scene")
    path = tmp_path / "finish_scene.bin"
    F.write_case(path, R.W, R.H, job, frames)
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "rescale_demo")
    out = subprocess.run([exe, str(path), "1.4", "6"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["forms_equal"] == 1 and res["windows_equal"] == 1
    dev, host, none = res["device"], res["host"], res["none"]
    assert dev == host  # the device and host chains give equal hashes
    assert [dev[k]["decision"] for k in ("accepted", "rejected", "disabled")] == [2, 1, 0]
    acc = dev["accepted"]
    assert acc["H_M_out"] != dev["rejected"]["H_M_out"] and acc["idepth"] != none["idepth"] and acc["eval"] != none["eval"]
    assert acc["tables"] != none["tables"] and acc["null_basis"] != none["null_basis"] and acc["rank"] == 7
    assert (acc["trapped"], acc["fails"], acc["scale_error"], acc["applied_scale"]) == (1, 0, 0.5, pytest.approx(1.4, abs=1e-6))
    for k, words in (("rejected", (0, 1, 2.0, 1.0)), ("disabled", (0, 0, -1.0, 1.0))):  # the chain without the call
        assert {w: dev[k][w] for w in WINDOW} == {w: none[w] for w in WINDOW}, k
        assert (dev[k]["trapped"], dev[k]["fails"], dev[k]["scale_error"], dev[k]["applied_scale"]) == words
    # S1 through a ScaleState: accept (trapped), trapped jump, five more rejections of which the last untraps and returns -1, accept
    assert res["sequence"] == "AtRtRtRtRtRtUgAt"
