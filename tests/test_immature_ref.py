"""CPU: the host form dsm_optimize_immature_points_host against the checker tests/_immature_ref.py, bit for bit (DESIGN.md section 13,
M1-M8, U1-U9): the 96 x 64 scene for min_obs 1 and 3, windows of 1, 2 and 9 frames, gn_iterations 0, no points; the branches the scene
must reach, asserted on the checker's output alone; the invalid calls."""
import numpy as np
import pytest

import _immature_ref as R


def test_scene_reaches_every_branch():
    """on the checker's output alone: a form that skips a branch cannot equal it"""
    _, _, exp, _ = R.case("scene")
    tr = exp["trace"]
    counts = dict(activated=int((exp["status"] == 1).sum()), status_0=int((exp["status"] == 0).sum()),
                  accepted_steps=tr["accepted"], rejected_steps=tr["rejected"], oob_after_nonzero_partial_sum=tr["oob_after_partial_sum"],
                  non_finite_sample_oob=tr["oob_non_finite_sample"], entered_oob=tr["entered_oob"], return0_first_pass=tr["return0_first_pass"],
                  return0_inside_loop=tr["return0_in_loop"], convergence_breaks=tr["convergence_break"], clamped=tr["clamped"],
                  final_in=int((exp["res_state"] == R.IN).sum()), final_outlier=int((exp["res_state"] == R.OUTLIER).sum()),
                  final_oob=int((exp["res_state"] == R.OOB).sum()), deleted_min_obs_1=int((exp["status"] == 2).sum()))
    _, _, exp3, _ = R.case("scene_min_obs_3")
    counts["deleted_min_obs_3"] = int((exp3["status"] == 2).sum())
    counts["hosts_used"] = 5 * len(set(R.case("scene")[0]["host"].tolist()))
    print(counts)
    assert all(v >= 5 for v in counts.values()), counts
    assert counts["deleted_min_obs_3"] > counts["deleted_min_obs_1"]
    assert set(exp["iterations"].tolist()) == {0, 1, 2, 3}  # the loop is left after every number of trials
    assert (exp["res_state"] == R.HOST).sum() == len(exp["status"])  # one host column per point


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_form_equals_checker(built, name):
    from direct_stereo_slam_amd import immature

    job, frames, exp, its = R.case(name)
    got = immature.optimize_immature_points_host(R.W, R.H, job, frames, gn_iterations=its)
    R.assert_equal(got, exp)
    n_res = len(job["frame_ids"]) - 1
    if n_res == 0:
        assert (got["status"] == 0).all() and (got["hdd"] == 0).all()  # no residuals: Hdd = 0
    if its == 0:
        assert (got["iterations"] == 0).all()


def test_host_form_with_other_thresholds(built):
    """huber_th, min_idepth_h_act and gn_iterations are read, not assumed"""
    from direct_stereo_slam_amd import immature

    job, frames, exp_default, _ = R.case("no_iterations")
    kw = dict(huber_th=np.float32(4.0), min_idepth_h_act=np.float32(400.0), gn_iterations=6)
    exp = R.optimize(R.W, R.H, job, frames, **kw)
    assert exp["iterations"].max() > 3 and not np.array_equal(exp["status"], exp_default["status"])
    R.assert_equal(immature.optimize_immature_points_host(R.W, R.H, job, frames, **kw), exp)


def test_host_form_refuses_invalid_calls_and_writes_nothing(built):
    from direct_stereo_slam_amd import _lib, immature
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, _, _ = R.case("two_frames")
    for what, bad, kw in R.invalid_jobs(job):
        b = immature.ImmatureBatch([bad])
        before = [{k: v.copy() for k, v in out.items()} for out, _ in b.outs]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, **kw)
        for (out, _), bef in zip(b.outs, before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    # n_frames outside [1, 9] and a NULL array, on the C structure itself
    b = immature.ImmatureBatch([job])
    for n_frames in (0, 10):
        b.arr[0].n_frames = n_frames
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames)
    b.arr[0].n_frames = 2
    b.arr[0].weights = None
    with pytest.raises(DsmError):
        b.run_host(R.W, R.H, 0, frames)
    b.arr[0].weights = b.keep[0][5].ctypes.data_as(_lib.c_float_p)
    b.arr[0].n_pts = -1
    with pytest.raises(DsmError):
        b.run_host(R.W, R.H, 0, frames)
    assert (b.outs[0][0]["status"] == 77).all()  # the sentinel the mirror fills the outputs with
