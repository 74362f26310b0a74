"""GPU: the ICP fallback on the device (dsm_icp_batch) against the numpy checker of its contract (tests/_icp_ref.py):
integers exactly (pairs kept per search, iterations, end state, ok), tfm_target_source and the score to rounding; a job's bits do not
depend on the batch it runs in; the loop chain as LoopHandler runs it; the C++ adaptor's demo."""
import os
import re
import subprocess

import numpy as np
import pytest

import _icp_ref as R
from direct_stereo_slam_amd import icp as I
from direct_stereo_slam_amd._lib import DsmError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_matches_checker(got, src, tgt, guess, **params):
    want = R.icp(src, tgt, guess, **params)
    if want["state"] != R.EMPTY:
        assert abs(float(want["score"]) / 1.5 - 1) > 1e-3, "scene too close to ICP_THRES for an exact `ok` comparison"
    assert got["state"] == want["state"] and got["iterations"] == want["iterations"], (got, want)
    assert got["corr_counts"] == want["corr_counts"] and got["ok"] == want["ok"], (got, want)
    np.testing.assert_allclose(got["tfm"][:3, :3], want["tfm"][:3, :3], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["tfm"][:3, 3], want["tfm"][:3, 3], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(got["tfm"][3], want["tfm"][3])
    if want["state"] == R.EMPTY:
        assert got["score"] == np.inf
    else:
        assert abs(float(got["score"]) - float(want["score"])) <= 1e-5 * float(want["score"]), (got["score"], want["score"])
    return want


def _scenes():
    guess = R.rigid(R.rot((0.0, 0.01, 0.0)), [0.05, 0.0, 0.0])
    small = R.scene(1, 2000)
    large = R.blobs(3, 2000, (0, 0.1, 0), (1.5, 0.5, 0))
    pts = np.random.default_rng(1).normal(0, 3, (500, 3))
    tie_src, tie_tgt, _ = R.ties(7)
    return {
        "small_motion": (small[0], small[1], np.eye(4)),
        "small_motion_with_guess": (small[0], small[1], guess),
        "large_motion": (large[0], large[1], np.eye(4)),
        "far_apart": (pts, pts + np.array([20.0, 0.0, 3.0]), guess),
        "equidistant_targets": (tie_src, tie_tgt, np.eye(4)),
        "empty_source": (pts[:0], pts, guess),
        "empty_target": (pts, pts[:0], guess),
        "two_points": (pts[:2], pts, np.eye(4)),
    }


@pytest.mark.parametrize("name", list(_scenes()))
def test_scene_equals_checker(ctx, name):
    src, tgt, guess = _scenes()[name]
    got = I.icp(ctx, src, tgt, guess)
    want = assert_matches_checker(got, src, tgt, guess)
    expected_state = {"small_motion": R.TRANSFORM, "large_motion": R.ITERATIONS, "far_apart": R.NO_CORRESPONDENCES, "empty_source": R.EMPTY,
                      "empty_target": R.EMPTY, "two_points": R.NO_CORRESPONDENCES}.get(name)
    if expected_state is not None:
        assert got["state"] == expected_state
    if name == "large_motion":
        assert got["iterations"] == 5
    if name in ("far_apart", "empty_source", "empty_target"):
        assert not got["ok"] and np.array_equal(got["tfm"], guess) and want["iterations"] == 0


@pytest.mark.parametrize("seed", [7, 8])
def test_exact_ties_go_to_the_smallest_target_index(ctx, seed):
    """D2: every source point has two distinct targets at exactly the same float distance; which one wins changes the first
    increment's cross-covariance.  The device must take the smaller index -- inside one LDS tile and across target slices."""
    src, tgt, tgt_swapped = R.ties(seed)
    for t in (tgt, tgt_swapped):
        got = I.icp(ctx, src, t, np.eye(4))
        want = assert_matches_checker(got, src, t, np.eye(4))
        other = R.icp(src, tgt_swapped if t is tgt else tgt, np.eye(4))  # the result the larger index would give
        assert np.abs(want["tfm"][:3, 3] - other["tfm"][:3, 3]).max() > 0.1
        assert np.abs(got["tfm"][:3, 3] - other["tfm"][:3, 3]).max() > 0.1


def test_constructed_end_states_and_parameters(ctx):
    pts = np.random.default_rng(1).normal(0, 3, (500, 3))
    got = I.icp(ctx, pts, pts, np.eye(4), transformation_epsilon=-1.0)  # no transformation test: the MSE repeats
    assert got["state"] == R.ABS_MSE and got["score"] == 0
    assert_matches_checker(got, pts, pts, np.eye(4), eps=-1.0)
    src, tgt, T = R.scene(5, 3000, rotvec=(0.01, 0.03, 0.0), trans=(0.3, 0.05, 0.2), overlap=0.7)
    got = I.icp(ctx, src, tgt, np.eye(4), max_iterations=40, transformation_epsilon=1e-8)
    assert_matches_checker(got, src, tgt, np.eye(4), max_iterations=40, eps=1e-8)
    ang, tr = R.pose_error(got["tfm"], T)
    assert got["state"] == R.TRANSFORM and ang < 0.1 and tr < 0.05


@pytest.mark.parametrize("n_src,n_tgt", [(2000, 2500), (10000, 9000), (20000, 20000)])
def test_large_clouds_equal_checker(ctx, n_src, n_tgt):
    src, tgt, _ = R.scene(11 + n_src, n_src, n_tgt=n_tgt, rotvec=(0.0, 0.04, 0.01), trans=(0.3, 0.0, 0.4))
    guess = R.rigid(R.rot((0.0, 0.02, 0.0)), [0.1, 0.0, 0.2])
    assert_matches_checker(I.icp(ctx, src, tgt, guess), src, tgt, guess)


def _mixed_jobs():
    sizes = [0, 1, 2, 3, 40, 300, 1000, 2000, 5000, 9000, 20000]
    jobs = []
    for j in range(64):
        n_src, n_tgt = sizes[j % len(sizes)], sizes[(3 * j + 5) % len(sizes)]
        if j % 7 == 0:
            src, tgt, _ = R.blobs(j, max(n_src, 1), (0, 0.1, 0), (1.5, 0.5, 0))
        else:
            src, tgt, _ = R.scene(100 + j, max(n_src, 1), n_tgt=max(n_tgt, 1))
        jobs.append((src[:n_src], tgt[:n_tgt], R.rigid(R.rot((0.0, 0.002 * j, 0.0)), [0.01 * j, 0.0, 0.0])))
    return jobs


def test_batch_results_are_bit_identical_to_single_calls(ctx):
    jobs = _mixed_jobs()
    batch = I.IcpBatch(ctx, jobs)
    batch.run()
    first = batch.results()
    batch.run()
    again = batch.results()
    for j, (a, b) in enumerate(zip(first, again)):
        assert a["tfm"].tobytes() == b["tfm"].tobytes() and a["score"].tobytes() == b["score"].tobytes() and a["corr_counts"] == b["corr_counts"], j
    for j in list(range(0, 64, 5)) + [63]:
        alone = I.icp(ctx, *jobs[j])
        assert alone["tfm"].tobytes() == first[j]["tfm"].tobytes(), j
        assert alone["score"].tobytes() == first[j]["score"].tobytes(), j
        assert (alone["ok"], alone["state"], alone["iterations"], alone["corr_counts"]) == \
            (first[j]["ok"], first[j]["state"], first[j]["iterations"], first[j]["corr_counts"]), j
    # and the batch against the checker, on the jobs small enough for numpy
    for j in (1, 4, 7, 14, 15, 16, 22, 28):
        assert_matches_checker(first[j], *jobs[j])


def test_invalid_calls_write_nothing(ctx):
    from direct_stereo_slam_amd._lib import check

    pts = np.random.default_rng(2).normal(0, 3, (300, 3))
    good = (pts, pts + 0.1, np.eye(4))
    bad_guess = np.eye(4)
    bad_guess[0, 3] = np.nan
    for jobs, params in (([good, (pts, pts, bad_guess)], {}), ([good, (pts, pts, np.eye(4))], dict(max_iterations=0)),
                         ([good], dict(max_iterations=65)), ([good], dict(max_corr_dist=-1.0)), ([good], dict(transformation_epsilon=np.inf))):
        b = I.IcpBatch(ctx, jobs, **params)
        b.outs[0]["tfm"][...] = 7.0
        b.outs[0]["score"][0] = -3.0
        with pytest.raises(DsmError):
            check(ctx.L.dsm_icp_batch(ctx.h, len(b.arr), b.arr, *b.params))
        assert np.all(b.outs[0]["tfm"] == 7.0) and b.outs[0]["score"][0] == -3.0
    b = I.IcpBatch(ctx, [good, good])
    b.arr[1].n_src = -1
    with pytest.raises(DsmError):
        check(ctx.L.dsm_icp_batch(ctx.h, 2, b.arr, *b.params))
    assert b.outs[0]["score"][0] == 0


def _place(seed, n_pts=20000):
    """one place seen from two nearby camera poses: the keyframes' jobs for loop_descriptors_batch and the true T_cur_matched"""
    rng = np.random.default_rng(seed)
    world = R.street(rng, n_pts)
    T_cur_matched = R.rigid(R.rot((0.0, 0.05, 0.0)), [0.4, 0.0, 1.2])
    kf_ids = np.array([100, 101])
    pt_kf = rng.choice(kf_ids, n_pts)
    matched = (kf_ids, np.zeros((2, 6)), np.hstack([np.eye(3), np.zeros((3, 1))]), pt_kf, world)
    cur = (kf_ids, np.zeros((2, 6)), T_cur_matched[:3], pt_kf, world)
    return matched, cur, T_cur_matched


def test_loop_chain_as_loophandler_runs_it(ctx):
    from direct_stereo_slam_amd.ringdb import loop_descriptors_batch

    for seed in range(3):
        matched_job, cur_job, T_true = _place(seed)
        matched, cur = loop_descriptors_batch(ctx, [matched_job, cur_job], 40.0)
        guess = np.linalg.inv(cur["tfm_pca_rig"]) @ matched["tfm_pca_rig"]  # LoopHandler.cpp:266-268
        got = I.icp(ctx, matched["pts_spherical"], cur["pts_spherical"], guess)
        assert_matches_checker(got, matched["pts_spherical"], cur["pts_spherical"], guess)
        assert got["ok"]
        ang, tr = R.pose_error(got["tfm"], T_true)
        ang0, tr0 = R.pose_error(guess, T_true)
        assert ang < 0.2 and tr < 0.1, (ang, tr)  # within 0.2 degrees and 10 cm of the truth
        assert tr < tr0


def test_cpp_demo_equals_python_path(ctx, tmp_path):
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "icp_demo")
    assert os.path.exists(exe)
    jobs = [_scenes()[k] for k in ("small_motion_with_guess", "large_motion", "far_apart", "empty_target")]
    jobs.append(R.scene(21, 6000, n_tgt=5000)[:2] + (np.eye(4),))
    blob = bytearray(np.int32(len(jobs)).tobytes())
    for src, tgt, guess in jobs:
        src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
        blob += np.array([len(src), len(tgt)], np.int32).tobytes() + np.asarray(guess, np.float64).tobytes() + src.tobytes() + tgt.tobytes()
    path = tmp_path / "matches.bin"
    path.write_bytes(bytes(blob))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"matches={len(jobs)} mismatches=0" in out.stdout
    py = I.icp_batch(ctx, jobs)
    lines = re.findall(r"match (\d+) ok=(\d) state=(\d+) iterations=(\d+) score=(\S+) tfm=(\S+)", out.stdout)
    assert len(lines) == len(jobs)
    for (j, ok, state, it, score, tfm), r in zip(lines, py):
        assert (bool(int(ok)), int(state), int(it)) == (r["ok"], r["state"], r["iterations"]), j
        assert np.float32(float(score)) == r["score"] or (r["score"] == np.inf and score == "inf"), j
        assert np.array_equal(np.array([float(x) for x in tfm.split(",")]).reshape(4, 4), r["tfm"]), j
