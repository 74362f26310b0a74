"""GPU: dsm_window_* and dsm_optimize_immature_points_batch against the checker tests/_immature_ref.py -- status, states and iterations
exactly, idepth, Hdd, bd and energy bit for bit."""
import numpy as np
import pytest

import _immature_ref as R

pytestmark = pytest.mark.gpu


def window_of(ctx, job, frames, capacity=None):
    from direct_stereo_slam_amd import immature

    win = immature.KeyframeWindow(ctx, R.W, R.H, capacity or len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


def run(ctx, cases, **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import immature

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    res = immature.optimize_immature_points_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], **kw)
    for win in wins:
        win.close()
    return res


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_checker(ctx, name):
    """5 frames: four residuals, half a wave; 9 frames: eight residuals, all 64 lanes; 1 frame: no residual at all"""
    job, frames, exp, its = R.case(name)
    if name == "nine_frames":
        assert len(frames) == 9 and (exp["res_state"] != R.OOB).all(axis=1).any()  # a point whose eight residuals all count
    R.assert_equal(run(ctx, [(job, frames)], gn_iterations=its)[0], exp)


def test_other_thresholds(ctx):
    job, frames, _, _ = R.case("no_iterations")
    kw = dict(huber_th=np.float32(4.0), min_idepth_h_act=np.float32(400.0), gn_iterations=6)
    R.assert_equal(run(ctx, [(job, frames)], **kw)[0], R.optimize(R.W, R.H, job, frames, **kw))


def test_mixed_batch_equals_each_job_alone(ctx):
    """jobs of 5, 1, 9, 3 (no points), 2 and again 5 frames in one call: every job as the checker has it, and as the job alone"""
    names = ["scene", "one_frame", "nine_frames", "no_points", "two_frames", "scene_min_obs_3"]
    cs = [R.case(n) for n in names]
    together = run(ctx, [(c[0], c[1]) for c in cs])
    for n, c, g in zip(names, cs, together):
        R.assert_equal(g, c[2])
        alone = run(ctx, [(c[0], c[1])])[0]
        for k in R.FIELDS_BITS + R.FIELDS_EXACT:
            assert alone[k].tobytes() == g[k].tobytes(), (n, k)
    assert len(together[3]["status"]) == 0


def test_one_window_serves_several_jobs_and_slots_are_reused(ctx):
    """drop / put: a frame's place is taken by the next frame; a window of capacity 6 holding the scene's five frames in another
    order than the job lists them, and two jobs on it in one call"""
    from direct_stereo_slam_amd import immature
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp, _ = R.case("scene")
    job3, _, exp3, _ = R.case("scene_min_obs_3")
    ids = [int(i) for i in job["frame_ids"]]
    win = immature.KeyframeWindow(ctx, R.W, R.H, 6)
    junk = np.full((R.H, R.W), 7.0, np.float32)
    for fid in (1, 2, 3, 4, 5, 6):
        win.put_host(fid, junk + fid)
    with pytest.raises(DsmError):
        win.put_host(ids[0], frames[0])  # full
    with pytest.raises(DsmError):
        win.drop(99)  # unknown
    for fid, new in zip((3, 1, 6, 2, 5), (4, 2, 0, 3, 1)):  # the job's frames arrive out of order, each into a freed place
        win.drop(fid)
        win.put_host(ids[new], frames[new])
    with pytest.raises(DsmError):
        win.put_host(ids[2], frames[2])  # duplicate
    with pytest.raises(DsmError):
        win.get(3)  # dropped
    assert np.array_equal(win.get(4), junk + 4)
    for fid, img in zip(ids, frames):
        assert np.array_equal(win.get(fid), img, equal_nan=True)
    res = immature.optimize_immature_points_batch(ctx, [dict(job, window=win), dict(job3, window=win)])
    R.assert_equal(res[0], exp)
    R.assert_equal(res[1], exp3)
    win.close()


def test_put_from_tracker_equals_put_host(ctx):
    """geometry 96 x 64, 3 levels: level 0 of a frame handed to a tracker slot, copied on the device"""
    from direct_stereo_slam_amd import immature, synth
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    job, frames, exp, _ = R.case("scene")
    ids = [int(i) for i in job["frame_ids"]]
    trk = TrackerAndScaler(ctx, R.W, R.H, 3, synth.KITTI_T_STEREO, R.CAM)
    other = TrackerAndScaler(ctx, 128, 64, 3, synth.KITTI_T_STEREO, R.CAM)
    win = immature.KeyframeWindow(ctx, R.W, R.H, 5)
    with pytest.raises(DsmError):
        win.put_from_tracker(ids[0], trk, 0)  # nothing in the slot yet
    other.upload_image(0, np.zeros((64, 128), np.float32))
    with pytest.raises(DsmError):
        win.put_from_tracker(ids[0], other, 0)  # another geometry
    for k, (fid, img) in enumerate(zip(ids, frames)):
        trk.upload_image(k & 1, img)
        win.put_from_tracker(fid, trk, k & 1)
        assert np.array_equal(win.get(fid), img, equal_nan=True)
    with pytest.raises(DsmError):
        win.put_from_tracker(ids[1], trk, 0)  # duplicate id
    R.assert_equal(immature.optimize_immature_points_batch(ctx, [dict(job, window=win)])[0], exp)
    win.close(), trk.close(), other.close()


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import immature
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp, _ = R.case("two_frames")
    win = window_of(ctx, job, frames)
    big = immature.KeyframeWindow(ctx, 128, 64, 2)
    for fid in job["frame_ids"]:
        big.put_host(int(fid), np.zeros((64, 128), np.float32))
    good = dict(job, window=win)
    calls = [(what, [good, dict(bad, window=win)], kw) for what, bad, kw in R.invalid_jobs(job)]
    calls.append(("a frame id that is not in the window", [good, dict(job, window=win, frame_ids=np.array([100, 555], np.int32))], {}))
    calls.append(("mixed geometries", [good, dict(job, window=big)], {}))
    calls.append(("no window", [good, dict(job, window=None)], {}))
    for what, jobs, kw in calls:
        b = immature.ImmatureBatch(jobs)
        before = [{k: v.copy() for k, v in out.items()} for out, _ in b.outs]
        with pytest.raises(DsmError):
            b.run(ctx, **kw)
        for (out, _), bef in zip(b.outs, before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    b = immature.ImmatureBatch([good, good])
    for n_frames in (0, 10):
        b.arr[1].n_frames = n_frames
        with pytest.raises(DsmError):
            b.run(ctx)
    b.arr[1].n_frames = 2
    b.arr[1].color = None
    with pytest.raises(DsmError):
        b.run(ctx)
    assert all((out["status"] == 77).all() for out, _ in b.outs)
    with pytest.raises(DsmError):
        immature.KeyframeWindow(ctx, R.W, R.H, 17)
    R.assert_equal(immature.optimize_immature_points_batch(ctx, [good])[0], exp)  # the window and the context are still usable
    win.close(), big.close()
