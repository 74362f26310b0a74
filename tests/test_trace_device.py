"""GPU: dsm_trace_points_batch against the checker tests/_trace_ref.py -- statuses, steps and counts exactly, every float bit for bit,
NaN payload aside.  Everything runs on the checker's 160 x 64 scene."""
import numpy as np
import pytest

import _trace_ref as R

pytestmark = pytest.mark.gpu


class Frames:
    """a KeyframeWindow holding the given planes under the ids 0, 1, ..."""

    def __init__(self, ctx, planes):
        from direct_stereo_slam_amd import immature

        self.win = immature.KeyframeWindow(ctx, R.W, R.H, len(planes))
        for k, p in enumerate(planes):
            self.win.put_host(k, p)

    def job(self, job, k=0):
        return dict(job, target=self.win, target_frame_id=k)

    def close(self):
        self.win.close()


@pytest.fixture(scope="module")
def frames(ctx):
    """the scenes' new frames on the device: seed 1, seed 2, and seed 1 moved sideways by one and two pixels"""
    t1, t2 = R.scene(seed=1)[1], R.scene(seed=2, n_random=60)[1]
    f = Frames(ctx, [t1, t2, R.sequence()[1][0], R.sequence()[2][0]])
    yield f
    f.close()


FRAME_OF_SEED = {1: 0, 2: 1}


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_checker(ctx, frames, name):
    from direct_stereo_slam_amd import trace

    job, _, exp, params = R.case(name)
    got = trace.trace_points_batch(ctx, [frames.job(job, FRAME_OF_SEED[R.CASES[name][0]["seed"]])], **params)[0]
    R.assert_equal(got, exp)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 65, 0])
def test_partial_groups_and_partial_waves(ctx, frames, n):
    """the first n points of the scene's narrowed and bordering points (searched, skipped and out of bounds mixed)"""
    from direct_stereo_slam_amd import trace

    job, _, exp, _ = R.case("defaults")
    idx = np.arange(152, 152 + n)
    got = trace.trace_points_batch(ctx, [frames.job(R.subset(job, idx))])[0]
    R.assert_equal(got, R.subset_result(exp, idx))
    assert len(got["status"]) == n and got["counts"].sum() == n


def test_one_wave_with_3_45_and_99_steps_and_early_exits(ctx, frames):
    """eight points = one wave, max_pix_search = 0.5 and min_improvement = 0 (no BADCONDITION exit): intervals of 1.76 and 43.5 px on
    the sideways host (3 and 45 steps), a fresh point (99 steps), and points that leave at T1, T2 and T3"""
    from direct_stereo_slam_amd import trace

    G, U, Q = R.GOOD, R.UNINITIALIZED, 2.0
    pts = [(0, 10, 30, G, 0.0, 1.76 / 16, Q, 0.0), (0, 12, 20, G, 0.0, 43.5 / 16, Q, 0.0), (0, 9, 40, U, 0.0, np.inf, 10000.0, 0.0),
           (0, 40, 30, R.OOB, 0.2, 0.3, Q, 0.0), (0, 50, 25, G, 0.25, 0.26, Q, 0.0), (0, 3, 30, U, 0.0, np.nan, 10000.0, 0.0),
           (0, 20, 44, G, 0.0, 43.5 / 16, Q, 0.0), (0, 30, 12, G, 0.0, 1.76 / 16, Q, 0.0)]
    job, target, _ = R.make_scene(seed=1, only=pts)
    assert np.array_equal(target, R.scene(seed=1)[1], equal_nan=True)
    params = dict(max_pix_search=0.5, min_improvement=0.0)
    exp = R.trace(R.W, R.H, target, job, **params)
    assert exp["steps"].tolist() == [3, 45, 99, 0, 0, 0, 45, 3] and exp["status"][3:6].tolist() == [R.OOB, R.SKIPPED, R.OOB]
    R.assert_equal(trace.trace_points_batch(ctx, [frames.job(job)], **params)[0], exp)


def test_mixed_batch_equals_each_job_alone(ctx, frames):
    """five jobs in one call at max_pix_search = 0.5: the whole scene (searches of 99 steps), narrowed points on the first three of its
    hosts, no hosts and no points, one host, and the scene of seed 2 against its own frame"""
    from direct_stereo_slam_amd import trace

    job, _, exp, params = R.case("wide")
    job2 = R.case("huber_4")[0]
    narrowed = np.flatnonzero((job["host"] < 3) & np.isfinite(job["idepth_max"]))
    one_host = np.flatnonzero(job["host"] == 0)[:21]
    empty = R.subset(job, np.arange(0), n_hosts=0)
    jobs = [frames.job(job), frames.job(R.subset(job, narrowed, n_hosts=3), 2), frames.job(empty, 3), frames.job(R.subset(job, one_host, n_hosts=1)),
            frames.job(job2, 1)]
    together = trace.trace_points_batch(ctx, jobs, **params)
    R.assert_equal(together[0], exp)
    assert len(together[2]["status"]) == 0 and (together[2]["counts"] == 0).all()
    assert together[0]["steps"].max() == 99 and together[1]["steps"].max() < 99
    for j, g in zip(jobs, together):
        alone = trace.trace_points_batch(ctx, [j], **params)[0]
        for k in alone:
            assert alone[k].tobytes() == g[k].tobytes(), k


def test_tracker_slot_and_window_frame_give_the_same(ctx, frames):
    from direct_stereo_slam_amd import synth, trace
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    job, target, exp, _ = R.case("defaults")
    trk = TrackerAndScaler(ctx, R.W, R.H, 3, synth.KITTI_T_STEREO, (R.FX, R.FY, R.CX, R.CY))
    trk.upload_intensity(1, [target] + [np.zeros((R.H >> l, R.W >> l), np.float32) for l in (1, 2)])
    from_slot = trace.trace_points_batch(ctx, [dict(job, target=trk, target_slot=1)])[0]
    from_window = trace.trace_points_batch(ctx, [frames.job(job)])[0]
    for k in from_slot:
        assert from_slot[k].tobytes() == from_window[k].tobytes(), k
    R.assert_equal(from_slot, exp)
    both = trace.trace_points_batch(ctx, [dict(job, target=trk, target_slot=1), frames.job(job)])  # and the two kinds in one call
    R.assert_equal(both[0], exp), R.assert_equal(both[1], exp)
    trk.close()


def test_three_frames_in_sequence(ctx, frames):
    """the outputs of one call are the inputs of the next: the checker run three times"""
    from direct_stereo_slam_amd import trace

    got = R.case("defaults")[0]
    for k, (_, _, exp) in zip((0, 2, 3), R.sequence()):
        res = trace.trace_points_batch(ctx, [frames.job(got, k)])[0]
        R.assert_equal(res, exp)
        got = R.advance(got, res)


def test_invalid_calls_are_refused_before_any_output_is_written(ctx, frames):
    from direct_stereo_slam_amd import immature, synth, trace
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler

    job, _, exp, _ = R.case("no_gn")
    good = frames.job(job, 1)
    trk = TrackerAndScaler(ctx, R.W, R.H, 3, synth.KITTI_T_STEREO, (R.FX, R.FY, R.CX, R.CY))  # nothing in its slots
    big = immature.KeyframeWindow(ctx, 176, 64, 1)
    big.put_host(0, np.zeros((64, 176), np.float32))
    other = Context(0)
    foreign = immature.KeyframeWindow(other, R.W, R.H, 1)
    foreign.put_host(0, R.scene(seed=1)[1])
    calls = [(what, [good, frames.job(bad, 1)], kw) for what, bad, kw in R.invalid_calls(job)]
    calls += [("an empty slot", [good, dict(job, target=trk, target_slot=0)], {}), ("slot 2", [good, dict(job, target=trk, target_slot=2)], {}),
              ("an id that is not in the window", [good, frames.job(job, 9)], {}), ("no target", [good, dict(job, target=None)], {}),
              ("mixed geometries", [good, dict(job, target=big, target_frame_id=0)], {}),
              ("a window of another context", [good, dict(job, target=foreign, target_frame_id=0)], {})]
    for what, jobs, kw in calls:
        b = trace.TraceBatch(jobs)
        before = [{k: v.copy() for k, v in st.items()} for st, _ in b.state]
        with pytest.raises(DsmError):
            b.run(ctx, trace.params(**kw))
        for (st, _), bef in zip(b.state, before):
            assert all(np.array_equal(st[k], bef[k], equal_nan=k != "status") for k in st), what
    b = trace.TraceBatch([good, good])  # both a tracker and a window
    b.arr[1].target_tracker = trk.h
    with pytest.raises(DsmError):
        b.run(ctx)
    assert (b.state[0][0]["steps"] == -1).all()
    R.assert_equal(trace.trace_points_batch(ctx, [good], gn_iterations=0)[0], exp)  # the window and the context are still usable
    foreign.close(), other.close(), big.close(), trk.close()
