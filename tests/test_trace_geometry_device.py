"""GPU: dsm_trace_points_batch against the checker tests/_trace_ref.py at 101 x 53 and at 24 x 20 -- statuses, steps and counts exactly,
every float bit for bit.  What the scene reaches there is asserted in tests/test_trace_geometry_ref.py on the checker alone."""
import numpy as np
import pytest

import _trace_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_device_equals_checker_from_a_window_and_from_a_tracker_slot(ctx, geom):
    from direct_stereo_slam_amd import immature, synth, trace
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    w, h = geom
    job, target, exp, _ = R.geometry_case(w, h)
    win = immature.KeyframeWindow(ctx, w, h, 1)
    win.put_host(0, target)
    R.assert_equal(trace.trace_points_batch(ctx, [dict(job, target=win, target_frame_id=0)])[0], exp)
    trk = TrackerAndScaler(ctx, w, h, 1, synth.KITTI_T_STEREO, (0.4 * w, 0.4 * w, (w - 1) / 2.0, (h - 1) / 2.0))
    trk.upload_intensity(0, [target])
    R.assert_equal(trace.trace_points_batch(ctx, [dict(job, target=trk, target_slot=0)])[0], exp)
    trk.close(), win.close()


@pytest.mark.parametrize("n", [1, 9, 63, 65])
def test_partial_waves_at_101_x_53(ctx, n):
    """the last n points of the scene: the points next to the four sides, kept and sent out by T2 in one wave"""
    from direct_stereo_slam_amd import immature, trace

    w, h = R.GEOMETRIES[0]
    job, target, exp, _ = R.geometry_case(w, h)
    idx = np.arange(len(job["host"]) - n, len(job["host"]))
    win = immature.KeyframeWindow(ctx, w, h, 1)
    win.put_host(0, target)
    got = trace.trace_points_batch(ctx, [dict(R.subset(job, idx), target=win, target_frame_id=0)])[0]
    R.assert_equal(got, R.subset_result(exp, idx))
    win.close()
