"""GPU: dsm_optimize_immature_points_batch against the checker tests/_immature_ref.py at 101 x 53 with nine frames -- status, states
and iterations exactly, idepth, Hdd, bd and energy bit for bit.  What the window reaches is asserted in
tests/test_immature_geometry_ref.py on the checker alone."""
import pytest

import _immature_ref as R

pytestmark = pytest.mark.gpu


def test_device_equals_checker_alone_and_twice_in_a_batch(ctx):
    from direct_stereo_slam_amd import immature

    w, h = R.GEOMETRY
    job, frames, exp = R.geometry_case()
    wins = [immature.KeyframeWindow(ctx, w, h, len(frames)) for _ in range(2)]
    for win in wins:
        for fid, img in zip(job["frame_ids"], frames):
            win.put_host(int(fid), img)
    R.assert_equal(immature.optimize_immature_points_batch(ctx, [dict(job, window=wins[0])])[0], exp)
    for got in immature.optimize_immature_points_batch(ctx, [dict(job, window=wins[0]), dict(job, window=wins[1])]):
        R.assert_equal(got, exp)
    for win in wins:
        win.close()
