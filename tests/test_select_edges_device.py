"""GPU: dsm_select_pixels_batch against the checker tests/_select_ref.py at remainder sizes, at the two camera sizes of
tests/golden/cams and at the potential cap -- the map, the counts, the passes, the new potential and every point array exactly, floats
bit for bit.  What these shapes reach is asserted in tests/test_select_edges_ref.py on the checker alone."""
import numpy as np
import pytest

import _select_ref as R

pytestmark = pytest.mark.gpu


class Rig:
    """per shape: a tracker with the scene in slot 0, and a selector for four jobs"""

    def __init__(self, ctx, shape):
        from direct_stereo_slam_amd import pixelselect, synth
        from direct_stereo_slam_amd.tracker import TrackerAndScaler

        w, h = shape
        self.trk = TrackerAndScaler(ctx, w, h, 3, synth.KITTI_T_STEREO, (100.0, 100.0, w / 2.0, h / 2.0))
        self.trk.upload_image(0, R.scene(w, h))
        self.sel = pixelselect.PixelSelector(ctx, w, h, 4, R.pattern(w, h))

    def job(self, case, **more):
        return R.edge_job_of(case, tracker=self.trk, slot=0, **more)

    def close(self):
        self.sel.close(), self.trk.close()


@pytest.fixture(scope="module")
def rigs(ctx):
    r = {shape: Rig(ctx, shape) for shape in R.EDGE_SHAPES + R.CAMERA_SHAPES}
    yield r
    for x in r.values():
        x.close()


@pytest.mark.parametrize("shape", R.EDGE_SHAPES + R.CAMERA_SHAPES)
def test_tracker_levels_are_the_checkers_pyramid(rigs, shape):
    """before anything is compared: a difference in levels 1 and 2 (odd sizes drop a column or a row) would not be the selector's"""
    for lvl, plane in enumerate(R.pyramid(R.scene(*shape))):
        got = rigs[shape].trk.get_frame(0, lvl)[..., 0]
        assert got.shape == plane.shape and np.array_equal(got.view(np.uint32), plane.view(np.uint32)), lvl


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_device_equals_checker(rigs, name):
    from direct_stereo_slam_amd import pixelselect

    case = R.EDGE_CASES[name]
    rig = rigs[case["shape"]]
    got = pixelselect.select_pixels_batch(rig.sel, [rig.job(case)], **case["params"])[0]
    R.assert_equal(got, R.edge_expected(name))


def test_a_job_without_point_arrays_alone_and_second_in_a_batch(rigs):
    """max_pts = 0 and NULL point arrays: counts, map and n_pts as the checker's, and the job before it keeps every point"""
    from direct_stereo_slam_amd import pixelselect

    case, exp = R.EDGE_CASES["no_point_arrays"], R.edge_expected("no_point_arrays")
    w, h = case["shape"]
    rig = rigs[(w, h)]
    alone = pixelselect.SelectBatch([rig.job(case)], w, h)
    R.null_point_arrays(alone, 0)
    alone.run(rig.sel)
    R.assert_equal(alone.results()[0], exp)
    first = f"{w}x{h}-down"
    assert R.EDGE_CASES[first]["params"] == case["params"] == {}
    both = pixelselect.SelectBatch([rig.job(R.EDGE_CASES[first]), rig.job(case)], w, h)
    R.null_point_arrays(both, 1)
    both.run(rig.sel)
    got = both.results()
    R.assert_equal(got[0], R.edge_expected(first)), R.assert_equal(got[1], exp)
    assert got[1]["n_pts"] == exp["n_pts"] >= 100 and len(got[1]["u"]) == 0


def test_four_potentials_in_one_call_in_two_orders(rigs):
    """1226 x 370, entering at 1, 3, 4096 and 5: every job equals the checker's, whichever job it is in the call"""
    from direct_stereo_slam_amd import pixelselect

    rig = rigs[R.CAMERA_SHAPES[1]]
    jobs = [rig.job(R.EDGE_CASES[n]) for n in R.BATCH_OF_FOUR]
    for order in ([0, 1, 2, 3], [2, 3, 1, 0]):
        got = pixelselect.select_pixels_batch(rig.sel, [jobs[k] for k in order], recursions=1)
        for k, g in zip(order, got):
            R.assert_equal(g, R.batch_expected(R.BATCH_OF_FOUR[k], 1))
