"""GPU: dsm_select_pixels_batch against the checker tests/_select_ref.py -- the map, the counts, the passes, the new potential and every
point array exactly, floats bit for bit, NaN patterns included.  The frames are handed to a tracker as
level-0 images; levels 1 and 2 are the tracker's own."""
import numpy as np
import pytest

import _select_ref as R

pytestmark = pytest.mark.gpu


class Rig:
    """per shape: a tracker with the scene in slot 0 and the constant image in slot 1, and a selector for four jobs"""

    def __init__(self, ctx, shape):
        from direct_stereo_slam_amd import pixelselect, synth
        from direct_stereo_slam_amd.tracker import TrackerAndScaler

        w, h = shape
        self.trk = TrackerAndScaler(ctx, w, h, 3, synth.KITTI_T_STEREO, (100.0, 100.0, w / 2.0, h / 2.0))
        self.trk.upload_image(0, R.scene(w, h))
        self.trk.upload_image(1, np.full((h, w), 77.0, np.float32))
        self.sel = pixelselect.PixelSelector(ctx, w, h, 4, R.pattern(w, h))

    def job(self, case, **more):
        return R.job_of(case, tracker=self.trk, slot=1 if case.get("constant") else 0, **more)

    def close(self):
        self.sel.close(), self.trk.close()


@pytest.fixture(scope="module")
def rigs(ctx):
    r = {shape: Rig(ctx, shape) for shape in R.SHAPES}
    yield r
    for x in r.values():
        x.close()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_tracker_levels_are_the_checkers_pyramid(rigs, shape):
    """before anything is compared: a difference in levels 1 and 2 would not be the selector's"""
    for slot, image in ((0, R.scene(*shape)), (1, np.full(shape[::-1], 77.0, np.float32))):
        for lvl, plane in enumerate(R.pyramid(image)):
            got = rigs[shape].trk.get_frame(slot, lvl)[..., 0]
            assert got.shape == plane.shape and np.array_equal(got.view(np.uint32), plane.view(np.uint32)), (slot, lvl)


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_checker(rigs, name):
    from direct_stereo_slam_amd import pixelselect

    case = R.CASES[name]
    rig = rigs[case["shape"]]
    got = pixelselect.select_pixels_batch(rig.sel, [rig.job(case)], **case["params"])[0]
    R.assert_equal(got, R.expected(name))


def test_three_jobs_in_one_call_equal_single_calls_and_any_order(rigs):
    """different potentials and densities, one of them on the constant image, one with an inverse response, one without a map"""
    from direct_stereo_slam_amd import pixelselect

    w, h = R.SHAPES[1]
    rig = rigs[(w, h)]
    names = [f"{w}x{h}-adapt3-3000", "constant_image", f"{w}x{h}-adapt1-150", "b_inv"]
    jobs = [rig.job(R.CASES[n]) for n in names]
    together = pixelselect.select_pixels_batch(rig.sel, jobs)
    for n, g in zip(names, together):
        R.assert_equal(g, R.expected(n))
    order = [2, 0, 3, 1]
    permuted = pixelselect.select_pixels_batch(rig.sel, [jobs[k] for k in order])
    for k, g in zip(order, permuted):
        R.assert_equal(g, R.expected(names[k]))
    for j, n in zip(jobs, names):
        R.assert_equal(pixelselect.select_pixels_batch(rig.sel, [j])[0], R.expected(n))
    no_map = pixelselect.select_pixels_batch(rig.sel, [dict(jobs[0], want_map=False), jobs[2]])
    R.assert_equal(no_map[0], R.expected(names[0]), with_map=False), R.assert_equal(no_map[1], R.expected(names[2]))
    assert "map" not in no_map[0]


def test_potential_carries_from_call_to_call(rigs):
    """the potential a call leaves is what the sequence enters its next keyframe with (P12)"""
    from direct_stereo_slam_amd import pixelselect

    w, h = R.SHAPES[0]
    rig, pot = rigs[(w, h)], 3
    for _ in range(3):
        exp = R.select_ref(R.scene(w, h), R.pattern(w, h), pot, 300.0, R.MAX_PTS)
        got = pixelselect.select_pixels_batch(rig.sel, [dict(tracker=rig.trk, slot=0, density=300.0, potential=pot, max_pts=R.MAX_PTS)])[0]
        R.assert_equal(got, exp)
        pot = got["potential"]


def test_points_go_straight_into_a_trace_call(ctx, rigs):
    """the arrays have the layout dsm_trace_job consumes: fresh points against their own frame under the identity"""
    from direct_stereo_slam_amd import pixelselect, trace

    w, h = R.SHAPES[0]
    rig = rigs[(w, h)]
    got = pixelselect.select_pixels_batch(rig.sel, [dict(tracker=rig.trk, slot=0, density=300.0, potential=3, max_pts=R.MAX_PTS)])[0]
    n = len(got["u"])
    assert n == got["n_pts"] > 100
    job = dict(target=rig.trk, target_slot=0, krki=np.eye(3, dtype=np.float32).reshape(1, 9), kt=np.array([[5.0, 0.0, 0.0]], np.float32),
               aff=np.array([[1.0, 0.0]], np.float32), host=np.zeros(n, np.int32), trace_uv=np.zeros((n, 2), np.float32),
               trace_interval=np.zeros(n, np.float32), **{k: got[k] for k in R.KEYS if k != "type"})
    res = trace.trace_points_batch(ctx, [job])[0]
    assert res["counts"].sum() == n and res["counts"][trace.UNINITIALIZED] == 0
