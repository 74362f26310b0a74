"""What dsm_select_pixels_host and dsm_select_pixels_batch refuse: every refusal is raised on the host form
without a GPU and on the batch form with one, before any output is written."""
import ctypes as C

import numpy as np
import pytest

import _select_ref as R

W, H = R.SHAPES[0]
NAN, INF = float("nan"), float("inf")
# (what, changes to the job dict, changes to the parameters)
SHARED = [
    ("a potential below 1", dict(potential=0), {}),
    ("a potential above the cap", dict(potential=4097), {}),
    ("a density of zero", dict(density=0.0), {}),
    ("a negative density", dict(density=-5.0), {}),
    ("a density that is not finite", dict(density=INF), {}),
    ("a density that is NaN", dict(density=NAN), {}),
    ("a negative max_pts", dict(max_pts=-1), {}),
    ("negative recursions", {}, dict(recursions=-1)),
    ("recursions above 4", {}, dict(recursions=5)),
    ("pattern_padding below 2", {}, dict(pattern_padding=1)),
    ("pattern_padding above 8", {}, dict(pattern_padding=9)),
] + [(f"a non-finite {k}", {}, {k: v}) for v in (NAN, INF) for k in
     ("min_grad_hist_cut", "min_grad_hist_add", "grad_downweight_per_level", "th_factor", "outlier_th", "outlier_th_sum_component",
      "overall_energy_th_weight")]
NULLS = ["potential_io", "n_pts_out", "num_total_out", "u", "v", "energy_th", "grad_h", "color", "weights", "status", "idepth_min", "idepth_max",
         "quality", "type"]
JOB = dict(density=300.0, potential=3, max_pts=600)


def untouched(b):
    st = b.state[0][0]
    return st["ints"][1:].tolist() == [-1] * 6 and (st["map"] == 255).all() and not st["u"].any() and not st["status"].any()


def run_host(b, **kw):
    from direct_stereo_slam_amd import pixelselect

    b.run_host(0, R.pyramid(R.scene(W, H)), R.pattern(W, H), pixelselect.params(**kw))


@pytest.mark.parametrize("what,job,kw", SHARED, ids=[s[0] for s in SHARED])
def test_host_form_refuses(built, what, job, kw):
    from direct_stereo_slam_amd import pixelselect
    from direct_stereo_slam_amd._lib import DsmError

    b = pixelselect.SelectBatch([dict(JOB, **job)], W, H)
    with pytest.raises(DsmError):
        run_host(b, **kw)
    assert untouched(b), what


@pytest.mark.parametrize("field", NULLS)
def test_host_form_refuses_null_arrays(built, field):
    from direct_stereo_slam_amd import pixelselect
    from direct_stereo_slam_amd._lib import DsmError

    b = pixelselect.SelectBatch([JOB], W, H)
    setattr(b.arr[0], field, None)
    with pytest.raises(DsmError):
        run_host(b)


def test_host_form_refuses_small_frames_and_null_planes(built):
    from direct_stereo_slam_amd import _lib, pixelselect
    from direct_stereo_slam_amd._lib import DsmError, c_float_p

    L = _lib.load()
    for w, h in ((31, 64), (64, 31)):
        b = pixelselect.SelectBatch([JOB], w, h)
        with pytest.raises(DsmError):
            b.run_host(0, [np.zeros((h >> l, w >> l), np.float32) for l in range(3)], np.zeros(w * h, np.uint8))
    b = pixelselect.SelectBatch([JOB], W, H)
    planes = [a.ctypes.data_as(c_float_p) for a in R.pyramid(R.scene(W, H))]
    rp = R.pattern(W, H).ctypes.data_as(C.POINTER(C.c_ubyte))
    p = pixelselect.params()
    for k in range(3):
        args = list(planes)
        args[k] = None
        assert L.dsm_select_pixels_host(W, H, *args, rp, C.byref(b.arr[0]), C.byref(p)) == -1
    assert L.dsm_select_pixels_host(W, H, *planes, None, C.byref(b.arr[0]), C.byref(p)) == -1
    assert L.dsm_select_pixels_host(W, H, *planes, rp, None, C.byref(p)) == -1
    assert L.dsm_select_pixels_host(W, H, *planes, rp, C.byref(b.arr[0]), None) == -1
    assert untouched(b)
    assert L.dsm_select_pixels_host(W, H, *planes, rp, C.byref(b.arr[0]), C.byref(p)) == 0  # and the job itself is fine
    with pytest.raises(TypeError):
        pixelselect.params(no_such_field=1)


@pytest.mark.gpu
def test_batch_form_refuses(ctx):
    from direct_stereo_slam_amd import pixelselect, synth
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler

    K = (100.0, 100.0, W / 2.0, H / 2.0)
    trk = TrackerAndScaler(ctx, W, H, 3, synth.KITTI_T_STEREO, K)
    trk.upload_image(0, R.scene(W, H))
    sel = pixelselect.PixelSelector(ctx, W, H, 2, R.pattern(W, H))
    good = dict(JOB, tracker=trk, slot=0)
    two_levels = TrackerAndScaler(ctx, W, H, 2, synth.KITTI_T_STEREO, K)
    two_levels.upload_image(0, R.scene(W, H))
    big = TrackerAndScaler(ctx, W + 32, H, 3, synth.KITTI_T_STEREO, K)
    big.upload_image(0, np.zeros((H, W + 32), np.float32))
    other = Context(0)
    foreign = TrackerAndScaler(other, W, H, 3, synth.KITTI_T_STEREO, K)
    foreign.upload_image(0, R.scene(W, H))
    calls = [(what, [good, dict(good, **job)], kw) for what, job, kw in SHARED]
    calls += [("an empty slot", [good, dict(good, slot=1)], {}), ("slot 2", [good, dict(good, slot=2)], {}), ("no tracker", [good, dict(JOB)], {}),
              ("fewer than 3 levels", [good, dict(good, tracker=two_levels)], {}), ("mixed geometry", [good, dict(good, tracker=big)], {}),
              ("a tracker of another context", [good, dict(good, tracker=foreign)], {}), ("more jobs than max_jobs", [good, good, good], {})]
    for what, jobs, kw in calls:
        b = pixelselect.SelectBatch(jobs, W, H)
        with pytest.raises(DsmError):
            b.run(sel, pixelselect.params(**kw))
        assert untouched(b), what  # all or nothing: the good job before the bad one was not run either
    for field in NULLS:
        b = pixelselect.SelectBatch([good, good], W, H)
        setattr(b.arr[1], field, None)
        with pytest.raises(DsmError):
            b.run(sel)
        assert untouched(b), field
    b = pixelselect.SelectBatch([good], W, H)
    assert ctx.L.dsm_select_pixels_batch(sel.h, 0, b.arr, C.byref(pixelselect.params())) == -1
    assert ctx.L.dsm_select_pixels_batch(sel.h, 1, None, C.byref(pixelselect.params())) == -1
    assert ctx.L.dsm_select_pixels_batch(sel.h, 1, b.arr, None) == -1
    assert ctx.L.dsm_select_pixels_batch(None, 1, b.arr, C.byref(pixelselect.params())) == -1
    for w, h, n, rp in ((31, 64, 1, np.zeros(31 * 64, np.uint8)), (W, H, 0, R.pattern(W, H)), (W, H, 4097, R.pattern(W, H))):
        hnd = C.c_void_p()
        assert ctx.L.dsm_pixel_selector_create(ctx.h, w, h, n, rp.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(hnd)) == -1 and not hnd.value
    # the selector and the context are still usable
    R.assert_equal(pixelselect.select_pixels_batch(sel, [dict(good, max_pts=R.MAX_PTS)])[0], R.expected(f"{W}x{H}-adapt3-300"))
    sel.close(), foreign.close(), other.close(), big.close(), two_levels.close(), trk.close()
