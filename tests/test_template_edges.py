"""The device template builder (csrc/template_kernels.hip through dsm_tracker_set_ref_from_points / dsm_set_refs_from_points) against
the numpy checker tests/_template_ref.py at the edges of every stage: border pixels, full capacity, holes and non-finite values, long
per-pixel lists, emit blocks with nothing to emit, levels smaller than a wave, and a level with more than 1024 emit blocks (the
block-count scan's second pass).  Every comparison is bit for bit on all four lists of every level; tests/test_template_ref.py holds
the checker against the C oracle and the host form and asserts, on the CPU, that each case has the property it is named for."""
import numpy as np
import pytest

import _template_ref as R
from _scenes import regrad

pytestmark = pytest.mark.gpu

F = np.float32
POSE0 = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)  # (qx, qy, qz, qw, tx, ty, tz): the identity


def _tracker(ctx, geom):
    from direct_stereo_slam_amd import synth as S
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    w, h, nl = R.GEOMETRIES[geom]
    K = (0.9 * w, 0.9 * w, w / 2 - 0.5, h / 2 - 0.5)
    trk = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, K)
    trk.makeK(*K)
    return trk


@pytest.fixture(scope="module")
def trackers(ctx):
    """one tracker per geometry, shared by the cases of this module: each case also follows whatever the one before left behind"""
    cache = {}

    def get(geom):
        if geom not in cache:
            cache[geom] = _tracker(ctx, geom)
        return cache[geom]

    yield get
    for t in cache.values():
        t.close()


def _install(trk, c, frame=False):
    """the keyframe's pyramid into slot 0: the intensity planes alone, or whole (I, dx, dy) levels as makeImages forms them"""
    if frame:
        trk.upload_frame(0, [regrad(d) for d in R.dip(c.planes)], 1.0)
    else:
        trk.upload_intensity(0, c.planes, 1.0)


def _assert_template(trk, n, ref, what, idepth=None):
    assert n == ref.counts, (what, n, ref.counts)
    for l in range(len(ref.counts)):
        got = trk.get_template(l)
        for k, name in enumerate(("u", "v", "idepth", "color")):
            exp = idepth[l] if (k == 2 and idepth is not None) else ref.lists[k][l]
            assert len(got[k]) == len(exp), (what, l, name, len(got[k]), len(exp))
            np.testing.assert_array_equal(got[k], exp, err_msg=f"{what}: level {l}, {name}")


def _set(trk, c, frame_id=1):
    return trk.setCoarseTrackingRefFromPoints(frame_id, (0.01, 2.0), 1.25, c.pu, c.pv, c.pid, c.pw)


def _job(trk, c, frame_id, pu=None):
    return {"tracker": trk, "ref_frame_id": frame_id, "ref_aff": (0.0, 0.0), "ref_exposure": 1.0, "pu": c.pu if pu is None else pu, "pv": c.pv,
            "pidepth": c.pid, "pweight": c.pw}


@pytest.mark.parametrize("name", R.CASES)
def test_device_template_equals_reference(trackers, name):
    c = R.case(name)
    trk = trackers(c.geom)
    _install(trk, c, frame=name.startswith("border"))
    n = _set(trk, c, 7)
    assert trk.refFrameID == 7
    if name == "twopass-big":
        print("emit blocks of level 0:", R.emit_blocks(c.w, c.h), "entries:", n)
    _assert_template(trk, n, c.ref, name)


def test_batched_jobs_dense_next_to_empty(ctx):
    """one dsm_set_refs_from_points call: a full-capacity job on either side of an empty one -- a workspace overrun between jobs shows"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    names = ["dense-g68", "empty-g68", "single-g68", "collisions-g68", "dense-g68"]
    trks = [_tracker(ctx, "g68") for _ in names]
    jobs = []
    for j, (trk, name) in enumerate(zip(trks, names)):
        _install(trk, R.case(name))
        jobs.append(_job(trk, R.case(name), 20 + j))
    ns = TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, jobs)
    for j, (trk, name, n) in enumerate(zip(trks, names, ns)):
        assert trk.refFrameID == 20 + j
        _assert_template(trk, n, R.case(name).ref, f"job {j} ({name})")
    for t in trks:
        t.close()


def test_repeated_calls_leave_no_state(ctx):
    trk = _tracker(ctx, "g68")
    for k, name in enumerate(("dense-g68", "single-g68", "empty-g68", "border-g68")):
        c = R.case(name)
        _install(trk, c)
        _assert_template(trk, _set(trk, c, k), c.ref, f"call {k} ({name})")
    trk.close()


def test_scale_coarse_depth_after_device_template(trackers):
    """scaleCoarseDepthL0 (TrackerAndScaler.cpp:329-336): idepth /= scale in float32, everything else untouched"""
    c = R.case("border-odd")
    trk = trackers("odd")
    _install(trk, c)
    n = _set(trk, c)
    trk.scaleCoarseDepthL0(1.7)
    _assert_template(trk, n, c.ref, "scaled", idepth=[a / F(1.7) for a in c.ref.lists[2]])
    assert all(a.dtype == F for a in c.ref.lists[2])


# ---- the coordinate contract -----------------------------------------------------------------------------------------------------------

def _refused(size):
    return [np.nan, np.inf, -np.inf, 1e20, -1.6, size - 0.5]


def _accepted(size):
    return [-0.4, -1.4, np.nextafter(F(size - 0.5), F(0))]


@pytest.mark.parametrize("axis", ["u", "v"])
def test_device_coordinate_contract(trackers, axis):
    """accepted exactly when pu + 0.5f and pv + 0.5f are finite and truncate into [0, w) x [0, h); anything else fails the call with
    DSM_ERR_INVALID and leaves the tracker without a reference"""
    from direct_stereo_slam_amd._lib import DsmError

    c = R.case("border-tiny")
    trk = trackers("tiny")
    _install(trk, c)
    size = c.w if axis == "u" else c.h
    k = len(c.pu) // 2
    wrong = []
    for bad in _refused(size):
        pu, pv = c.pu.copy(), c.pv.copy()
        (pu if axis == "u" else pv)[k] = bad
        assert not R.accepted(pu, pv, c.w, c.h)[k]
        _set(trk, c)  # a valid reference, to be lost
        try:
            trk.setCoarseTrackingRefFromPoints(2, (0, 0), 1.0, pu, pv, c.pid, c.pw)
            wrong.append((bad, "accepted"))
            continue
        except DsmError as e:
            if "dsm error -1" not in str(e):  # DSM_ERR_INVALID
                wrong.append((bad, str(e)))
        with pytest.raises(DsmError, match="dsm error -4"):  # DSM_ERR_STATE: no reference
            trk.trackNewestCoarse(POSE0, [0, 0], c.nl - 1)
    assert not wrong, wrong
    for good in _accepted(size):
        pu, pv = c.pu.copy(), c.pv.copy()
        (pu if axis == "u" else pv)[k] = good
        ref = R.make_coarse_depth(c.w, c.h, c.nl, pu, pv, c.pid, c.pw, c.planes)
        n = trk.setCoarseTrackingRefFromPoints(3, (0, 0), 1.0, pu, pv, c.pid, c.pw)
        _assert_template(trk, n, ref, f"{axis} = {good!r}")


def test_bad_job_fails_the_whole_batch(ctx):
    """one refused point in the middle job of three: the call fails, no tracker of it keeps a reference, and a good call afterwards
    builds the reference's templates"""
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    names = ["border-g68", "collisions-g68", "blocks-g68"]
    trks = [_tracker(ctx, "g68") for _ in names]
    for trk, name in zip(trks, names):
        _install(trk, R.case(name))
    good = [_job(trk, R.case(name), 30 + j) for j, (trk, name) in enumerate(zip(trks, names))]
    TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, good)
    for trk in trks:
        trk.trackNewestCoarse(POSE0, [0, 0], 2)  # with a reference the call is taken (whatever it converges to)
    pu = R.case(names[1]).pu.copy()
    pu[len(pu) // 2] = np.nan
    bad = [good[0], _job(trks[1], R.case(names[1]), 41, pu=pu), good[2]]
    with pytest.raises(DsmError, match="dsm error -1"):
        TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, bad)
    for trk in trks:
        with pytest.raises(DsmError, match="dsm error -4"):
            trk.trackNewestCoarse(POSE0, [0, 0], 2)
    ns = TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, good)
    for j, (trk, name, n) in enumerate(zip(trks, names, ns)):
        _assert_template(trk, n, R.case(name).ref, f"after the failed call, job {j} ({name})")
    for t in trks:
        t.close()
