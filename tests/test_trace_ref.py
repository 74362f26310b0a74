"""CPU: the host form dsm_trace_points_host against the checker tests/_trace_ref.py, bit for bit: the
160 x 64 scene with the default settings and with max_pix_search = 0.5, other settings; the branches the scene must reach, asserted
on the checker's output alone; the invalid calls; and two properties of the checker itself."""
import numpy as np
import pytest

import _trace_ref as R


def test_scene_reaches_every_branch():
    """on the checker's output alone, over the two cases "defaults" (maxPix = 6.05 px) and "wide" (max_pix_search = 0.5, the search
    reaches its cap): a form that skips a branch cannot equal the checker on both"""
    d, wd = R.case("defaults")[2], R.case("wide")[2]
    assert abs(float(np.float32(R.W + R.H) * np.float32(0.027)) - 6.05) < 0.01
    total = {k: d["branches"][k] + wd["branches"][k] for k in R.REQUIRED}
    print(total)
    assert all(v >= 5 for v in total.values()), {k: v for k, v in total.items() if v < 5}
    assert wd["steps"].max() == 99 and wd["branches"]["T7_cap"] >= 5 and d["steps"].max() <= 10
    assert set(np.unique(d["status"])) == {R.GOOD, R.OOB, R.OUTLIER, R.SKIPPED, R.BADCONDITION}
    assert (d["counts"] == np.bincount(d["status"], minlength=6)).all() and d["counts"].sum() == len(d["status"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_form_equals_checker(built, name):
    from direct_stereo_slam_amd import trace

    job, target, exp, params = R.case(name)
    R.assert_equal(trace.trace_points_host(R.W, R.H, target, job, **params), exp)


def test_other_settings_change_the_outcome():
    """huber_th, gn_iterations, min_test_radius and stepsize are read, not assumed (the checker's outputs differ between the cases)"""
    base = R.trace(R.W, R.H, R.case("no_gn")[1], R.case("no_gn")[0])
    for name in ("huber_4", "no_gn", "gn_6", "radius_1", "half_steps"):
        exp = R.case(name)[2]
        assert any(not R.same_bits(exp[k], base[k]) for k in ("idepth_min", "quality", "trace_uv")), name
    assert R.case("half_steps")[2]["steps"].max() > base["steps"].max()


def test_three_frames_in_sequence_host(built):
    """the outputs of one call are the inputs of the next; every frame is the scene's texture moved sideways by one more pixel"""
    from direct_stereo_slam_amd import trace

    got = R.case("defaults")[0]
    for frame, _, exp in R.sequence():
        res = trace.trace_points_host(R.W, R.H, frame, got)
        R.assert_equal(res, exp)
        got = R.advance(got, res)
    assert exp["branches"]["T1"] > 8 and exp["branches"]["T3_skipped"] > 16  # the state has moved on


def test_host_form_refuses_invalid_calls_and_writes_nothing(built):
    from direct_stereo_slam_amd import _lib, trace
    from direct_stereo_slam_amd._lib import DsmError

    job, target, _, _ = R.case("no_gn")

    def refused(b, p=None):
        before = [{k: v.copy() for k, v in st.items()} for st, _ in b.state]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, target, p)
        for (st, _), bef in zip(b.state, before):
            assert all(np.array_equal(st[k], bef[k], equal_nan=k != "status") for k in st)

    for what, bad, kw in R.invalid_calls(job):
        refused(trace.TraceBatch([bad]), trace.params(**kw))
    # NULL arrays and negative counts, on the C structure itself
    for field in ("krki", "kt", "aff", "host", "u", "v", "energy_th", "grad_h", "color", "weights", "status", "idepth_min", "idepth_max",
                  "quality", "trace_uv", "trace_interval"):
        b = trace.TraceBatch([job])
        setattr(b.arr[0], field, None)
        refused(b)
    for field in ("n_pts", "n_hosts"):
        b = trace.TraceBatch([job])
        setattr(b.arr[0], field, -1)
        refused(b)
    b = trace.TraceBatch([job])
    assert _lib.load().dsm_trace_points_host(R.W, R.H, None, b.arr, trace.params()) == -1  # no target plane
    assert _lib.load().dsm_trace_points_host(R.W, R.H, target.ctypes.data_as(_lib.c_float_p), b.arr, None) == -1  # no settings
    # no hosts and no points is a valid job
    empty = {k: np.asarray(v)[:0] for k, v in job.items()}
    res = trace.trace_points_host(R.W, R.H, target, empty)
    assert len(res["status"]) == 0 and (res["counts"] == 0).all()


def test_good_points_bracket_the_true_inverse_depth():
    """A clean pair with known depth: the plane at idepth 0.25 seen by every host, no stripes, no NaN, no noise, fresh points.  The
    pattern's shift at the truth is at most 4.2 px, inside the 6.05 px searched, and the texture's shortest wavelength is 9 px, above
    that range, so the energy has one minimum on the line; the interval is the refined position +- err with err >= 0.4 px, four
    times the 0.1 px at which the refinement stops.  So every GOOD point must bracket 0.25.  Hosts 0 - 3 (translation across the
    optical axis): host 4's interval may straddle its epipole and host 6 is no camera."""
    job, target, truth = R.scene(seed=3, plain=True, noise=0.0)
    res = R.trace(R.W, R.H, target, job)
    good = (res["status"] == R.GOOD) & (job["host"] < 4)
    assert good.sum() >= 40
    assert (res["idepth_min"][good] <= truth).all() and (res["idepth_max"][good] >= truth).all()
    assert np.isfinite(res["idepth_max"][good]).all() and (res["trace_interval"][good] <= 20.0).all()  # narrowed from [0, inf): 2 err, err <= 10


def test_second_trace_against_the_same_frame_skips_most_good_points():
    job, target, first, _ = R.case("defaults")
    second = R.trace(R.W, R.H, target, R.advance(job, first))
    was_good = first["status"] == R.GOOD
    settled = np.isin(second["status"][was_good], (R.SKIPPED, R.BADCONDITION))
    print(int(was_good.sum()), int(settled.sum()))
    assert was_good.sum() >= 100 and settled.mean() > 0.5
