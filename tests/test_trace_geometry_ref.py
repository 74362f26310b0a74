"""CPU: dsm_trace_points_host against the checker tests/_trace_ref.py at a second geometry, 101 x 53, and at 24 x 20, just above the
8 x 8 minimum -- bit for bit -- and what the scene built for any geometry (_trace_ref.make_scene_at)
must reach there, asserted on the checker's output alone; the figures in the comments are what it reaches."""
import numpy as np
import pytest

import _trace_ref as R


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_host_form_equals_checker(built, geom):
    from direct_stereo_slam_amd import trace

    job, target, exp, _ = R.geometry_case(*geom)
    R.assert_equal(trace.trace_points_host(*geom, target, job), exp)


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_every_side_has_points_that_t2_keeps_and_points_that_it_sends_out(geom):
    """next to each side at least three points on either side of T2's bound, all within 1.5 px of it: the decisive projection (at
    idepth_min) in float64"""
    w, h = geom
    job, _, exp, sides = R.geometry_case(w, h)
    for side in R.SIDES:
        axis, bound, sign = R.side_bound(side, w, h)
        kept = out = 0
        for i, delta in zip(sides[side], R.SIDE_DELTAS):
            hst = int(job["host"][i])
            p = R.project(job["krki"][hst], job["kt"][hst], float(job["u"][i]), float(job["v"][i]), float(job["idepth_min"][i]))
            inside_by = sign * (p[axis] - bound)
            assert abs(inside_by) < 1.5 and abs(inside_by - delta) < 1e-4, (side, i, inside_by)
            assert 4 < p[1 - axis] < (h, w)[axis] - 5  # the other coordinate does not decide
            assert min(job["u"][i], w - 1 - job["u"][i], job["v"][i], h - 1 - job["v"][i]) <= 9  # the point itself is next to the side
            left_at_t2 = "T2_oob" in exp["point_branches"][i]
            assert left_at_t2 == (not inside_by > 0), (side, i, inside_by)
            if left_at_t2:
                assert exp["status"][i] == R.OOB and exp["steps"][i] == 0 and exp["trace_uv"][i].tolist() == [-1, -1]
            kept, out = kept + (not left_at_t2), out + left_at_t2
        assert kept >= 3 and out >= 3, (side, kept, out)  # 3 and 4 (one of them exactly on the bound) at every side
    assert sum(len(v) for v in sides.values()) == 28


def test_every_status_occurs_at_101_x_53():
    job, _, exp, _ = R.geometry_case(101, 53)
    counts = exp["counts"]
    assert (counts[:5] >= 3).all() and counts[R.UNINITIALIZED] == 0, counts  # 81 good, 57 out of bounds, 6 outliers, 25 skipped, 15 ill-conditioned
    assert (job["status"] == R.UNINITIALIZED).sum() >= 3 and (job["status"] == R.OOB).sum() >= 3 and (job["status"] == R.OUTLIER).sum() >= 3
    for k in range(len(job["kt"])):  # fresh and narrowed points on every host
        on = job["host"] == k
        assert (on & (job["status"] == R.UNINITIALIZED)).sum() >= 5 and (on & np.isfinite(job["idepth_max"])).sum() >= 5, k
    for b in ("T1", "T2_oob", "T3_oob", "T3_skipped", "T4_taken", "T4_oob", "T6_badcondition", "T12_outlier", "T12_outlier_to_oob", "T13_swap", "T15"):
        assert exp["branches"][b] >= 3, (b, exp["branches"][b])  # 6, 32, 10, 25, 61, 5, 15, 6, 4, 8, 81
    assert len(job["host"]) % 64 and len(job["host"]) % 8 == 0 and len(job["host"]) > 128  # 184 points: a partial last wave


def test_most_points_leave_at_24_x_20():
    job, _, exp, _ = R.geometry_case(24, 20)
    n = len(job["host"])
    assert exp["counts"][R.OOB] > n // 2 and exp["branches"]["T2_oob"] >= 50, exp["counts"]  # 100 of 184 out of bounds, 76 of them at T2
    assert exp["counts"][R.GOOD] >= 20 and exp["steps"].max() >= 2  # 63: the search still runs
    assert abs(float(np.float32(24 + 20) * np.float32(0.027)) - 1.188) < 1e-3  # maxPix: little more than a pixel
