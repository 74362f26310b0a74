"""CPU: dsm_optimize_immature_points_host against the checker tests/_immature_ref.py at a second geometry, 101 x 53, nine frames that
shift the pattern towards every side -- bit for bit -- and what that window must reach, asserted on the
checker's output alone; the figures in the comments are what it reaches."""
import numpy as np

import _immature_ref as R


def test_host_form_equals_checker(built):
    from direct_stereo_slam_amd import immature

    job, frames, exp = R.geometry_case()
    R.assert_equal(immature.optimize_immature_points_host(*R.GEOMETRY, job, frames), exp)


def test_residuals_leave_over_every_side_and_some_points_keep_all_eight():
    w, h = R.GEOMETRY
    job, frames, exp = R.geometry_case()
    n, nf = len(job["host"]), len(frames)
    assert nf == 9 and w % 2 == 1 and h % 2 == 1 and n % 8 == 0 and n % 64  # 88 points: the last wave is partial
    assert ((exp["res_state"] == R.IN).sum(axis=1) == 8).sum() >= 3  # 13 points whose eight residuals all count
    over = dict.fromkeys(R.SIDES, 0)
    for i in range(n):
        for f in range(nf):
            if exp["res_state"][i, f] == R.OOB:
                sides = R.sides_left_at(w, h, job, i, f)
                if len(sides) == 1:  # out of bounds from the first pass on, over this side alone
                    over[sides.pop()] += 1
    assert all(v >= 10 for v in over.values()), over  # 34 left, 57 right, 75 top, 74 bottom
    tr = exp["trace"]
    for k in ("accepted", "rejected", "oob_after_partial_sum", "oob_first_pixel", "oob_non_finite_sample", "entered_oob", "clamped"):
        assert tr[k] >= 3, (k, tr[k])  # 220, 35, 66, 208, 3, 731, 211
    assert sorted(np.unique(exp["status"])) == [0, 1, 2]  # 3, 79, 6
    for s in range(4):  # ten points within 8 px of each side
        d = [job["u"], w - 1 - job["u"], job["v"], h - 1 - job["v"]][s]
        assert (d[-40 + 10 * s:][:10] <= 8).all()
