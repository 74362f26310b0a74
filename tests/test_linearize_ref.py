"""CPU: the host form dsm_linearize_residuals_host against the checker tests/_linearize_ref.py, bit for bit (DESIGN.md section 16,
L1-L8, B1-B4): the 96 x 64 scenes of 5 and 9 frames, windows of 1, 2 and 3 frames, no points; the branches the scenes must reach,
asserted on the checker's output alone; the geometric Jacobians against central differences of a float64 projection; the order
statistic of B2 at its edges; the invalid calls."""
import numpy as np
import pytest

import _linearize_ref as R

OTHER = dict(huber_th=4.0, outlier_th_sum_component=900.0, scale_idepth=2.0, scale_f=30.0, scale_c=20.0, thn=0.45, fac_median=1.2,
             cw=0.3, ow=0.8)


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_scene_reaches_every_branch(name):
    """on the checker's output alone: a form that skips a branch cannot equal it"""
    job, frames, exp, _ = R.case(name)
    tags = exp["tags"]
    exits = [t["exit"] for t in tags]
    l4 = [t for t in tags if t["exit"] == "l4"]
    l7 = [t for t in tags if "th_from" in t]
    keep, is_new = exp["keep"].astype(bool), np.asarray(job["is_new"]).astype(bool)
    counts = dict(l1_entry=exits.count("l1_entry"), l2_drescale=exits.count("l2_drescale"), l2_bounds=exits.count("l2_bounds"),
                  l4_first_failure_at_0=sum(1 for t in l4 if t["first_fail"] == 0), l4_first_failure_later=sum(1 for t in l4 if t["first_fail"] >= 1),
                  l4_non_finite=sum(1 for t in l4 if t["non_finite"]), hw_below_1=sum(t["hw_lt1"] for t in tags), hw_1=sum(t["hw_eq1"] for t in tags),
                  outlier_by_energy=exits.count("outlier_energy"), outlier_by_wji2=exits.count("outlier_wji2"), ended_in=exits.count("in"),
                  kept_new=int((keep & is_new).sum()), kept_old=int((keep & ~is_new).sum()), th_from_host=sum(1 for t in l7 if t["th_from"] == "host"),
                  th_from_target=sum(1 for t in l7 if t["th_from"] == "target"), entered_outlier=int((np.asarray(job["state_in"]) == R.OUTLIER).sum()),
                  hosts_used=3 * len(set(np.asarray(job["host"]).tolist())) // len(frames))
    print(counts)
    assert all(v >= 3 for v in counts.values()), counts
    assert int(exp["defined"].sum()) == counts["ended_in"] + counts["outlier_by_energy"] + counts["outlier_by_wji2"]
    assert (exp["new_energy_with_outlier"][~exp["defined"]] == -1).all() and (exp["new_energy_with_outlier"][exp["defined"]] >= 0).all()
    assert np.array_equal(exp["new_energy"][~exp["defined"]], np.asarray(job["energy_in"])[~exp["defined"]])  # L1
    # the residual list does not cover every (point, frame) pair
    assert len(tags) < len(job["host"]) * (len(frames) - 1)
    # L2 and L4 read different inputs on part of the pairs and points
    assert (np.asarray(job["idepth_zero_scaled"]) != np.asarray(job["idepth_scaled"])).sum() >= 3
    A = R.arrays_of(job)
    assert sum(1 for a in range(len(frames)) for b in range(len(frames)) if a != b and not np.array_equal(A["pre_RTll_0"][a, b], np.eye(3, dtype=np.float32).reshape(9))) >= 3


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_form_equals_checker(built, name):
    from direct_stereo_slam_amd import linearize

    job, frames, exp, _ = R.case(name)
    got = linearize.linearize_residuals_host(R.W, R.H, job, frames)
    R.assert_equal(got, exp)
    if len(job["point"]) == 0:  # B4
        assert got["energy"] == 0.0 and got["new_frame_energy_th"] == np.float32(1152.0)
    if not job["fix_linearization"]:
        assert (got["keep"] == 77).all() and (got["rel_bs"] == -7).all()  # not written: the mirror's fill values


def test_rows_of_oob_residuals_are_not_written(built):
    from direct_stereo_slam_amd import linearize

    job, frames, exp, _ = R.case("scene")
    got = linearize.linearize_residuals_host(R.W, R.H, job, frames)
    assert (~exp["defined"]).sum() >= 3
    for k in R.FIELDS_DEFINED:
        assert (got[k][~exp["defined"]] == -7).all(), k


def test_host_form_with_other_parameters_flags_and_outputs(built):
    """every parameter is read, not assumed; zero_jab_a / _b blank JabF after the sums; fix_linearization off; optional outputs NULL"""
    from direct_stereo_slam_amd import linearize

    job, frames, exp_default, _ = R.case("scene")
    job = R.prefix(job, 120)
    exp = R.linearize(R.W, R.H, job, frames, OTHER)
    assert not np.array_equal(exp["new_state"], exp_default["new_state"][:120]) and exp["new_frame_energy_th"] != exp_default["new_frame_energy_th"]
    R.assert_equal(linearize.linearize_residuals_host(R.W, R.H, job, frames, linearize.default_params(**OTHER)), exp)
    base = R.linearize(R.W, R.H, job, frames)
    for za, zb in ((1, 0), (0, 1), (1, 1)):
        kw = dict(zero_jab_a=za, zero_jab_b=zb)
        e = R.linearize(R.W, R.H, job, frames, kw)
        d = e["defined"]
        assert (e["J"][d, 46:54] == 0).all() == bool(za) and (e["J"][d, 54:62] == 0).all() == bool(zb)
        assert np.array_equal(e["J"][:, 62:], base["J"][:, 62:])  # the sums took the unzeroed values
        R.assert_equal(linearize.linearize_residuals_host(R.W, R.H, job, frames, linearize.default_params(**kw)), e)
    off = dict(job, fix_linearization=0)
    got = linearize.linearize_residuals_host(R.W, R.H, off, frames)
    R.assert_equal(got, R.linearize(R.W, R.H, off, frames))
    assert (got["keep"] == 77).all()
    got = linearize.linearize_residuals_host(R.W, R.H, job, frames, outputs=())
    R.assert_equal(got, base, outputs=())
    assert (got["J"] == -7).all() and (got["keep"] == 77).all()


def test_frame_energy_threshold_at_its_edges(built):
    """B2: count = 10 under the default thn (the float32 product 0.7f * 10 truncates to 7, the double product to 6), count = 1, and no
    residual against the newest frame"""
    from direct_stereo_slam_amd import linearize

    job, frames, exp, _ = R.case("scene")
    last = len(frames) - 1
    counted = [r for r in range(len(job["point"])) if job["target"][r] == last and exp["new_energy_with_outlier"][r] >= 0]
    others = [r for r in range(len(job["point"])) if job["target"][r] != last][:40]
    assert len(counted) >= 10
    assert int(np.float32(0.7) * np.float32(10)) == 7 and int(0.7 * 10) == 7 and int(float(np.float32(0.7)) * 10) == 6
    for n in (10, 1, 0):
        sub, e = R.case_subset("scene", sorted(others + counted[:n]))
        if n == 10:
            vals = sorted(float(e["new_energy_with_outlier"][i]) for i in range(len(sub["point"])) if sub["target"][i] == last)
            assert len(vals) == 10 and vals[6] != vals[7]
            th7 = np.float32(np.float32(13.0) + np.float32(np.float32(np.sqrt(np.float32(vals[7]))) * np.float32(1.5)) * np.float32(0.5))
            assert e["new_frame_energy_th"] == np.float32(th7 * th7)
        if n == 0:
            assert e["new_frame_energy_th"] == np.float32(1152.0)
        R.assert_equal(linearize.linearize_residuals_host(R.W, R.H, sub, frames), e)


# ---- L3 against central differences of a float64 restatement of the centre projection --------------------------------------------------

def _se3_exp(xi):
    """exp of the twist (translation first) as a 4 x 4 matrix, by its series"""
    v, w = xi[:3], xi[3:]
    A = np.zeros((4, 4))
    A[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    A[:3, 3] = v
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 12):
        term = term @ A / k
        out = out + term
    return out


def _project64(K4, T, u, v, idepth):
    fx, fy, cx, cy = K4
    p = T[:3, :3] @ np.array([(u - cx) / fx, (v - cy) / fy, 1.0]) + T[:3, 3] * idepth
    return np.array([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy])


def _central(f, x0):
    h = 1e-6 * max(abs(x0), 1.0)
    return (f(x0 + h) - f(x0 - h)) / (2 * h)


def test_geometric_jacobians_equal_central_differences():
    """Jpdd, Jpdxi and Jpdc of the checker against derivatives of the projection with respect to idepth, a left-multiplied exp(xi) on the
    host-to-target transform and (fx, fy, cx, cy) in units of SCALE_F / SCALE_C, where the linearisation point is the current state.
    Bar: 1e-4 of the row's largest magnitude (float32 rounding over the ~20 operations of a row is ~1e-6; a wrong term is O(1))."""
    job, frames, exp, _ = R.case("nine_frames")
    A = R.arrays_of(job)
    P = dict(R.PARAMS)
    checked = 0
    for r in range(len(A["point"])):
        p, tgt = int(A["point"][r]), int(A["target"][r])
        hst = int(A["host"][p])
        if (hst + tgt) % 2 == 1 or A["idepth_zero_scaled"][p] != A["idepth_scaled"][p]:
            continue  # the linearisation point differs from the current state
        R0, T0 = A["pre_RTll_0"][hst, tgt], A["pre_tTll_0"][hst, tgt]
        c, _ = R.centre(A["cam6"], R0, T0, A["u"][p], A["v"][p], A["idepth_zero_scaled"][p], R.W, R.H)
        if c is None:
            continue
        Jpdxi, Jpdc, Jpdd = (np.array(x, np.float64) for x in R.geometric(A["cam6"], R0, T0, c, P))
        K4 = [float(x) for x in A["cam6"][:4]]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R0.astype(np.float64).reshape(3, 3), T0.astype(np.float64)
        u, v, idp = float(A["u"][p]), float(A["v"][p]), float(A["idepth_zero_scaled"][p])
        fd_dd = _central(lambda x: _project64(K4, T, u, v, x), idp) * P["scale_idepth"]
        fd_xi = np.stack([_central(lambda x, k=k: _project64(K4, _se3_exp(np.eye(6)[k] * x) @ T, u, v, idp), 0.0) for k in range(6)], axis=1)
        scale = [P["scale_f"], P["scale_f"], P["scale_c"], P["scale_c"]]
        fd_dc = np.stack([_central(lambda x, k=k: _project64([K4[i] + (x * scale[k] if i == k else 0.0) for i in range(4)], T, u, v, idp), 0.0)
                          for k in range(4)], axis=1)
        for got, fd in ((Jpdd, fd_dd), (Jpdxi[0], fd_xi[0]), (Jpdxi[1], fd_xi[1]), (Jpdc[0], fd_dc[0]), (Jpdc[1], fd_dc[1])):
            assert np.abs(got - fd).max() <= 1e-4 * np.abs(fd).max(), (r, got, fd)
        assert np.array_equal(exp["J"][r, 8:30], np.concatenate([Jpdxi[0], Jpdxi[1], Jpdc[0], Jpdc[1], Jpdd]).astype(np.float32)) or not exp["defined"][r]
        checked += 1
    assert checked >= 20


def test_host_form_refuses_invalid_calls_and_writes_nothing(built):
    from direct_stereo_slam_amd import _lib, linearize
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, _, _ = R.case("two_frames")

    def refused(b, params=None):
        before = [{k: v.copy() for k, v in out.items()} for out, _ in b.outs]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, params)
        for (out, _), bef in zip(b.outs, before):
            assert all(np.array_equal(out[k], bef[k]) for k in out)

    for what, bad, kw in R.invalid_jobs(job):
        refused(linearize.LinearizeBatch([bad]), linearize.default_params(**kw))
    # n_frames outside [1, 16], negative counts and NULL arrays, on the C structure itself
    b = linearize.LinearizeBatch([job])
    for field, values in (("n_frames", (0, 17)), ("n_pts", (-1,)), ("n_res", (-1,))):
        old = getattr(b.arr[0], field)
        for x in values:
            setattr(b.arr[0], field, x)
            refused(b)
        setattr(b.arr[0], field, old)
    for field in ("frame_ids", "pre_RTll_0", "pre_tTll_0", "pre_KRKiTll", "pre_KtTll", "pre_aff_mode", "pre_b0_mode", "frame_energy_th", "host", "u",
                  "idepth_zero_scaled", "weights", "point", "target", "state_in", "energy_in", "is_new", "new_state", "new_energy",
                  "new_energy_with_outlier", "energy_out", "new_frame_energy_th_out"):
        b = linearize.LinearizeBatch([job])
        setattr(b.arr[0], field, None)
        refused(b)
    b = linearize.LinearizeBatch([job])
    with pytest.raises(DsmError):
        check = _lib.check
        check(_lib.load().dsm_linearize_residuals_host(R.W, R.H, b.arr, None, None))
    b.run_host(R.W, R.H, 0, frames)  # and the job itself is fine
    R.assert_equal(b.results()[0], R.case("two_frames")[2])


def test_host_form_at_another_geometry(built):
    """101 x 53, nine frames moving towards every side: residuals leave their targets over each of the four bounds"""
    from direct_stereo_slam_amd import linearize

    job, frames, exp = R.geometry_case()
    w, h = R.GEOMETRY
    gone = [R.sides_left(w, h, job, r) for r in range(len(job["point"])) if exp["tags"][r]["exit"] in ("l2_bounds", "l4")]
    for side in R.SIDES:
        assert sum(1 for g in gone if side in g) >= 3, side
    assert (exp["new_state"] == R.IN).sum() >= 20
    R.assert_equal(linearize.linearize_residuals_host(w, h, job, frames), exp)
