"""CPU: the checker of the end of optimize behind its loop (tests/_finish_ref.py) covers the ground the device
tests rely on, asserted on its output alone; the host form dsm_window_finish_host equals it bit for bit on every output (both use the
same C library); and two properties that do not depend on the stated order of operations."""
import numpy as np
import pytest

import _finish_ref as F
import _linearize_ref as R
import _optimize_ref as O
import _step_ref as T
from direct_stereo_slam_amd import finish as S
from direct_stereo_slam_amd import optimize as OS
from direct_stereo_slam_amd._lib import DsmError

f32, f64 = np.float32, np.float64
FRAME_SCENES = ("one_frame", "two_frames", "three_frames", "scene", "nine_frames", "sixteen_frames")  # 1, 2, 3, 5, 9 and 16 frames
GROUND = ("scene", "nine_frames", "two_frames", "three_frames")


def host(job, frames, max_iterations, w=R.W, h=R.H, **op):
    return S.window_finish_host(w, h, dict(job, max_iterations=max_iterations), frames, optimize_params=OS.default_optimize_params(**op))


def assert_host_equals(job, frames, max_iterations, what, **op):
    loop, exp = F.run(job, frames, max_iterations, op)
    o, got = host(job, frames, max_iterations, **op)
    assert o["pattern"] == loop["pattern"] and o["n_passes"] == loop["n_passes"], what
    F.assert_equal(got, exp, what=what)
    F.assert_rows_equal(got, exp, what)
    return loop, exp


# ---- the ground, on the checker's output alone --------------------------------------------------------------------------------------

def test_checker_covers_every_branch_of_the_bookkeeping():
    seen = set()
    for name in GROUND:
        job, _, _, exp = F.expected(name)
        point, is_new = np.asarray(job["point"]), np.asarray(job["is_new"])
        keep, rel = exp["keep"], exp["rel_bs"]
        last_in, last_out = np.asarray(job["last_res"]), exp["last_res_out"]
        mrb_in, mrb_out = np.asarray(job["max_rel_baseline_in"], f32), exp["max_rel_baseline_out"]
        seen |= {"removed"} if (keep == 0).any() else set()
        seen |= {"kept"} if (keep == 1).any() else set()
        for r in np.flatnonzero((keep == 1) & (is_new != 0)):
            seen.add("raises" if rel[r] > mrb_in[point[r]] else "does not raise")
        assert (mrb_out >= mrb_in).all()
        for p in range(len(job["host"])):
            l0, l1 = last_in[p]
            if l0 >= 0:
                seen.add("slot 0 updated")
                assert exp["last_state_out"][p, 0] == exp["new_state"][l0]
                if not keep[l0]:
                    seen.add("slot 0 cleared")
                    assert last_out[p, 0] == -1
            if l1 >= 0 and l1 != l0:
                seen.add("slot 1 updated")
                assert exp["last_state_out"][p, 1] == exp["new_state"][l1]
                if not keep[l1]:
                    seen.add("slot 1 cleared")
                    assert last_out[p, 1] == -1
            if l1 >= 0 and l1 == l0:
                seen.add("slot 1 names slot 0's residual")
                assert exp["last_state_out"][p, 1] == np.asarray(job["last_state_in"])[p, 1] and last_out[p, 1] == l1
            mine = np.flatnonzero(point == p)
            if any(not keep[r] and r != l0 and r != l1 for r in mine):
                seen.add("removed residual in neither slot")
            if len(mine) and exp["point_dropped"][p]:
                seen.add("point dropped")
                assert exp["n_res_kept"][p] == 0 and exp["point_index_out"][p] == -1
        assert exp["n_res_out"] == int(keep.sum()) and exp["n_pts_out"] == int((exp["point_dropped"] == 0).sum())
        assert list(exp["res_index_out"][keep == 1]) == list(range(exp["n_res_out"])) and (exp["res_index_out"][keep == 0] == -1).all()
        assert exp["lost"] == 0 and np.isfinite(exp["rmse"])
    want = {"removed", "kept", "raises", "does not raise", "slot 0 updated", "slot 1 updated", "slot 0 cleared", "slot 1 cleared",
            "slot 1 names slot 0's residual", "removed residual in neither slot", "point dropped"}
    assert seen == want, want - seen


def test_checker_z2_replaces_the_pairs_of_the_newest_frame_alone():
    for name in ("scene", "two_frames", "one_frame"):
        job, _, _, exp = F.expected(name)
        n = len(job["frame_ids"])
        f = n - 1
        AH0, AT0 = np.asarray(job["ad_host"], f64).reshape(n, n, 8, 8), np.asarray(job["ad_target"], f64).reshape(n, n, 8, 8)
        for h in range(n):
            for t in range(n):
                same = exp["ad_host_out"][h, t].tobytes() == AH0[h, t].tobytes() and exp["ad_target_out"][h, t].tobytes() == AT0[h, t].tobytes()
                assert same == (h != f and t != f), (name, h, t)  # h == f, t == f and the diagonal (f, f) are Z2's
        a = exp["ad_host_out"][f, f, 6, 6] / 10.0
        assert exp["ad_target_out"][f, f, 7, 7] == -1000.0 and exp["ad_target_out"][f, f, 6, 6] == -10.0 * a and exp["ad_host_out"][f, f, 7, 7] == 1000.0 * a


# ---- the host form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FRAME_SCENES)
def test_host_form_equals_the_checker_bit_for_bit(built, name):
    """1, 2, 3, 5, 9 and 16 frames, six iterations; every scene with residuals rejects a step"""
    job, frames = F.scene(name)
    _, _, loop, exp = F.expected(name)
    if len(job["point"]):
        assert "R" in loop["pattern"]
    o, got = host(job, frames, 6)
    assert o["pattern"] == loop["pattern"]
    F.assert_equal(got, exp, what=name)
    F.assert_rows_equal(got, exp, name)


@pytest.mark.parametrize("name", ["one_frame", "two_frames", "three_frames", "scene"])
def test_host_form_max_iterations_0_and_force_accept(built, name):
    job, frames = F.scene(name)
    assert_host_equals(job, frames, 0, (name, 0))
    loop, _ = assert_host_equals(job, frames, 6, (name, "force"), force_accept=1)
    assert loop["pattern"] == "A" * loop["n_iterations"]


def test_host_form_embedded_outputs_are_the_optimize_calls(built):
    job, frames = F.scene("three_frames")
    o, _ = host(job, frames, 6)
    ref = OS.window_optimize_host(R.W, R.H, dict(job, max_iterations=6), frames)
    for k, v in ref.items():
        if k != "raw":
            assert np.asarray(o[k]).tobytes() == np.asarray(v).tobytes(), k


@pytest.mark.parametrize("n_res", [0, 1, 255, 256, 257])
def test_host_form_residual_counts(built, n_res):
    base, frames = T.scene("scene")
    assert len(base["point"]) >= 257
    job = F.seeded(O.window_job(R.prefix(base, n_res)), 100 + n_res)
    _, exp = assert_host_equals(job, frames, 2, n_res)
    assert len(exp["keep"]) == n_res


@pytest.mark.parametrize("n_pts", [63, 64, 65])
def test_host_form_point_counts(built, n_pts):
    base, frames = T.make_scene(seed=40 + n_pts, n_frames=2, n_pts=n_pts)
    job = F.seeded(O.window_job(base), n_pts)
    _, exp = assert_host_equals(job, frames, 2, n_pts)
    assert len(exp["point_dropped"]) == n_pts


def newest_frame_hosts_nothing():
    """(job, frames): three_frames without the points of the newest frame and their residuals: the newest frame is a target alone"""
    base, frames = T.scene("three_frames")
    n = len(base["frame_ids"])
    hosts = np.asarray(base["host"])
    stay = np.flatnonzero(hosts != n - 1)
    assert 0 < len(stay) < len(hosts)
    new_of = np.full(len(hosts), -1)
    new_of[stay] = np.arange(len(stay))
    job = R.subset(base, np.flatnonzero(new_of[np.asarray(base["point"])] >= 0))
    job["point"] = new_of[np.asarray(job["point"])].astype(np.int32)
    for k in ("host", "u", "v", "color", "weights", "idepth_backup", "idepth_step", "prior", "hdd_lin", "bd_lin", "hcd_lin"):
        if job.get(k) is not None:
            a = np.asarray(job[k])
            job[k] = a.reshape(len(hosts), -1)[stay].reshape((len(stay),) + a.shape[1:]).copy()
    job = F.seeded(O.window_job(job), 77)
    assert (np.asarray(job["host"]) != n - 1).all() and len(job["point"]) > 0
    return job, frames


def test_host_form_newest_frame_hosts_nothing(built):
    job, frames = newest_frame_hosts_nothing()
    assert_host_equals(job, frames, 3, "newest frame hosts nothing")


def test_host_form_optional_outputs_null(built):
    job, frames = F.scene("three_frames")
    _, full = host(job, frames, 3)
    b = S.FinishBatch([dict(job, max_iterations=3)], finish_outputs=())
    b.run_host(R.W, R.H, 0, frames)
    _, got = b.results()[0]
    F.assert_equal(got, full, [k for k in F.ALL_OUT if k != "cam_to_world_out"])
    assert (got["cam_to_world_out"] == S.FILL).all() and (got["J_out"] == S.FILL).all()
    assert not (full["cam_to_world_out"] == S.FILL).any()


def invalid_cases(job):
    m = len(job["host"])
    point = np.asarray(job["point"])
    other = int(np.flatnonzero(point != 0)[0])  # a residual of another point than point 0

    def with_(key, at, value):
        a = np.array(job[key], copy=True)
        a.reshape(-1)[at] = value
        return dict(job, **{key: a})

    bad = [("last_res -2", with_("last_res", 0, -2), {}), ("last_res n_res", with_("last_res", 1, len(point)), {}),
           ("last_res of another point", with_("last_res", 0, other), {}), ("last_state_in 3", with_("last_state_in", 2 * m - 1, 3), {}),
           ("n_good_residuals_in -1", with_("n_good_residuals_in", m - 1, -1), {}), ("max_rel_baseline_in NaN", with_("max_rel_baseline_in", 0, np.nan), {}),
           ("max_rel_baseline_in inf", with_("max_rel_baseline_in", m - 1, np.inf), {}),
           ("max_iterations 21", dict(job, max_iterations=21), {}), ("idepth_step given", dict(job, idepth_step=np.zeros(m, f32)), {}),
           ("state_backup NaN", dict(job, state_backup=np.full_like(np.asarray(job["state_backup"], f64), np.nan)), {})]
    bad += [(f"no {k}", job, dict(omit=(k,))) for k in F.FINISH_IN + tuple(k for k in S.FINISH_OUT if k not in S.FINISH_OPTIONAL)]
    return bad


def test_host_form_refuses_all_or_nothing(built):
    job, frames = F.scene("three_frames")
    good = dict(job, max_iterations=3)
    for what, bad, kw in invalid_cases(good):
        b = S.FinishBatch([bad], **kw)
        before = {k: v.copy() for k, v in b.all_outputs()[0].items()}
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames)
        for k, v in b.all_outputs()[0].items():
            assert v.tobytes() == before[k].tobytes(), (what, k)
    b = S.FinishBatch([good])
    with pytest.raises(DsmError):
        b.run_host(R.W, R.H, 0, frames, optimize_params=OS.default_optimize_params(lambda_init=np.nan))


# ---- independent of the stated order ------------------------------------------------------------------------------------------------

def _matrix(pose):
    x, y, z, w = pose[:4]
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + 2.0 * w * K + 2.0 * K @ K
    M[:3, 3] = pose[4:7]
    return M


def test_adjoint_block_is_the_adjoint_of_the_relative_pose(built):
    """-AH[0:6, 0:6]^T with the rows' scales taken out (powers of two: exact) against Adj(T_t T_h^-1) formed by numpy from 4 x 4 matrices
    in float64.  The bound: an entry of R goes through the quaternion product (7 roundings), the normalisation (9) and quat_to_rot (6) on
    magnitudes of at most 2, the translation through quat_rotate twice (about 30) on magnitudes of at most |t|, and an entry of t^ R adds
    5; numpy's matrices take about as many again.  2 x 64 roundings of 2^-53 on magnitudes of at most 2 max(1, |t|): 256 x 2^-53 x max(1, |t|)."""
    sc = np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0])
    worst = 0.0
    for name in ("scene", "nine_frames", "two_frames"):
        job, frames = F.scene(name)
        _, got = host(job, frames, 2)
        n = len(job["frame_ids"])
        f = n - 1
        ev = got["world_to_cam_eval_out"]
        for h in range(n):
            for t in range(n):
                if h != f and t != f:
                    continue
                L0 = _matrix(ev[t]) @ np.linalg.inv(_matrix(ev[h]))
                Rm, tv = L0[:3, :3], L0[:3, 3]
                That = np.array([[0.0, -tv[2], tv[1]], [tv[2], 0.0, -tv[0]], [-tv[1], tv[0], 0.0]])
                Adj = np.block([[Rm, That @ Rm], [np.zeros((3, 3)), Rm]])
                mine = -(got["ad_host_out"][h, t, :6, :6] / sc[:, None]).T
                bound = 256 * 2.0 ** -53 * max(1.0, float(np.linalg.norm(tv)))
                err = float(np.abs(mine - Adj).max())
                worst = max(worst, err / bound)
                assert err <= bound, (name, h, t, err, bound)
                assert np.array_equal(got["ad_target_out"][h, t, :6, :6], np.diag(sc))
    print(f"\nworst error of an adjoint entry: {worst:.3f} of its bound")


def test_dropping_z1_is_seen(built):
    """at the old evaluation point the newest frame's delta_f is not zero, at the new one it is, in every bit; and the host form is
    told apart from the mutation"""
    job, frames, loop, exp = F.expected("scene")
    n = len(job["frame_ids"])
    assert not exp["delta_x_out"][4 + 8 * (n - 1):].any()
    assert not exp["frames_at"]["delta_f"][n - 1][0] and exp["state_out"][n - 1, :6].tobytes() == np.zeros(6).tobytes()
    old = F.finish(job, frames, loop, keep_old=True)
    assert np.abs(old["delta_x_out"][4 + 8 * (n - 1):][:6]).min() > 0.0
    _, got = host(job, frames, 6)
    with pytest.raises(AssertionError):
        F.assert_equal(got, old, ("delta_x_out",))
    with pytest.raises(AssertionError):
        F.assert_equal(got, old, ("pre_RTll_0_out",))
    F.assert_equal(got, exp, ("delta_x_out", "pre_RTll_0_out"))


# ---- the second keyframe --------------------------------------------------------------------------------------------------------------

def test_host_chain_equals_the_checkers_chain(built):
    """optimize + finish, the finish's outputs to the marginalisation, its prior and the shrunk window to the next optimize + finish:
    the host forms equal the checkers bit for bit at every stage, and the chain is not trivial"""
    from direct_stereo_slam_amd import marginalize as MG

    job, frames = F.scene("scene")
    exp = F.checker_chain("scene")
    got = F.keyframe_chain(job, frames, 6, lambda j, f, its: host(j, f, its), lambda m, f: MG.window_marginalize_host(R.W, R.H, m, f))
    F.assert_equal(got["fin"], exp["fin"])
    assert np.array_equal(got["marg"]["verdict"], exp["marg"]["verdict"]) and got["marg"]["n_res_marg"] == exp["marg"]["n_res_marg"]
    assert got["marg"]["H_M_out"].tobytes() == exp["marg"]["H_M_out"].tobytes() and got["marg"]["b_M_out"].tobytes() == exp["marg"]["b_M_out"].tobytes()
    assert got["loop2"]["pattern"] == exp["loop2"]["pattern"]
    F.assert_equal(got["fin2"], exp["fin2"])
    verdict = exp["marg"]["verdict"]
    assert (verdict == 0).any() and (verdict == 1).any() and exp["marg"]["n_res_marg"] > 0
    assert exp["fin2"]["n_res_out"] > 0 and (np.asarray(exp["two"]["last_res"]) >= 0).any() and len(exp["two"]["frame_ids"]) == len(job["frame_ids"]) - 1
