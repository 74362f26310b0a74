"""GPU: dsm_window_finish_batch.

Device against device, byte for byte: the embedded optimize job's outputs equal dsm_window_optimize_batch's on the same job, and the
final linearisation equals dsm_linearize_residuals_batch fed with the call's own returned tables, calibration, depths, states and
frame_energy_th -- the kernels and the inputs are the same, so no tolerance applies.  Device against the checker tests/_finish_ref.py
from the device's own read-back: Z1, Z2's rows 0-5, adHTdeltaF and Z5-Z8 bit for bit; what goes through exp or sincos (Z2's affine
entries, Z3's tables) as tests/test_step_device.py compares the same quantities: Q4's factor within one float ulp, then the tables bit
for bit from the device's own factor and poses.  End to end against the checker: every decision and integer equal."""
import numpy as np
import pytest

import _finish_ref as F
import _linearize_ref as R
import _optimize_ref as O
import _step_ref as T
from test_optimize_device import assert_same_bytes
from test_step_device import window_of

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LIN_KEYS = ("new_state", "new_energy", "new_energy_with_outlier", "keep", "rel_bs")


def run(ctx, cases, op=None, w=R.W, h=R.H, **kw):
    """the cases ((job with max_iterations, frames) pairs) as ONE call, each on a window of its own: (loop, finish) pairs"""
    from direct_stereo_slam_amd import finish, optimize, step

    wins = []
    for job, frames in cases:
        win = step.KeyframeWindow(ctx, w, h, len(frames))
        for fid, img in zip(job["frame_ids"], frames):
            win.put_host(int(fid), img)
        wins.append(win)
    res = finish.window_finish_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)],
                                     optimize_params=optimize.default_optimize_params(**(op or {})), **kw)
    for win in wins:
        win.close()
    return res


def optimize_alone(ctx, job, frames, op=None):
    from direct_stereo_slam_amd import optimize

    win = window_of(ctx, job, frames)
    res = optimize.window_optimize_batch(ctx, [dict({k: v for k, v in job.items() if k not in F.FINISH_IN}, window=win)],
                                         optimize_params=optimize.default_optimize_params(**(op or {})))[0]
    win.close()
    return res


def linearize_again(ctx, job, frames, o, got, w=R.W, h=R.H):
    """dsm_linearize_residuals_batch with the fix flag on what the call returned"""
    from direct_stereo_slam_amd import linearize, step

    P = R.PARAMS
    lin = F.final_job(job, dict(o, new_frame_energy_th=o["frame_energy_th_out"]), {k: got[k + "_out"] for k in T.PRE}, list(got["cam_out"]), P)
    win = step.KeyframeWindow(ctx, w, h, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    res = linearize.linearize_residuals_batch(ctx, [dict(lin, window=win)])[0]
    win.close()
    return res


def check(ctx, job, frames, o, got, what="", w=R.W, h=R.H):
    """one job's results against the optimize call, the linearize call and the checker's pieces on the device's own read-back"""
    sp, P = T.SP, R.PARAMS
    n = len(job["frame_ids"])
    f = n - 1
    # Z1, bit for bit
    ev, state, zero = F.new_eval_point(job, o)
    for k, a in (("world_to_cam_eval_out", ev), ("state_out", state), ("state_zero_out", zero)):
        assert got[k].tobytes() == np.array(a, f64).tobytes(), (what, k)
    # D2 at the new point: the newest frame has no pose state (the series branch, no sincos); every other frame's inputs are the last
    # pass's, whose world_to_cam the optimize call returns
    Fr = F.frames_at(ev, state, zero, sp)
    Wd = [[float(x) for x in row] for row in o["world_to_cam"]]
    Wd[f] = Fr["W"][f]
    Fr["W"], Fr["C"] = Wd, [T.se3_inverse(x) for x in Wd]
    assert got["cam_to_world_out"].tobytes() == np.array(Fr["C"], f64).tobytes(), what
    # Z2: rows 0-5 bit for bit; the affine entries from the device's own factor, which is within one float ulp of the checker's
    sa = sp["scale_a"]
    a_dev = np.zeros((n, n), f32)
    expo = np.asarray(job["exposure"], f32)
    for hh in range(n):
        for t in range(n):
            if hh == f or t == f:
                a_dev[hh, t] = f32(got["ad_host_out"][hh, t, 6, 6] / sa)
                own = f32(F.aff_a0(Fr["aff0"][hh], Fr["aff0"][t], expo[hh], expo[t]))
                assert abs(float(a_dev[hh, t]) - float(own)) <= float(np.spacing(own)), (what, hh, t)
    AH, AT = F.adjoints(job, ev, Fr["Ei"], Fr["aff0"], sp, a_of=a_dev)
    assert got["ad_host_out"].tobytes() == AH.tobytes() and got["ad_target_out"].tobytes() == AT.tobytes(), what
    # Z3
    cam, c_delta = F.calibration(job, o, P)
    assert got["cam_out"].tobytes() == np.array(cam, f32).tobytes() and got["c_delta_out"].tobytes() == np.array(c_delta, f32).tobytes(), what
    dx = np.array([float(c) for c in c_delta] + [x for k in range(n) for x in Fr["delta_f"][k]], f64)
    assert got["delta_x_out"].tobytes() == dx.tobytes(), what
    assert got["ad_ht_delta_out"].tobytes() == F.ad_ht_delta(got["ad_host_out"], got["ad_target_out"], Fr["delta_f"]).tobytes(), what
    if n > 1:
        own = F.tables(job, ev, zero, Fr, cam, sp)["pre_aff_mode"][..., 0]
        a_tab = got["pre_aff_mode_out"][..., 0]
        assert (np.abs(a_tab.astype(f64) - own.astype(f64)) <= np.spacing(np.abs(own))).all(), what  # Q4: one float ulp
        pre = F.tables(job, ev, zero, Fr, cam, sp, aff_a=a_tab)
        for k in T.PRE:
            assert got[k + "_out"].tobytes() == pre[k].tobytes(), (what, k)
    # Z4: the same kernel on the same inputs
    if len(job["point"]):
        again = linearize_again(ctx, job, frames, o, got, w, h)
        for k in LIN_KEYS:
            assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), (what, k)
        assert f64(got["energy"]).tobytes() == f64(again["energy"]).tobytes() and f32(got["frame_energy_th_out"]).tobytes() == f32(again["new_frame_energy_th"]).tobytes()
        d = again["new_state"] != F.OOB
        assert got["J_out"][d].tobytes() == again["J"][d].tobytes(), what
    # Z5-Z8 from the device's own final linearisation
    F.assert_equal(got, F.bookkeeping(job, got, got["energy"]), F.BOOK_OUT, what)


def one(ctx, name, max_iterations=6, op=None):
    job, frames = F.scene(name)
    job = dict(job, max_iterations=max_iterations)
    o, got = run(ctx, [(job, frames)], op)[0]
    return job, frames, o, got


@pytest.mark.parametrize("name", ["scene", "nine_frames", "two_frames", "three_frames", "sixteen_frames", "one_frame", "three_frames_no_residuals", "no_points"])
def test_device_against_the_optimize_call_the_linearize_call_and_the_checker(ctx, name):
    job, frames, o, got = one(ctx, name)
    assert_same_bytes(o, optimize_alone(ctx, job, frames), name)
    check(ctx, job, frames, o, got, name)
    # end to end: every decision and integer
    _, _, loop, exp = F.expected(name)
    assert o["pattern"] == loop["pattern"]
    F.assert_equal(got, exp, F.DECISIONS, name)
    if len(job["point"]):
        bound = len(job["point"]) * 2.0 ** -22 * 2500.0 * 8  # section 20's bound on what the device's sincos and exp may move an energy by
        assert abs(float(got["energy"]) - float(exp["energy"])) <= bound


@pytest.mark.parametrize("op", [dict(force_accept=1), {}])
def test_max_iterations_0_and_force_accept(ctx, op):
    for its in (0, 6):
        job, frames, o, got = one(ctx, "three_frames", its, op)
        assert_same_bytes(o, optimize_alone(ctx, job, frames, op), (its, op))
        check(ctx, job, frames, o, got, (its, op))
        assert o["n_passes"] == 1 if its == 0 else (not op or o["n_passes"] == 7)


def test_residual_counts_in_one_call(ctx):
    """0, 1, 255, 256 and 257 residuals: the 256-residual tile of the prefix and of the ordered sum"""
    base, frames = T.scene("scene")
    sizes = (0, 1, 255, 256, 257)
    jobs = [dict(F.seeded(O.window_job(R.prefix(base, k)), 100 + k), max_iterations=2) for k in sizes]
    for (o, got), job, k in zip(run(ctx, [(j, frames) for j in jobs]), jobs, sizes):
        assert len(got["keep"]) == k
        check(ctx, job, frames, o, got, k)
        acc = 0.0
        for v in got["new_energy"]:
            acc += float(v)
        assert got["energy"] == acc
        assert list(got["res_index_out"][got["keep"] == 1]) == list(range(got["n_res_out"]))


def test_point_counts_in_one_call(ctx):
    """63, 64, 65 and 257 points (two frames): the wave and the 256-lane edge of fin_point_kernel and of the prefix over the points"""
    sizes = (63, 64, 65, 257)
    cases = []
    for m in sizes:
        base, frames = T.make_scene(seed=40 + m, n_frames=2, n_pts=m)
        cases.append((dict(F.seeded(O.window_job(base), m), max_iterations=2), frames))
    dropped = 0
    for (o, got), (job, frames), m in zip(run(ctx, cases), cases, sizes):
        assert len(got["point_dropped"]) == m
        check(ctx, job, frames, o, got, m)
        dropped += int(got["point_dropped"].sum())
    assert dropped > 0  # a dropped point


def test_mixed_batch_each_job_equals_itself_alone_in_two_orders(ctx):
    """1, 2, 3, 5, 9 and 16 frames; jobs that reject a step beside jobs that do not (two_frames stops after 2 accepted iterations): a
    finished job's finish does not depend on the passes the others still run"""
    names = (("scene", 6), ("one_frame", 6), ("nine_frames", 6), ("three_frames_no_residuals", 6), ("sixteen_frames", 6), ("two_frames", 2), ("three_frames", 3))
    cases = [(dict(F.scene(name)[0], max_iterations=its), F.scene(name)[1]) for name, its in names]
    together = run(ctx, cases)
    # the loop's outputs against dsm_window_optimize_batch on the SAME batch
    from direct_stereo_slam_amd import optimize

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    alone = optimize.window_optimize_batch(ctx, [dict({k: v for k, v in job.items() if k not in F.FINISH_IN}, window=win) for (job, _), win in zip(cases, wins)])
    for win in wins:
        win.close()
    for (o, _), ref, (name, _) in zip(together, alone, names):
        assert_same_bytes(o, ref, name)
    patterns = [o["pattern"] for o, _ in together]
    assert any("R" in p for p in patterns) and any(p and "R" not in p for p in patterns), patterns
    for (o, got), case, (name, _) in zip(together, cases, names):
        o1, g1 = run(ctx, [case])[0]
        assert_same_bytes(o, o1, name)
        F.assert_equal(got, g1, F.ALL_OUT + ("J_out",), name)
    again = run(ctx, cases[::-1] + cases[:1])
    for (o, got), (o1, g1) in zip(again, together[::-1] + together[:1]):
        assert_same_bytes(o, o1)
        F.assert_equal(got, g1, F.ALL_OUT + ("J_out",))


def test_two_jobs_on_one_window_two_calls_and_optional_outputs_null(ctx):
    from direct_stereo_slam_amd import finish

    job, frames = F.scene("three_frames")
    win = window_of(ctx, job, frames)
    jobs = [dict(job, window=win, max_iterations=its) for its in (6, 1)]
    a = finish.window_finish_batch(ctx, jobs)
    b = finish.window_finish_batch(ctx, jobs)
    lean = finish.window_finish_batch(ctx, jobs, finish_outputs=())
    win.close()
    for (o, got), (o2, got2), (o3, got3), its in zip(a, b, lean, (6, 1)):
        assert_same_bytes(o2, o)
        F.assert_equal(got2, got, F.ALL_OUT + ("J_out",))
        F.assert_equal(got3, got, [k for k in F.ALL_OUT if k != "cam_to_world_out"])
        assert (got3["cam_to_world_out"] == finish.FILL).all() and (got3["J_out"] == finish.FILL).all()
        _, _, o1, g1 = one(ctx, "three_frames", its)
        assert_same_bytes(o, o1)
        F.assert_equal(got, g1, F.ALL_OUT + ("J_out",))


def test_newest_frame_hosts_nothing(ctx):
    from test_finish_ref import newest_frame_hosts_nothing

    job, frames = newest_frame_hosts_nothing()
    job = dict(job, max_iterations=3)
    o, got = run(ctx, [(job, frames)])[0]
    check(ctx, job, frames, o, got)
    loop, exp = F.run(job, frames, 3)
    assert o["pattern"] == loop["pattern"]
    F.assert_equal(got, exp, F.DECISIONS)


def test_another_geometry(ctx):
    """one window at 101 x 53: a step scene's job on planes cut and padded to that size; device against device and the checker's pieces
    (the loop's checker is written for 96 x 64)"""
    from direct_stereo_slam_amd import optimize, step

    w, h = R.GEOMETRY
    base, fr = T.make_scene(seed=11, n_frames=3, n_pts=30)
    planes = []
    for img in fr:
        a = np.asarray(img, f32).reshape(R.H, R.W)
        b = np.zeros((h, w), f32)
        b[:, :R.W] = a[:h]
        b[:, R.W:] = a[:h, -1:]
        planes.append(b)
    job = dict(F.seeded(O.window_job(base), 11), max_iterations=2)
    o, got = run(ctx, [(job, planes)], w=w, h=h)[0]
    win = step.KeyframeWindow(ctx, w, h, len(planes))
    for fid, img in zip(job["frame_ids"], planes):
        win.put_host(int(fid), img)
    alone = optimize.window_optimize_batch(ctx, [dict({k: v for k, v in job.items() if k not in F.FINISH_IN}, window=win)])[0]
    win.close()
    assert_same_bytes(o, alone)
    check(ctx, job, planes, o, got, "101 x 53", w, h)
    assert got["n_res_out"] > 0


def test_refuses_all_or_nothing(ctx):
    from direct_stereo_slam_amd import finish, optimize
    from direct_stereo_slam_amd._lib import DsmError
    from test_finish_ref import invalid_cases

    job, frames = F.scene("three_frames")
    win = window_of(ctx, job, frames)
    good = dict(job, window=win, max_iterations=3)
    for what, bad, kw in invalid_cases(good):
        b = finish.FinishBatch([good, bad], **kw)
        before = [{k: v.copy() for k, v in o.items()} for o in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx)
        for o, was in zip(b.all_outputs(), before):
            for k, v in o.items():
                assert v.tobytes() == was[k].tobytes(), (what, k)
    b = finish.FinishBatch([good])
    with pytest.raises(DsmError):
        b.run(ctx, optimize_params=optimize.default_optimize_params(min_iterations=-1))
    win.close()


def test_the_second_keyframe(ctx):
    """the finish's outputs to dsm_window_marginalize_batch, its prior and the shrunk window to the next finish: verdicts, counts and
    decisions equal the checkers' chain"""
    from direct_stereo_slam_amd import marginalize

    job, frames = F.scene("scene")
    exp = F.checker_chain("scene")

    def finish_fn(j, f, its):
        return run(ctx, [(dict(j, max_iterations=its), f)])[0]

    def marg_fn(m, f):
        win = window_of(ctx, m, f)
        res = marginalize.window_marginalize_batch(ctx, [dict(m, window=win)])[0]
        win.close()
        return res

    got = F.keyframe_chain(job, frames, 6, finish_fn, marg_fn)
    F.assert_equal(got["fin"], exp["fin"], F.DECISIONS)
    assert np.array_equal(got["marg"]["verdict"], exp["marg"]["verdict"]) and got["marg"]["n_res_marg"] == exp["marg"]["n_res_marg"]
    assert got["marg"]["H_M_out"].shape == exp["marg"]["H_M_out"].shape
    assert got["loop2"]["pattern"] == exp["loop2"]["pattern"] and got["loop2"]["n_passes"] == exp["loop2"]["n_passes"]
    F.assert_equal(got["fin2"], exp["fin2"], F.DECISIONS)
    check(ctx, dict(got["two"], max_iterations=6), got["frames2"], got["loop2"], got["fin2"], "second keyframe")
