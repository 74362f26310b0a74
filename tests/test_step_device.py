"""GPU: dsm_window_step_batch against the checker tests/_step_ref.py.

The device's sincos (D2) and exp (Q4) are its own library's and may differ from the checker's in the last places; nothing else may.
So world_to_cam is held to tests/test_lm_step.py's bounds for SE3::exp and the product with delta = 4 x 2^-53 (bit for bit for a zero
pose state, which takes the series branch), the float of Q4's factor to one float ulp, and EVERY other output is compared bit for bit
with the checker started from the device's own world_to_cam and factor.  One figure is not recoverable from the outputs: Q4's b entry
is formed from the double of the factor, so the checker forms it from its own exp; a last-place difference of the double would have
to fall on a rounding boundary of the float to show, and a mismatch there would be reported by the bit comparison."""
import math

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
import _solve_ref as SR
import _step_ref as T

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -53
DELTA = 4 * EPS
HES_OUT = HR.RAW + ("active", "JpJdF") + HR.PER_POINT
SOL_OUT = ("x", "step", "flags", "last_HS", "last_bS") + HR.STITCHED


def window_of(ctx, job, frames):
    from direct_stereo_slam_amd import step

    win = step.KeyframeWindow(ctx, R.W, R.H, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


def run(ctx, cases, **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import step

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    res = step.window_step_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], **kw)
    for win in wins:
        win.close()
    return res


def named(got):
    return dict(got, H_L=got["H_L_step"], b_L=got["b_L_step"])


def check(got, job, frames, worst=None):
    got = named(got)
    own = T.step(job)
    n = len(job["frame_ids"])
    for f in range(n):  # D2, as test_lm_step.py bounds SE3::exp and the product
        xi = own["scaled"][f][:6]
        theta, ups = math.sqrt(sum(x * x for x in xi[3:])), math.sqrt(sum(x * x for x in xi[:3]))
        Wd, Wc = got["world_to_cam"][f], own["world_to_cam"][f]
        if theta < 1e-10:
            assert Wd.tobytes() == Wc.tobytes(), f
            continue
        dq, dt = float(np.abs(Wd[:4] - Wc[:4]).max()), float(np.abs(Wd[4:] - Wc[4:]).max())
        t_bound = 8 * DELTA * (1 + 1 / theta) * ups + 8 * EPS * float(np.linalg.norm(Wc[4:]))
        assert dq <= 8 * DELTA and dt <= t_bound, (f, dq / DELTA, dt, t_bound)
        if worst is not None:
            worst["q"], worst["t"] = max(worst["q"], dq / DELTA), max(worst["t"], dt / t_bound if t_bound else 0.0)
    a_dev, a_own = got["pre_aff_mode"][..., 0], own["pre_aff_mode"][..., 0]
    ulp = np.spacing(np.abs(a_own))
    assert (np.abs(a_dev.astype(f64) - a_own.astype(f64)) <= ulp).all()  # Q4: one float ulp
    if worst is not None:
        worst["a"] = max(worst["a"], float((np.abs(a_dev.astype(f64) - a_own.astype(f64)) / ulp).max()) if n > 1 else 0.0)
    exp = T.run(job, frames, W=got["world_to_cam"], aff_a=a_dev)
    T.assert_step_equal(got, exp)
    SR.assert_equal(got, exp, outputs=SOL_OUT, hes_outputs=HES_OUT)
    return exp


@pytest.mark.parametrize("name", ["scene", "nine_frames", "one_frame", "two_frames", "three_frames", "fifteen_frames", "sixteen_frames",
                                  "three_frames_no_residuals", "no_priors", "no_h_m", "zero_step", "lambda_10", "null_2"])
def test_device_equals_checker(ctx, name):
    """the 5- and 9-frame scenes; 1, 2, 3, 15 and 16 frames (225 and 256 pair lanes, N = 124 and 132); no residuals; priors and H_M
    NULL; the zero step; one lambda and one null basis (section 18's tests own that ground); every scene has an exposure of 0"""
    job, frames = T.scene(name)
    worst = dict(q=0.0, t=0.0, a=0.0)
    check(run(ctx, [(job, frames)])[0], job, frames, worst)
    print(f"\n{name}: worst |dq| {worst['q']:.3f} delta (bound 8), |dt| {worst['t']:.3f} of its bound, Q4's factor {worst['a']:.2f} float ulp (bound 1)")


def test_zero_step_world_to_cam_is_bit_equal(ctx):
    """a zero pose state takes the series branch on every frame: no sincos, so the device's poses are the checker's"""
    job, frames = T.scene("two_frames")
    z = np.asarray(job["state_zero"], f64).copy()
    z[:, :6] = 0.0
    job = dict(job, state_backup=z, stepfac=np.zeros(5, f32))
    got = run(ctx, [(job, frames)])[0]
    own = T.step(job)
    assert got["world_to_cam"].tobytes() == own["world_to_cam"].tobytes() and got["cam_to_world"].tobytes() == own["cam_to_world"].tobytes()


def test_point_counts_at_the_block_edges(ctx):
    """0, 63, 64, 65, 255, 256 and 257 points (two frames) in one call: the 256-lane edge of stp_point_kernel and its extra workgroup"""
    cases = [T.make_scene(seed=40 + m, n_frames=2, n_pts=m) for m in (0, 63, 64, 65, 255, 256, 257)]
    for got, (job, frames) in zip(run(ctx, cases), cases):
        check(got, job, frames)


def test_can_break(ctx):
    """can_break 1, and 0 because of each of the four comparisons alone"""
    jobs = T.break_jobs()
    frames = T.scene("two_frames")[1]
    for which, got in zip(jobs, run(ctx, [(j, frames) for j in jobs.values()])):
        exp = check(got, jobs[which], frames)
        assert got["can_break"] == exp["can_break"] == (1 if which == "break" else 0), which


def test_optional_outputs_null(ctx):
    job, frames = T.scene("three_frames")
    full = run(ctx, [(job, frames)])[0]
    got = run(ctx, [(job, frames)], outputs=())[0]
    for k in ("state", "calib", "idepth", "world_to_cam", "can_break", "step_sums", "energy_m", "x", "step", "flags", "energy", "new_frame_energy_th"):
        assert np.asarray(got[k]).tobytes() == np.asarray(full[k]).tobytes(), k
    for k in ("cam_to_world", "cam", "delta_x", "H_L_step", "b_L_step", "H_A", "last_HS") + T.PRE:
        assert (np.asarray(got[k]) == -7).all(), k
    got = run(ctx, [(job, frames)], outputs=("pre_aff_mode", "b_L_step"))[0]
    assert got["pre_aff_mode"].tobytes() == full["pre_aff_mode"].tobytes() and got["b_L_step"].tobytes() == full["b_L_step"].tobytes()
    assert (got["pre_KRKiTll"] == -7).all() and (got["H_L_step"] == -7).all()


def test_mixed_batch_equals_each_job_alone(ctx):
    """jobs of 5, 1, 9, 3 (no residuals), 16 and 2 frames in one call: every job as the checker has it, and as the job alone; then two
    jobs on one window"""
    from direct_stereo_slam_amd import step

    names = ["scene", "one_frame", "nine_frames", "three_frames_no_residuals", "sixteen_frames", "two_frames"]
    cs = [T.scene(n) for n in names]
    together = run(ctx, cs)
    for n, c, g in zip(names, cs, together):
        alone = run(ctx, [c])[0]
        for k, v in g.items():
            assert np.asarray(alone[k]).tobytes() == np.asarray(v).tobytes(), (n, k)
    for n in (0, 2):
        check(together[n], *cs[n])
    job, frames = T.scene("scene")
    other = dict(job, stepfac=np.array([0.5, 0.25, 1.0, 0.0, 0.5], f32))
    win = window_of(ctx, job, frames)
    res = step.window_step_batch(ctx, [dict(job, window=win), dict(other, window=win)])
    win.close()
    for k, v in together[0].items():
        assert np.asarray(res[0][k]).tobytes() == np.asarray(v).tobytes(), k
    check(res[1], other, frames)


def test_two_consecutive_runs_are_bit_equal(ctx):
    from direct_stereo_slam_amd import step

    job, frames = T.scene("nine_frames")
    win = window_of(ctx, job, frames)
    b = step.StepBatch([dict(job, window=win), dict(job, window=win)])
    b.run(ctx)
    first = b.results()
    b.run(ctx)
    second = b.results()
    win.close()
    for a, c in zip(first, second):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes() for k in a)
    assert all(np.asarray(first[0][k]).tobytes() == np.asarray(first[1][k]).tobytes() for k in first[0])


def test_solve_on_the_returned_tables_and_a_reject(ctx):
    """Device against device.  The sol outputs of the step call equal, byte for byte, dsm_window_solve_batch on the job completed with
    the call's own pass-through outputs.  And a reject (all factors 0, lambda x 100) after a step returns the backup state and the
    heads of a first call of the loop (a zero step from the same backup)."""
    from direct_stereo_slam_amd import solve

    job, frames = T.scene("scene")
    got = run(ctx, [(job, frames)])[0]
    cjob = {k: v for k, v in job.items() if k not in T.STEP_IN}
    cjob.update({k: got[k] for k in T.PRE})
    cjob.update(cam=got["cam"][:4], cam_inv=got["cam"][4:], idepth_scaled=got["idepth"] * f32(1.0), idepth_zero_scaled=got["idepth"] * f32(1.0),
                delta=None, delta_x=got["delta_x"], H_L=got["H_L_step"], b_L=got["b_L_step"])
    win = window_of(ctx, job, frames)
    sol = solve.window_solve_batch(ctx, [dict(cjob, window=win)])[0]
    win.close()
    for k, v in sol.items():
        assert np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), k
    zero = np.zeros(5, f32)
    first = run(ctx, [(dict(job, stepfac=zero), frames)])[0]
    reject = run(ctx, [(dict(job, stepfac=zero, **{"lambda": float(job["lambda"]) * 100}), frames)])[0]
    assert reject["state"].tobytes() == np.asarray(job["state_backup"], f64).tobytes()
    assert reject["idepth"].tobytes() == np.asarray(job["idepth_backup"], f32).tobytes()
    for k in ("new_state", "new_energy", "new_energy_with_outlier", "energy", "new_frame_energy_th", "energy_m"):
        assert np.asarray(reject[k]).tobytes() == np.asarray(first[k]).tobytes(), k
    assert reject["x"].tobytes() != first["x"].tobytes()


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import step
    from direct_stereo_slam_amd._lib import DsmError

    job, frames = T.scene("three_frames")
    win = window_of(ctx, job, frames)
    good = dict(job, window=win)
    calls = [(what, [good, dict(bad, window=win)]) for what, bad in T.invalid_jobs(job)]
    calls.append(("no window", [good, dict(job, window=None)]))
    tgt = np.asarray(job["target"]).copy()
    tgt[0] = 3
    calls.append(("target out of range", [good, dict(job, target=tgt, window=win)]))
    for what, jobs in calls:
        b = step.StepBatch(jobs)
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx)
        for out, bef in zip(b.all_outputs(), before):
            assert all(out[k].tobytes() == bef[k].tobytes() for k in out), what
    for kw in (dict(scale_a=np.nan), dict(scale_xi_rot=0.0)):
        with pytest.raises(DsmError):
            step.StepBatch([good]).run(ctx, step_params=step.default_step_params(**kw))
    for k in ("state_out", "can_break", "energy_m"):
        b = step.StepBatch([good, good])
        setattr(b.arr[1], k, None)
        with pytest.raises(DsmError):
            b.run(ctx)
        assert (b.outs[0][0]["state"] == -7).all() and (b.sol.outs[0][0]["x"] == -7).all(), k
    check(step.window_step_batch(ctx, [good])[0], job, frames)  # the window and the context are still usable
    win.close()
