"""GPU: dsm_window_optimize_batch.

Device against device, byte for byte: the one call equals a host-driven loop of dsm_window_step_batch calls with B1, B2, the decision
and the commits on the host -- the kernels and the inputs are the same, so no tolerance is needed.  Device against the checker
tests/_optimize_ref.py: the same decisions, and the last energy within n_res x 2^-22 x 20000 (tests/test_step_demo.py's bound with its
reasoning: the device's sincos and exp may differ from the C library's in the last place)."""
import numpy as np
import pytest

import _linearize_ref as R
import _optimize_ref as O
import _step_ref as T
from test_step_device import window_of

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
NOT_ARRAYS = ("margins", "committed", "raw", "break_tests")


def run(ctx, cases, op=None, **kw):
    """the cases ((job with max_iterations, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import optimize

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    res = optimize.window_optimize_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)],
                                         optimize_params=optimize.default_optimize_params(**(op or {})), **kw)
    for win in wins:
        win.close()
    return res


def one(ctx, job, frames, max_iterations, op=None):
    return run(ctx, [(dict(O.window_job(job), max_iterations=max_iterations), frames)], op)[0]


def loop_of_step_calls(ctx, job, frames, max_iterations, op=None, stepsizes=None):
    """the parent's route: one dsm_window_step_batch call per pass, B1 and B2 from linearize_job_summary, the loop in Python"""
    from direct_stereo_slam_amd import step

    win = window_of(ctx, job, frames)
    ref = O.run(job, frames, max_iterations, op, stepsizes, pass_fn=lambda j: step.window_step_batch(ctx, [dict(j, window=win)])[0])
    win.close()
    return ref


def assert_same_bytes(got, ref, what=""):
    """every key of ref: every embedded output and every log entry"""
    for k, v in ref.items():
        if k in NOT_ARRAYS:
            continue
        if isinstance(v, (str, int)):
            assert got[k] == v, (what, k, got[k], v)
            continue
        a, b = np.asarray(got[k]), np.asarray(v)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def assert_summary(got):
    """device B1 and B2 against linearize_job_summary's values from the read-back of the same (last) pass, bit for bit"""
    assert f64(got["pass_energy"][-1][0]).tobytes() == f64(got["energy"]).tobytes(), (got["pass_energy"][-1][0], got["energy"])
    assert f32(got["frame_energy_th_out"]).tobytes() == f32(got["new_frame_energy_th"]).tobytes(), (got["frame_energy_th_out"], got["new_frame_energy_th"])
    assert f64(got["pass_energy"][-1][1]).tobytes() == f64(got["energy_m"]).tobytes()


@pytest.mark.parametrize("name", O.SCENES)
def test_one_call_equals_the_loop_of_step_calls_byte_for_byte(ctx, name):
    """all ten scenes; max_iterations 0, 1 and 6; force_accept 0 and 1; fixed_lambda 1e-5"""
    job, frames = T.scene(name)
    for max_iterations, op in [(0, {}), (1, {}), (6, {}), (0, dict(force_accept=1)), (1, dict(force_accept=1)), (6, dict(force_accept=1)),
                               (6, dict(fixed_lambda=1e-5)), (6, dict(min_iterations=0))]:
        got = one(ctx, job, frames, max_iterations, op)
        assert_same_bytes(got, loop_of_step_calls(ctx, job, frames, max_iterations, op), (name, max_iterations, op))
        assert_summary(got)
        if op.get("force_accept"):
            assert got["pattern"] == "A" * got["n_iterations"]


@pytest.mark.parametrize("name", [name for name in O.SCENES if name not in ("one_frame", "three_frames_no_residuals", "no_points")])
def test_device_against_the_checker(ctx, name):
    """scenes with residuals: the checker's decisions and breaks, the last energy within the bound; the scenes without residuals are
    held device against device above"""
    job, frames, exp = O.expected(name)
    got = one(ctx, job, frames, 6)
    n_res = len(job["point"])
    assert n_res > 0
    assert got["pattern"] == exp["pattern"] and list(got["iter_can_break"]) == list(exp["iter_can_break"])
    assert got["n_passes"] == exp["n_passes"] and got["pass_lambda"].tobytes() == exp["pass_lambda"].tobytes()
    bound = n_res * 2.0 ** -22 * 2500.0 * 8
    diff = abs(float(got["last_energy"].sum()) - float(exp["last_energy"].sum()))
    print(f"\n{name}: {got['pattern']}, last energy differs by {diff:.3g} (bound {bound:.3g})")
    assert diff <= bound


@pytest.mark.parametrize("name", ["scene", "two_frames", "nine_frames"])
def test_step_momentum_against_the_checker_from_the_device_step_sizes(ctx, name):
    """the device's exp may differ from the C library's in the last place: the checker starts from the device's own step sizes; the
    device's are within one float ulp of the checker's own"""
    job, frames, own = O.expected(name, step_momentum=1)
    got = one(ctx, job, frames, 6, dict(step_momentum=1))
    sizes = list(got["iter_stepsize"]) + [1.0] * 6
    exp = O.run(job, frames, 6, dict(step_momentum=1), stepsizes=sizes)
    assert got["pattern"] == exp["pattern"] and list(got["iter_can_break"]) == list(exp["iter_can_break"])
    assert got["iter_stepsize"][0] == 1.0
    if got["pattern"] == own["pattern"]:
        assert (np.abs(got["iter_stepsize"].astype(f64) - own["iter_stepsize"].astype(f64)) <= np.spacing(own["iter_stepsize"])).all()
    bound = len(job["point"]) * 2.0 ** -22 * 2500.0 * 8
    assert abs(float(got["last_energy"].sum()) - float(exp["last_energy"].sum())) <= bound
    # and device against device, the host-driven loop taking the device's step sizes
    assert_same_bytes(got, loop_of_step_calls(ctx, job, frames, 6, dict(step_momentum=1), stepsizes=sizes), name)


def test_b1_over_residual_prefixes(ctx):
    """0, 1, 255, 256 and 257 residuals, in one call: the 256-value tile of the ordered sum"""
    job, frames = T.scene("scene")
    assert len(job["point"]) >= 257
    cases = [(dict(O.window_job(R.prefix(job, k)), max_iterations=2), frames) for k in (0, 1, 255, 256, 257)]
    for got, k in zip(run(ctx, cases), (0, 1, 255, 256, 257)):
        assert len(got["new_energy"]) == k
        assert_summary(got)
        acc = 0.0
        for v in got["new_energy"]:
            acc += float(v)
        assert got["pass_energy"][-1][0] == acc
    assert run(ctx, cases[:1])[0]["frame_energy_th_out"] == 1152.0


def eligible(got, job):
    n = len(job["frame_ids"])
    return np.flatnonzero((np.asarray(job["target"]) == n - 1) & (got["new_energy_with_outlier"] >= 0))


def test_b2_counts_against_the_newest_frame(ctx):
    """Values against the newest frame: 0, 1 and 10 (nth = 7 of 10); 255, 256 and 257, the tile of the first sweep, which rides on B1d's
    walk of 256 residuals a trip; 1023, 1024 and 1025, the trip of the later sweeps, which read the compacted list 4 x 256 keys at a
    time; 2049, three trips; and every one the scene has.  Pass 0 linearises every residual at the same state whatever the other
    residuals are, so a first run tells which residuals count."""
    job, frames = T.make_scene(seed=77, n_frames=2, n_pts=8000)
    first = one(ctx, job, frames, 0)
    yes = eligible(first, job)
    no = np.setdiff1d(np.arange(len(job["point"])), yes)
    assert len(yes) > 2049, len(yes)
    counts = (0, 1, 10, 255, 256, 257, 1023, 1024, 1025, 2049, len(yes))
    subs = [R.subset(job, np.sort(np.concatenate([yes[:k], no[:40]]))) for k in counts]
    res = run(ctx, [(dict(O.window_job(s), max_iterations=0), frames) for s in subs]) + [first]
    for got, s, k in zip(res, subs + [job], counts + (len(yes),)):
        vals = np.sort(got["new_energy_with_outlier"][eligible(got, s)])
        assert len(vals) == k
        assert_summary(got)
        if k == 0:
            assert got["frame_energy_th_out"] == 1152.0
            continue
        nth = int(f32(0.7) * f32(k))
        assert k != 10 or nth == 7
        th = f32(np.sqrt(vals[nth]) * f32(1.5))
        th = f32(f32(f32(26.0) * f32(0.5)) + f32(th * f32(0.5)))
        assert got["frame_energy_th_out"] == f32(th * th), k
    # and with iterations, where every pass has its own values
    res = run(ctx, [(dict(O.window_job(s), max_iterations=2), frames) for s in subs[3:]])
    for got in res:
        assert_summary(got)


def test_commit_lanes_at_the_block_edges(ctx):
    """0, 63, 64, 65, 255, 256 and 257 points (two frames) in one call, three iterations: opt_commit_kernel's 256-lane edge"""
    sizes = (0, 63, 64, 65, 255, 256, 257)
    cases = [T.make_scene(seed=40 + m, n_frames=2, n_pts=m) for m in sizes]
    res = run(ctx, [(dict(O.window_job(job), max_iterations=3), frames) for job, frames in cases])
    for got, (job, frames), m in zip(res, cases, sizes):
        assert_same_bytes(got, loop_of_step_calls(ctx, job, frames, 3), m)
        assert got["n_passes"] >= 4


def test_a_prior_is_added_once_per_pass(ctx):
    """stp_frame_kernel adds the prior to the staged H_L and b_L in place: three and more passes on one arena must restore them"""
    job, frames = T.scene("scene")
    assert job.get("state_prior") is not None
    got = one(ctx, job, frames, 6, dict(force_accept=1))
    assert got["n_passes"] == 7
    ref = loop_of_step_calls(ctx, job, frames, 6, dict(force_accept=1))
    assert_same_bytes(got, ref)
    N = 4 + 8 * len(job["frame_ids"])
    H = np.asarray(job["H_L"], f64).reshape(N, N)
    assert np.array_equal(np.diag(got["H_L_step"]), np.diag(H) + np.asarray(job["state_prior"], f64))


MIXED = (("scene", 6), ("one_frame", 6), ("nine_frames", 6), ("three_frames_no_residuals", 6), ("sixteen_frames", 6), ("two_frames", 2), ("no_h_m", 6))


def test_mixed_batch_each_job_equals_itself_alone(ctx):
    """1, 2, 3, 5, 9 and 16 frames, with and without residuals, finishing after 3 to 10 passes: a finished job keeps its last pass
    while the others go on, and does not depend on them"""
    cases = [(dict(O.window_job(T.scene(name)[0]), max_iterations=its), T.scene(name)[1]) for name, its in MIXED]
    together = run(ctx, cases)
    passes = [g["n_passes"] for g in together]
    assert min(passes) == 3 and max(passes) == 10, passes
    for got, case, (name, _) in zip(together, cases, MIXED):
        assert_same_bytes(got, run(ctx, [case])[0], name)
        assert_summary(got)
    # the other order, and twice the same job
    again = run(ctx, cases[::-1] + cases[:1])
    for got, ref in zip(again, together[::-1] + together[:1]):
        assert_same_bytes(got, ref)


def test_two_jobs_on_one_window_and_two_consecutive_calls(ctx):
    from direct_stereo_slam_amd import optimize

    job, frames = T.scene("three_frames")
    win = window_of(ctx, job, frames)
    jobs = [dict(O.window_job(job), window=win, max_iterations=its) for its in (6, 1)]
    a = optimize.window_optimize_batch(ctx, jobs)
    b = optimize.window_optimize_batch(ctx, jobs)
    win.close()
    for got, again, its in zip(a, b, (6, 1)):
        assert_same_bytes(again, got)
        assert_same_bytes(got, one(ctx, job, frames, its))
    assert a[0]["n_iterations"] == 6 and a[1]["n_iterations"] == 1


def test_with_and_without_the_second_group_of_passes(ctx):
    """all accepted: 1 + max_iterations passes finish every job and nothing more is enqueued; one rejection: the second group runs"""
    job, frames = T.scene("two_frames")
    for op, second in ((dict(force_accept=1), False), ({}, True)):
        got = one(ctx, job, frames, 6, op)
        assert (got["n_passes"] > 7) == second, got["pattern"]
        assert_same_bytes(got, loop_of_step_calls(ctx, job, frames, 6, op))


def test_refuses_all_or_nothing(ctx):
    from direct_stereo_slam_amd import optimize
    from direct_stereo_slam_amd._lib import DsmError
    from test_optimize_ref import INVALID_PARAMS, invalid_cases

    job, frames = T.scene("three_frames")
    win = window_of(ctx, job, frames)
    good = dict(O.window_job(job), window=win, max_iterations=3)
    cases = [(what, bad, kw, {}) for what, bad, kw in invalid_cases(good)] + [(str(p), good, {}, p) for p in INVALID_PARAMS]
    for what, bad, kw, op in cases:
        b = optimize.OptimizeBatch([good, bad], **kw)
        before = [{k: v.copy() for k, v in o.items()} for o in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx, optimize_params=optimize.default_optimize_params(**op))
        for o, was in zip(b.all_outputs(), before):
            for k, v in o.items():
                assert v.tobytes() == was[k].tobytes(), (what, k)
    win.close()
