"""GPU: dsm_window_solve_batch against the checker tests/_solve_ref.py -- x, every point's step, the flags, the optional matrices and
every output of the accumulation bit for bit."""
import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
import _solve_ref as SR

pytestmark = pytest.mark.gpu

HES_OUT = HR.RAW + ("active", "JpJdF") + HR.PER_POINT


def window_of(ctx, job, frames):
    from direct_stereo_slam_amd import solve

    win = solve.KeyframeWindow(ctx, R.W, R.H, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


def run(ctx, cases, params=None, **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import solve

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    res = solve.window_solve_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], params, **kw)
    for win in wins:
        win.close()
    return res


@pytest.mark.parametrize("name", SR.NAMES)
def test_device_equals_checker(ctx, name):
    """5 and 9 frames, 1, 2, 3 and 16 frames, no points, no residuals, the 1e-10 clamp, shift_prior_to_zero on and off"""
    job, frames, exp = SR.case(name)
    got = run(ctx, [(job, frames)])[0]
    SR.assert_equal(got, exp, hes_outputs=HES_OUT)


@pytest.mark.parametrize("nf", [7, 8, 15])
def test_frame_counts_at_the_lane_edges(ctx, nf):
    """N = 60, 68 (the 64-lane edge of the row-per-lane solve; 76 is nine_frames) and 124 (the 128 edge; 132 is sixteen_frames, which
    also takes more than 64 KB of LDS)"""
    job, frames, exp = SR.frames_case(nf)
    assert exp["active"].sum() > 20
    SR.assert_equal(run(ctx, [(job, frames)])[0], exp, hes_outputs=HES_OUT)


def test_solver_edges(ctx):
    """ties, tied groups, an all-zero system, a zero pivot mid-way, a NaN from the scaling, N = 12: one call, and each alone"""
    edges = SR.edge_cases()
    together = run(ctx, [(j, f) for j, f, _ in edges.values()])
    for (name, (job, frames, exp)), got in zip(edges.items(), together):
        SR.assert_equal(got, exp)
        SR.assert_equal(run(ctx, [(job, frames)])[0], exp)
    assert together[list(edges).index("negative_diagonal")]["flags"] == 1


@pytest.mark.parametrize("variant", [dict(lam=lam) for lam in SR.LAMBDAS] + [dict(priors=False), dict(shift=0)] + [dict(n_null=k) for k in (1, 7, 8)],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()))
def test_variants(ctx, variant):
    """every lambda, priors NULL, shift off, n_null 1 / 7 / 8 (0 is every other test)"""
    job, frames, exp = SR.case("scene", **variant)
    SR.assert_equal(run(ctx, [(job, frames)])[0], exp, hes_outputs=HES_OUT)


def test_optional_outputs(ctx):
    """every optional output NULL; then given, where H_A, b_A, H_sc, b_sc are those of dsm_window_hessian_batch on the same job"""
    from direct_stereo_slam_amd import hessian

    job, frames, exp = SR.case("scene")
    got = run(ctx, [(job, frames)], outputs=())[0]
    SR.assert_equal(got, exp, outputs=("x", "step", "flags"))
    assert all((np.asarray(got[k]) == -7).all() for k in HR.STITCHED + ("last_HS", "last_bS") + HR.RAW + HR.PER_POINT)
    got = run(ctx, [(job, frames)], outputs=("H_sc", "last_bS", "hdi", "acc_D"))[0]
    SR.assert_equal(got, exp, outputs=("x", "step", "flags", "H_sc", "last_bS", "hdi", "acc_D"))
    assert (got["H_A"] == -7).all() and (got["last_HS"] == -7).all() and (got["acc_E"] == -7).all() and (got["bd_sum"] == -7).all()
    full = run(ctx, [(job, frames)])[0]
    win = window_of(ctx, job, frames)
    hes = hessian.window_hessian_batch(ctx, [dict(job, window=win)])[0]
    win.close()
    for k in HR.STITCHED + HR.RAW:
        assert full[k].tobytes() == hes[k].tobytes(), k


def test_point_counts_at_the_block_edges(ctx):
    """jobs of 63-65 and 127-129 points (two frames), one call; then a three-frame scene that holds points with 0, 1 and n - 1 = 2
    active residuals (in the larger scenes no point is active against every other frame)"""
    subs = [SR.with_solve(*HR.case_points("wide", m), seed=m) for m in (63, 64, 65, 127, 128, 129)]
    frames = HR.case("wide")[1]
    for got, (_, exp) in zip(run(ctx, [(s, frames) for s, _ in subs]), subs):
        SR.assert_equal(got, exp, hes_outputs=HES_OUT)
    job, frames, exp = SR.frames_case(3)
    per_point = np.bincount(np.asarray(job["point"])[exp["active"].astype(bool)], minlength=len(job["host"]))
    assert len(job["frame_ids"]) == 3 and all((per_point == k).sum() >= 3 for k in (0, 1, 2)), np.bincount(per_point)
    got = run(ctx, [(job, frames)])[0]
    SR.assert_equal(got, exp, hes_outputs=HES_OUT)
    assert all(got["step"][per_point == k].any() == (k > 0) for k in (0, 1, 2))


def test_mixed_batch_equals_each_job_alone(ctx):
    """jobs of 5, 1, 9, 3 (no residuals), 16 and 2 frames in one call: every job as the checker has it, and as the job alone; then two
    jobs on one window"""
    from direct_stereo_slam_amd import solve

    names = ["scene", "one_frame", "nine_frames", "three_frames_no_residuals", "sixteen_frames", "two_frames"]
    cs = [SR.case(n) for n in names]
    together = run(ctx, [(c[0], c[1]) for c in cs])
    for n, c, g in zip(names, cs, together):
        SR.assert_equal(g, c[2], hes_outputs=HES_OUT)
        alone = run(ctx, [(c[0], c[1])])[0]
        for k, v in g.items():
            assert np.asarray(alone[k]).tobytes() == np.asarray(v).tobytes(), (n, k)
    job, frames, exp = SR.case("scene")
    sub, exp_sub = SR.with_solve(*HR.case_prefix("scene", 77, fix=0))
    win = window_of(ctx, job, frames)
    res = solve.window_solve_batch(ctx, [dict(job, window=win), dict(sub, window=win)])
    win.close()
    SR.assert_equal(res[0], exp, hes_outputs=HES_OUT)
    SR.assert_equal(res[1], exp_sub, hes_outputs=HES_OUT)


def test_two_consecutive_runs_are_bit_equal(ctx):
    from direct_stereo_slam_amd import solve

    job, frames, exp = SR.case("nine_frames")
    win = window_of(ctx, job, frames)
    b = solve.SolveBatch([dict(job, window=win), dict(job, window=win)])
    b.run(ctx)
    first = b.results()
    b.run(ctx)
    second = b.results()
    win.close()
    for a, c in zip(first, second):
        SR.assert_equal(a, exp, hes_outputs=HES_OUT)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes() for k in a)
    assert all(np.asarray(first[0][k]).tobytes() == np.asarray(first[1][k]).tobytes() for k in first[0])


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import solve
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = SR.case("scene")
    win = window_of(ctx, job, frames)
    good = dict(job, window=win)
    calls = [(what, [good, dict(bad, window=win)], {}) for what, bad in SR.invalid_jobs(job) + HR.invalid_jobs(job)]
    calls += [(what, [good, dict(bad, window=win)], kw) for what, bad, kw in R.invalid_jobs(job)]
    calls.append(("no window", [good, dict(job, window=None)], {}))
    for what, jobs, kw in calls:
        b = solve.SolveBatch(jobs)
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx, solve.default_params(**kw))
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    for k in ("x", "step", "flags"):
        b = solve.SolveBatch([good, good])
        setattr(b.arr[1], k, None)
        with pytest.raises(DsmError):
            b.run(ctx)
        assert (b.outs[0][0]["x"] == -7).all() and (b.hes.lin.outs[0][0]["new_state"] == 77).all(), k
    SR.assert_equal(solve.window_solve_batch(ctx, [good])[0], exp, hes_outputs=HES_OUT)  # the window and the context are still usable
    win.close()
