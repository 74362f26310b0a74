"""GPU: dsm_window_hessian_batch against the checker tests/_hessian_ref.py -- the linearisation as its own checker has it, every float
of the per-residual and per-point outputs and every double of the accumulators and of the stitched matrices bit for bit (DESIGN.md
section 17, A0-A3, P1, S1-S3, T1, V)."""
import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R

pytestmark = pytest.mark.gpu


def window_of(ctx, job, frames):
    from direct_stereo_slam_amd import hessian

    win = hessian.KeyframeWindow(ctx, R.W, R.H, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


# what the new kernels walk in pieces: residuals per workgroup of hes_residual_kernel, points per workgroup of hes_point_kernel,
# records of one pair in LDS in hes_pair_kernel, points of one host and points of the job in LDS in hes_schur_kernel
RES_BLOCK, POINT_BLOCK, PAIR_CHUNK, SCHUR_CHUNK, HCC_CHUNK = 256, 64, 16, 32, 128


def run(ctx, cases, params=None, **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import hessian

    wins = [window_of(ctx, job, frames) for job, frames in cases]
    res = hessian.window_hessian_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], params, **kw)
    for win in wins:
        win.close()
    return res


@pytest.mark.parametrize("name", list(HR.CASES) + ["clamp", "wide", "sixteen_frames"])
def test_device_equals_checker(ctx, name):
    """5 and 9 frames, 1, 2, 3 and 16 frames, no points, no residuals, the 1e-10 clamp, shift_prior_to_zero on and off"""
    job, frames, exp = HR.case(name)
    got = run(ctx, [(job, frames)])[0]
    HR.assert_equal(got, exp)
    if len(job["point"]) == 0:
        assert all(not np.asarray(got[k]).any() for k in HR.STITCHED + HR.RAW)


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_without_fix_linearization(ctx, name):
    n = len(HR.case(name)[0]["point"])
    sub, exp = HR.case_prefix(name, n, fix=0)
    got = run(ctx, [(sub, HR.case(name)[1])])[0]
    HR.assert_equal(got, exp)
    assert (got["keep"] == 77).all() and (got["rel_bs"] == -7).all()


def test_optional_outputs_and_rows(ctx):
    """every optional output NULL; lin.J_out given: the rows are those of dsm_linearize_residuals_batch; optional inputs NULL"""
    from direct_stereo_slam_amd import linearize

    job, frames, exp = HR.case("scene")
    got = run(ctx, [(job, frames)], outputs=())[0]
    HR.assert_equal(got, exp, outputs=(), lin_outputs=())
    assert all((np.asarray(got[k]) == (77 if k == "active" else -7)).all() for k in HR.RAW + ("active", "JpJdF") + HR.PER_POINT)
    assert (got["J"] == -7).all() and (got["projected_to"] == -7).all()
    got = run(ctx, [(job, frames)], outputs=("J", "acc_D", "JpJdF", "bd_sum"))[0]
    HR.assert_equal(got, exp, outputs=("acc_D", "JpJdF", "bd_sum"), lin_outputs=("J",))
    win = window_of(ctx, job, frames)
    rows = linearize.linearize_residuals_batch(ctx, [dict(job, window=win)])[0]["J"]
    win.close()
    assert got["J"].tobytes() == rows.tobytes()  # the untouched rows of OOB residuals included
    bare = dict(job, prior=None, delta=None, hdd_lin=None, bd_lin=None, hcd_lin=None)
    HR.assert_equal(run(ctx, [(bare, frames)])[0], dict(exp, **HR.hessian(bare, exp, bare)))


def test_mixed_batch_equals_each_job_alone(ctx):
    """jobs of 5, 1, 9, 3 (no residuals) and 2 frames in one call: every job as the checker has it, and as the job alone; then two
    jobs on one window"""
    from direct_stereo_slam_amd import hessian

    names = ["scene", "one_frame", "nine_frames", "three_frames_no_residuals", "two_frames"]
    cs = [HR.case(n) for n in names]
    together = run(ctx, [(c[0], c[1]) for c in cs])
    for n, c, g in zip(names, cs, together):
        HR.assert_equal(g, c[2])
        alone = run(ctx, [(c[0], c[1])])[0]
        for k, v in g.items():
            assert np.asarray(alone[k]).tobytes() == np.asarray(v).tobytes(), (n, k)
    job, frames, exp = HR.case("scene")
    sub, exp_sub = HR.case_prefix("scene", 77, fix=0)
    win = window_of(ctx, job, frames)
    res = hessian.window_hessian_batch(ctx, [dict(job, window=win), dict(sub, window=win)])
    win.close()
    HR.assert_equal(res[0], exp)
    HR.assert_equal(res[1], exp_sub)


def test_chunk_edges(ctx):
    """residual prefixes at 0, 1 and at the edges of every piece the new kernels walk, each edge - 1, + 0, + 1: the job's residuals
    against RES_BLOCK (scene: 5 frames), the residuals of one pair against 1, 2 and 3 PAIR_CHUNK (wide: 2 frames), and the points
    of the job and of one host against POINT_BLOCK, SCHUR_CHUNK and HCC_CHUNK; all in one call, and some alone"""
    from direct_stereo_slam_amd import hessian

    job, frames, _ = HR.case("scene")
    assert len(job["point"]) > RES_BLOCK + 1
    subs = [HR.case_prefix("scene", n) for n in (0, 1, PAIR_CHUNK - 1, PAIR_CHUNK, PAIR_CHUNK + 1, RES_BLOCK - 1, RES_BLOCK, RES_BLOCK + 1)]
    wide, wide_frames, _ = HR.case("wide")
    in_pair = np.cumsum((np.asarray(wide["host"])[wide["point"]] == 0) & (np.asarray(wide["target"]) == 1))
    hosted = np.cumsum(np.asarray(wide["host"]) == 0)
    wide_subs = []
    for k in (1, 2, 3):
        for edge in (k * PAIR_CHUNK - 1, k * PAIR_CHUNK, k * PAIR_CHUNK + 1):
            wide_subs.append(HR.case_prefix("wide", int(np.flatnonzero(in_pair == edge)[0]) + 1))
    for block in (POINT_BLOCK, HCC_CHUNK):
        wide_subs += [HR.case_points("wide", m) for m in (block - 1, block, block + 1)]
    for chunk in (SCHUR_CHUNK, 2 * SCHUR_CHUNK):
        wide_subs += [HR.case_points("wide", int(np.flatnonzero(hosted == m)[0]) + 1) for m in (chunk - 1, chunk, chunk + 1)]
    win, wide_win = window_of(ctx, job, frames), window_of(ctx, wide, wide_frames)
    jobs = [dict(s, window=win) for s, _ in subs] + [dict(s, window=wide_win) for s, _ in wide_subs]
    for g, (_, e) in zip(hessian.window_hessian_batch(ctx, jobs), subs + wide_subs):
        HR.assert_equal(g, e)
    for j in (1, 4, len(subs) + 2, len(jobs) - 1):
        HR.assert_equal(hessian.window_hessian_batch(ctx, [jobs[j]])[0], (subs + wide_subs)[j][1])
    win.close(), wide_win.close()


def test_two_consecutive_runs_are_bit_equal(ctx):
    from direct_stereo_slam_amd import hessian

    job, frames, exp = HR.case("nine_frames")
    win = window_of(ctx, job, frames)
    b = hessian.HessianBatch([dict(job, window=win), dict(job, window=win)])
    b.run(ctx)
    first = b.results()
    b.run(ctx)
    second = b.results()
    win.close()
    for a, c in zip(first, second):
        HR.assert_equal(a, exp)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes() for k in a)
    assert all(np.asarray(first[0][k]).tobytes() == np.asarray(first[1][k]).tobytes() for k in first[0])


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import hessian
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = HR.case("scene")
    win = window_of(ctx, job, frames)
    good = dict(job, window=win)
    calls = [(what, [good, dict(bad, window=win)], {}) for what, bad in HR.invalid_jobs(job)]
    calls += [(what, [good, dict(bad, window=win)], kw) for what, bad, kw in R.invalid_jobs(job)]
    calls.append(("a frame id that is not in the window", [good, dict(good, frame_ids=np.arange(300, 305, dtype=np.int32))], {}))
    calls.append(("no window", [good, dict(job, window=None)], {}))
    for what, jobs, kw in calls:
        b = hessian.HessianBatch(jobs)
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx, hessian.default_params(**kw))
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    for k in HR.STITCHED:
        b = hessian.HessianBatch([good, good])
        setattr(b.arr[1], k, None)
        with pytest.raises(DsmError):
            b.run(ctx)
        assert (b.outs[0][0]["H_A"] == -7).all() and (b.lin.outs[0][0]["new_state"] == 77).all(), k
    HR.assert_equal(hessian.window_hessian_batch(ctx, [good])[0], exp)  # the window and the context are still usable
    win.close()
