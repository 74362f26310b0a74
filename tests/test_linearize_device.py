"""GPU: dsm_linearize_residuals_batch against the checker tests/_linearize_ref.py -- new_state exactly, every float bit for bit on the rows
L8 defines, the energy as the same double, the threshold bit for bit."""
import numpy as np
import pytest

import _linearize_ref as R

pytestmark = pytest.mark.gpu

OTHER = dict(huber_th=4.0, outlier_th_sum_component=900.0, scale_idepth=2.0, scale_f=30.0, scale_c=20.0, thn=0.45, fac_median=1.2,
             cw=0.3, ow=0.8)


def window_of(ctx, job, frames, w=R.W, h=R.H):
    from direct_stereo_slam_amd import linearize

    win = linearize.KeyframeWindow(ctx, w, h, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


def run(ctx, cases, params=None, w=R.W, h=R.H, **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import linearize

    wins = [window_of(ctx, job, frames, w, h) for job, frames in cases]
    p = linearize.default_params(**params) if params else None
    res = linearize.linearize_residuals_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], p, **kw)
    for win in wins:
        win.close()
    return res


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_checker(ctx, name):
    """5 and 9 frames with fix_linearization, 1, 2 and 3 frames, no points, no residuals"""
    job, frames, exp, _ = R.case(name)
    got = run(ctx, [(job, frames)])[0]
    R.assert_equal(got, exp)
    for k in R.FIELDS_DEFINED:  # L8: the rows of OOB residuals are not written
        assert (got[k][~exp["defined"]] == -7).all(), k
    if len(job["point"]) == 0:  # B4
        assert got["energy"] == 0.0 and got["new_frame_energy_th"] == np.float32(1152.0)


def test_other_parameters_flags_and_outputs(ctx):
    job, frames, _, _ = R.case("scene")
    job = R.prefix(job, 120)
    R.assert_equal(run(ctx, [(job, frames)], OTHER)[0], R.linearize(R.W, R.H, job, frames, OTHER))
    for za, zb in ((1, 0), (0, 1), (1, 1)):
        kw = dict(zero_jab_a=za, zero_jab_b=zb)
        R.assert_equal(run(ctx, [(job, frames)], kw)[0], R.linearize(R.W, R.H, job, frames, kw))
    off = dict(job, fix_linearization=0)
    got = run(ctx, [(off, frames)])[0]
    R.assert_equal(got, R.linearize(R.W, R.H, off, frames))
    assert (got["keep"] == 77).all() and (got["rel_bs"] == -7).all()  # not written without fix_linearization
    base = R.linearize(R.W, R.H, job, frames)
    got = run(ctx, [(job, frames)], outputs=())[0]  # every optional output NULL
    R.assert_equal(got, base, outputs=())
    assert (got["J"] == -7).all() and (got["projected_to"] == -7).all() and (got["keep"] == 77).all()
    got = run(ctx, [(job, frames)], outputs=("projected_to", "rel_bs"))[0]  # ... and some of them
    R.assert_equal(got, base, outputs=("projected_to", "rel_bs"))
    assert (got["J"] == -7).all() and (got["center_projected_to"] == -7).all()


def test_mixed_batch_equals_each_job_alone(ctx):
    """jobs of 5, 1, 9, 3 (no residuals) and 2 frames in one call: every job as the checker has it, and as the job alone; then the
    5-frame job twice on one window, once without fix_linearization"""
    from direct_stereo_slam_amd import linearize

    names = ["scene", "one_frame", "nine_frames", "three_frames_no_residuals", "two_frames"]
    cs = [R.case(n) for n in names]
    together = run(ctx, [(c[0], c[1]) for c in cs])
    for n, c, g in zip(names, cs, together):
        R.assert_equal(g, c[2])
        alone = run(ctx, [(c[0], c[1])])[0]
        for k, v in g.items():
            assert np.asarray(alone[k]).tobytes() == np.asarray(v).tobytes(), (n, k)
    assert len(together[3]["new_state"]) == 0
    job, frames, exp, _ = R.case("scene")
    sub, exp_sub = R.case_prefix("scene", 77, fix=0)
    win = window_of(ctx, job, frames)
    res = linearize.linearize_residuals_batch(ctx, [dict(job, window=win), dict(sub, window=win)])
    win.close()
    R.assert_equal(res[0], exp)
    R.assert_equal(res[1], exp_sub)


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_remainder_sizes(ctx, name):
    """eight residuals per wave, four waves per workgroup: the prefixes around both edges, in one call and each alone"""
    from direct_stereo_slam_amd import linearize

    job, frames, exp, _ = R.case(name)
    sizes = [0, 1, 7, 8, 9, 31, 32, 33, 257]
    # ... and a prefix whose last residual ends OOB in a partly filled wave
    last_oob = next(n for n in range(34, len(exp["new_state"])) if n % 8 and exp["new_state"][n - 1] == R.OOB and exp["new_state"][n - 2] != R.OOB)
    sizes.append(last_oob)
    subs = [R.case_prefix(name, n) for n in sizes]
    win = window_of(ctx, job, frames)
    together = linearize.linearize_residuals_batch(ctx, [dict(s, window=win) for s, _ in subs])
    for n, (s, e), g in zip(sizes, subs, together):
        assert len(g["new_state"]) == n
        R.assert_equal(g, e)
    for n in (1, 9, 33, last_oob):
        s, e = subs[sizes.index(n)]
        R.assert_equal(linearize.linearize_residuals_batch(ctx, [dict(s, window=win)])[0], e)
    win.close()


def test_other_geometry_every_side(ctx):
    """101 x 53 (odd width, a height that is no multiple of anything): residuals leave their targets over each of the four bounds"""
    job, frames, exp = R.geometry_case()
    w, h = R.GEOMETRY
    gone = [R.sides_left(w, h, job, r) for r in range(len(job["point"])) if exp["tags"][r]["exit"] in ("l2_bounds", "l4")]
    for side in R.SIDES:
        assert sum(1 for g in gone if side in g) >= 3, side
    assert (exp["new_state"] == R.IN).sum() >= 20
    R.assert_equal(run(ctx, [(job, frames)], w=w, h=h)[0], exp)


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import linearize
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp, _ = R.case("two_frames")
    win = window_of(ctx, job, frames)
    big = linearize.KeyframeWindow(ctx, 128, 64, 2)
    for fid in job["frame_ids"]:
        big.put_host(int(fid), np.zeros((64, 128), np.float32))
    good = dict(job, window=win)
    calls = [(what, [good, dict(bad, window=win)], kw) for what, bad, kw in R.invalid_jobs(job)]
    calls.append(("a frame id that is not in the window", [good, dict(job, window=win, frame_ids=np.array([200, 555], np.int32))], {}))
    calls.append(("mixed geometries", [good, dict(job, window=big)], {}))
    calls.append(("no window", [good, dict(job, window=None)], {}))
    for what, jobs, kw in calls:
        b = linearize.LinearizeBatch(jobs)
        before = [{k: v.copy() for k, v in out.items()} for out, _ in b.outs]
        with pytest.raises(DsmError):
            b.run(ctx, linearize.default_params(**kw))
        for (out, _), bef in zip(b.outs, before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    for n_frames in (0, 17):
        b = linearize.LinearizeBatch([good, good])
        b.arr[1].n_frames = n_frames
        with pytest.raises(DsmError):
            b.run(ctx)
    b = linearize.LinearizeBatch([good, good])
    b.arr[1].weights = None
    with pytest.raises(DsmError):
        b.run(ctx)
    assert all((out["new_state"] == 77).all() for out, _ in b.outs)
    R.assert_equal(linearize.linearize_residuals_batch(ctx, [good])[0], exp)  # the window and the context are still usable
    win.close(), big.close()
