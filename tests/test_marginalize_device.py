"""GPU: dsm_window_marginalize_batch against the checker tests/_marginalize_ref.py -- the verdicts, the prior after the points and after
the frames, res_to_zero and every output of the sub-window's linearisation and accumulation bit for bit (C, M1,
X1, A1', M2, G1-G7, Z, V).  The scenes are those of tests/test_marginalize_ref.py, at the geometry of the other window tests; one
case runs at 101 x 53."""
import ctypes as C

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
import _marginalize_ref as MR
import _solve_ref as SR

pytestmark = pytest.mark.gpu


def window_of(ctx, job, frames, w=R.W, h=R.H):
    from direct_stereo_slam_amd import marginalize

    win = marginalize.KeyframeWindow(ctx, w, h, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)
    return win


def run(ctx, cases, marg=None, geometry=(R.W, R.H), **kw):
    """the cases ((job, frames) pairs) as ONE call, each on a window of its own: the result dicts"""
    from direct_stereo_slam_amd import marginalize

    wins = [window_of(ctx, job, frames, *geometry) for job, frames in cases]
    mp = marginalize.default_marg_params(**marg) if marg else None
    res = marginalize.window_marginalize_batch(ctx, [dict(job, window=win) for (job, _), win in zip(cases, wins)], None, mp, **kw)
    for win in wins:
        win.close()
    return res


@pytest.mark.parametrize("name", list(MR.SCENES))
def test_device_equals_checker(ctx, name):
    """5, 9, 2, 1, 3, 4, 16 and 2 frames; a frame leaving at the first, a middle and the last position, two frames in one job, every
    frame, none; no points, no residuals; N = 132 takes more than 64 KB of LDS"""
    job, frames, exp = MR.case(name)
    MR.assert_equal(run(ctx, [(job, frames)])[0], exp)


@pytest.mark.parametrize("nf", [3, 10, 11])
def test_frame_counts_either_side_of_the_lds_switch(ctx, nf):
    """N = 84 and 92: mrg_frame_kernel's LDS is 64 352 and 76 320 bytes; and three frames with residuals (no point of three frames
    has the three residuals the default parameters ask for: LOOSE)"""
    job, frames, exp = MR.frames_case(nf, (nf // 3,), marg=MR.LOOSE)
    assert exp["n_res_marg"] > 0
    MR.assert_equal(run(ctx, [(job, frames)], marg=MR.LOOSE)[0], exp)


@pytest.mark.parametrize("marg_frames", [(), (0,), (2,), (4,), (0, 4), (1, 2), (0, 1, 2, 3, 4)], ids=str)
def test_frames_leaving_at_every_position(ctx, marg_frames):
    job, frames, exp = MR.case("scene", marg_frames=marg_frames)
    MR.assert_equal(run(ctx, [(job, frames)])[0], exp)


def test_no_point_of_verdict_one_and_no_prior(ctx):
    """no point of verdict 1 and no frame leaving: the inputs as values; then H_M / b_M NULL"""
    job, frames, exp = MR.case("two_frames", marg_frames=())
    assert not (exp["verdict"] == MR.MARGINALIZE).any()
    got = run(ctx, [(job, frames)])[0]
    MR.assert_equal(got, exp)
    assert (got["H_M_out"] == job["H_M"]).all() and (got["b_M_out"] == job["b_M"]).all()
    job, frames, exp = MR.case("scene", priors=False)
    MR.assert_equal(run(ctx, [(job, frames)])[0], exp)


def test_sub_window_sizes_at_the_block_edges(ctx):
    """sub-windows of 0, 1, 255, 256 and 257 residuals (mrg_fix_kernel's and hes_residual_kernel's 256) in one call, then of 63, 64
    and 65 points (hes_point_kernel's 64)"""
    for sizes in ([("nine_frames", dict(n_residuals=m)) for m in (0, 1, 255, 256, 257)], [("wide", dict(n_points=m)) for m in (63, 64, 65)]):
        cs = [MR.forced_case(base, **kw) for base, kw in sizes]
        for (base, kw), c in zip(sizes, cs):
            assert len(c[2]["sub_residuals"]) == kw.get("n_residuals", len(c[2]["sub_residuals"])) and len(c[2]["sub_points"]) == kw.get("n_points", len(c[2]["sub_points"]))
        for got, c in zip(run(ctx, [(c[0], c[1]) for c in cs], marg=MR.LOOSE), cs):
            MR.assert_equal(got, c[2])


def test_mixed_batch_equals_each_job_alone_in_two_orders(ctx):
    """jobs of 5, 1, 9, 3 and 16 frames of which 1, 1, 2, 0 and 1 frames leave, in one call and in the reverse order: every job as the
    checker has it and as the job alone; then two jobs on one window"""
    from direct_stereo_slam_amd import marginalize

    names = ["scene", "one_frame", "nine_frames", "three_frames_no_residuals", "sixteen_frames"]
    cs = [MR.case(n) for n in names]
    assert [len(c[0]["marg_frames"]) for c in cs] == [1, 1, 2, 0, 1]
    alone = [run(ctx, [(c[0], c[1])])[0] for c in cs]
    for order in (list(range(5)), list(range(4, -1, -1))):
        together = run(ctx, [(cs[i][0], cs[i][1]) for i in order])
        for i, g in zip(order, together):
            MR.assert_equal(g, cs[i][2])
            for k, v in g.items():
                assert np.asarray(alone[i][k]).tobytes() == np.asarray(v).tobytes(), (names[i], k)
    job, frames, exp = MR.case("scene")
    other, _, exp_other = MR.case("scene", marg_frames=(0, 4))
    win = window_of(ctx, job, frames)
    res = marginalize.window_marginalize_batch(ctx, [dict(job, window=win), dict(other, window=win)])
    win.close()
    MR.assert_equal(res[0], exp)
    MR.assert_equal(res[1], exp_other)


def test_two_consecutive_runs_are_bit_equal(ctx):
    from direct_stereo_slam_amd import marginalize

    job, frames, exp = MR.case("nine_frames")
    win = window_of(ctx, job, frames)
    b = marginalize.MarginalizeBatch([dict(job, window=win), dict(job, window=win)])
    b.run(ctx)
    first = b.results()
    b.run(ctx)
    second = b.results()
    win.close()
    for a, c in zip(first, second):
        MR.assert_equal(a, exp)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes() for k in a)
    assert all(np.asarray(first[0][k]).tobytes() == np.asarray(first[1][k]).tobytes() for k in first[0])


def test_optional_outputs(ctx):
    """res_to_zero and every optional output of hes NULL; then some given"""
    job, frames, exp = MR.case("scene")
    optional = MR.OWN[4:] + HR.STITCHED + HR.RAW + HR.PER_POINT + ("center_projected_to", "projected_to", "JpJdF")
    got = run(ctx, [(job, frames)], outputs=())[0]
    MR.assert_equal(got, exp, outputs=("verdict", "H_M_out", "b_M_out", "n_res_marg", "new_state", "new_energy", "new_energy_with_outlier"))
    assert all((np.asarray(got[k]) == MR.FILL).all() for k in optional) and (got["active"] == 77).all()
    asked = ("res_to_zero", "H_sc", "b_M_points", "hdi", "acc_E", "active")
    got = run(ctx, [(job, frames)], outputs=asked)[0]
    MR.assert_equal(got, exp, outputs=MR.OWN[:4] + asked, fills=tuple(k for k in optional if k not in asked))
    job, frames, exp = MR.case("one_frame")  # every frame leaves and H_M_points is not asked for: the points' prior stays on the device
    MR.assert_equal(run(ctx, [(job, frames)], outputs=())[0], exp, outputs=("verdict", "H_M_out", "b_M_out", "n_res_marg"))


def test_geometry_101_by_53(ctx):
    job, frames, exp = MR.geometry_case()
    assert exp["n_res_marg"] > 20
    MR.assert_equal(run(ctx, [(job, frames)], geometry=R.GEOMETRY)[0], exp)


def test_the_returned_prior_feeds_the_next_keyframe(ctx):
    """the second keyframe: the returned prior as H_M / b_M of dsm_window_solve_batch on the shrunken window equals the checker's chain"""
    from direct_stereo_slam_amd import solve

    job, frames, exp = MR.case("scene")
    got = run(ctx, [(job, frames)])[0]
    nxt, stay = MR.next_keyframe(job, got)
    ref, _ = MR.next_keyframe(job, exp)
    assert len(stay) == 4 and len(nxt["host"]) == (exp["verdict"] == MR.KEEP).sum() and len(nxt["point"]) > 50
    lin = R.linearize(R.W, R.H, ref, [frames[f] for f in stay])
    hes = dict(lin, **HR.hessian(ref, lin, ref))
    want = dict(hes, **SR.solve(ref, hes))
    win = window_of(ctx, nxt, [frames[f] for f in stay])
    res = solve.window_solve_batch(ctx, [dict(nxt, window=win)])[0]
    win.close()
    SR.assert_equal(res, want, hes_outputs=HR.RAW + ("active", "JpJdF") + HR.PER_POINT, lin_outputs=("center_projected_to", "projected_to"))
    assert np.isfinite(res["x"]).all() and np.abs(res["x"]).max() > 0


def test_invalid_calls_are_refused_before_any_output_is_written(ctx):
    from direct_stereo_slam_amd import marginalize
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = MR.case("scene")
    win = window_of(ctx, job, frames)
    good = dict(job, window=win)

    def refused(b, what, lp=None, mp=None):
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run(ctx, lp, mp)
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what

    calls = [(what, bad, {}) for what, bad in MR.invalid_jobs(job) + HR.invalid_jobs(job)] + list(R.invalid_jobs(job))
    for what, bad, kw in calls:
        refused(marginalize.MarginalizeBatch([good, dict(bad, window=win)]), what, marginalize.default_params(**kw))
    refused(marginalize.MarginalizeBatch([good, dict(job, window=None)]), "no window")
    for kw in MR.invalid_params():
        refused(marginalize.MarginalizeBatch([good]), kw, None, marginalize.default_marg_params(**kw))
    for k in ("verdict", "H_M_out", "b_M_out", "n_res_marg"):
        b = marginalize.MarginalizeBatch([good, good])
        setattr(b.arr[1], k, None)
        refused(b, k)
    room = np.zeros((len(job["point"]), 74), np.float32)
    for k, ptr in (("J_out", C.POINTER(C.c_float)), ("keep", C.POINTER(C.c_ubyte)), ("rel_bs", C.POINTER(C.c_float))):
        b = marginalize.MarginalizeBatch([good, good])
        setattr(b.arr[1].hes.lin, k, room.ctypes.data_as(ptr))
        refused(b, k)
    assert not room.any()
    MR.assert_equal(marginalize.window_marginalize_batch(ctx, [good])[0], exp)  # the window and the context are still usable
    win.close()
