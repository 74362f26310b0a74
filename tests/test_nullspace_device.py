"""GPU: dsm_window_nullspace_batch against the checker tests/_nullspace_ref.py.

With frame_null_in given nothing but + - x / sqrt lies on the device's path, so EVERY output is the checker's bit for bit.  Without it the
device's atan and tan (columns 3-5 of a frame's block) are its own library's: those columns are held to the analytic adjoint within
tests/test_nullspace_ref.py's bound (4 x the constant measured on the checker), columns 0-2 and 6 take the series branches and are the
checker's bit for bit, and everything behind the blocks is compared through the call's own frame_null_out."""
from fractions import Fraction

import numpy as np
import pytest

import _nullspace_ref as NR
import _solve_ref as SR
import _step_ref as T
from test_nullspace_ref import C_POSE, C_SCALE, adjoint_worst
from test_solve_ref import U, gamma

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
CORE = ("null_basis", "null_pinv", "sing", "rank", "flags")


def run(ctx, jobs, **kw):
    from direct_stereo_slam_amd import nullspace

    return nullspace.window_nullspace_batch(ctx, jobs, **kw)


def test_given_blocks_every_output_bit_for_bit(ctx):
    """1, 2, 3, 7, 8, 9, 15 and 16 frames (N = 60 / 68 / 76 around the 64-row edge, 124 / 132 around 128) and the rank-deficient scenes
    in ONE call, with the optional outputs given and NULL"""
    from direct_stereo_slam_amd import nullspace

    jobs = [NR.scene(name) for name in NR.GIVEN_SCENES]
    for got, name in zip(run(ctx, jobs), NR.GIVEN_SCENES):
        NR.assert_equal(got, NR.expected(name))
    for got, name in zip(run(ctx, jobs, outputs=()), NR.GIVEN_SCENES):
        NR.assert_equal(got, NR.expected(name), outputs=CORE)
        assert (got["frame_null"] == nullspace.FILL).all() and (got["null_x0_pre"] == nullspace.FILL).all()
    P = dict(scale_xi_trans=0.25, scale_xi_rot=2.0, scale_a=5.0, scale_b=100.0, solver_mode_delta=1e-3)
    NR.assert_equal(run(ctx, jobs[2:3], params=nullspace.default_nullspace_params(**P))[0], NR.nullspace(jobs[2], P))


def test_from_poses(ctx):
    """columns 0-2 and 6 bit for bit; columns 3-5 against the analytic adjoint; the call's own blocks fed back reproduce the rest"""
    jobs = [NR.scene(name) for name in NR.POSE_SCENES]
    res = run(ctx, jobs)
    worst = [0.0, 0.0]
    for got, job, name in zip(res, jobs, NR.POSE_SCENES):
        exp = NR.expected(name)
        a, b = got["frame_null"].reshape(-1, 6, 7), exp["frame_null"].reshape(-1, 6, 7)
        for col in (0, 1, 2, 6):
            assert NR.bits_equal(a[:, :, col], b[:, :, col]), (name, col)
        worst = [max(x, y) for x, y in zip(worst, adjoint_worst(got, job))]
        assert got["flags"] == exp["flags"] and got["rank"] == exp["rank"], (name, got["flags"], got["rank"])
        NR.assert_equal(got, NR.nullspace(dict(job, frame_null_in=got["frame_null"])))  # the checker behind the device's blocks
    print(f"\nadjoint, in (1 + |t|) 2^-53 / 1e-3: device pose {worst[0]:.3f} (bound {4 * C_POSE}), scale {worst[1]:.3f} (bound {4 * C_SCALE})")
    assert worst[0] <= 4 * C_POSE and worst[1] <= 4 * C_SCALE, worst
    back = run(ctx, [dict(job, frame_null_in=got["frame_null"]) for job, got in zip(jobs, res)])
    for again, got, name in zip(back, res, NR.POSE_SCENES):
        for k in CORE:
            assert np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes(), (name, k)


def test_batches(ctx):
    """a mixed batch of 5, 1, 9, 16 and 2 frames where each job equals itself alone; two jobs on the same poses; two consecutive runs"""
    jobs = [NR.make_job(70 + n, n) for n in (5, 1, 9, 16, 2)]
    jobs.append(jobs[2])
    res = run(ctx, jobs)
    again = run(ctx, jobs)
    for j, (got, job) in enumerate(zip(res, jobs)):
        alone = run(ctx, [job])[0]
        for k in NR.OUT:
            assert np.asarray(got[k]).tobytes() == np.asarray(alone[k]).tobytes() == np.asarray(again[j][k]).tobytes(), (j, k)
    for k in NR.OUT:
        assert np.asarray(res[2][k]).tobytes() == np.asarray(res[5][k]).tobytes(), k


def test_refusals_touch_no_output(ctx):
    from direct_stereo_slam_amd import nullspace
    from direct_stereo_slam_amd._lib import DsmError

    for what, bad, params in NR.invalid_jobs(NR.scene("frames_2")):
        batch = nullspace.NullspaceBatch([NR.scene("frames_3"), bad])
        with pytest.raises(DsmError):
            batch.run(ctx, nullspace.default_nullspace_params(**params) if params else None)
        for out in batch.all_outputs():
            for k, v in out.items():
                assert (v == (77 if k in ("rank", "flags") else nullspace.FILL)).all(), (what, k)


def test_through_the_step_call(ctx):
    """A _step_ref scene whose job carries the basis the new call computes from the job's own world_to_cam_eval: dsm_window_step_batch
    equals _step_ref on the same arrays bit for bit, and null_pinv x after F7, evaluated exactly, stays within section 18 check 3's
    expression with I - null_pinv null_basis in place of I - Q'Q:
      |P x'|_k <= gamma_N (|P||x|)_k + (|I - P Q| |t^|)_k + (|P| (gamma_n |Q||t^| + u (|x| + (1 + gamma_n) |Q||t^|)))_k"""
    from test_step_device import check as step_check
    from test_step_device import run as step_run

    job, frames = T.scene("three_frames")
    expo = np.asarray(job["exposure"], f32)
    null = run(ctx, [dict(world_to_cam_eval=job["world_to_cam_eval"], state_zero=job["state_zero"], exposure=np.where(expo > 0, expo, f32(1.0)))])[0]
    assert null["rank"] == 7 and null["flags"] == 0
    job = dict(job, null_basis=null["null_basis"], null_pinv=null["null_pinv"], n_null=null["n_null"])
    exp = step_check(step_run(ctx, [(job, frames)])[0], job, frames)
    Q, P, x0, x = null["null_basis"], null["null_pinv"], exp["x0"], exp["x"]
    N, nn = Q.shape
    assert x0.tobytes() != x.tobytes()
    F = np.vectorize(Fraction, otypes=[object])
    share = lambda v: np.array([float(abs(s)) for s in F(P).dot(F(v))])  # noqa: E731
    gram = np.array([[float(abs(v)) for v in row] for row in (F(np.eye(nn)) - F(P).dot(F(Q)))])
    at, aQ, aP = np.abs(SR.dsum_rows(P, x0)), np.abs(Q), np.abs(P)
    bound = gamma(N) * (aP @ np.abs(x0)) + gram @ at + aP @ (gamma(nn) * (aQ @ at) + U * (np.abs(x0) + (1 + gamma(nn)) * (aQ @ at)))
    print(f"\n|null_pinv x| after F7 at most {float((share(x) / bound).max()):.3f} of the bound; before F7 at least {float((share(x0) / bound).min()):.3g}")
    assert (share(x) <= bound * (1 + 1e-9)).all(), (share(x), bound)
    assert (share(x0) > 1e3 * bound).all()
