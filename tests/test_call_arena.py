"""GPU: the staging arena the batched calls share (csrc/call_arena.hpp), on a fresh context of its own: calls of different kinds one
after the other, from the smallest arena the suite asks for, through a re-allocation that moves all three regions, to the same calls
again inside the grown buffer, and after a refused call.  Every result is compared as its own test file compares it: against the
independent checker or oracle of that call, never against another run of the library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _loop_descriptors_equal_host_forms_and_oracle(ctx, job, lidar_range=40.0):
    """test_device_loopdet.test_device_pair_equals_host_forms_and_oracle, for one job"""
    from direct_stereo_slam_amd.ringdb import generate_spherical_points, loop_descriptors_batch, scancontext_generate
    from oracle import scancontext as SC

    r = loop_descriptors_batch(ctx, [job], lidar_range)[0]
    keep_h, sel_h, pts_h = generate_spherical_points(job[0], job[1], job[2], lidar_range, job[3], job[4])
    keep_o, sel_o, pts_o = SC.generate_spherical_points(job[0], job[1], job[2], lidar_range, job[3], job[4])
    assert 0 < len(sel_o) < len(job[3])
    np.testing.assert_array_equal(r["kf_keep"], keep_h)
    for sel, pts in ((sel_h, pts_h), (sel_o, pts_o)):
        np.testing.assert_array_equal(r["sel_idx"], sel)
        np.testing.assert_array_equal(r["pts_spherical"], pts)  # bit for bit
    rk_h, si_h, sv_h, tfm_h = scancontext_generate(pts_h, lidar_range)
    rk_o, si_o, sv_o, tfm_o = SC.generate(pts_o, lidar_range)
    for rk, si in ((rk_h, si_h), (rk_o, si_o)):
        np.testing.assert_array_equal(r["ringkey"], rk)
        np.testing.assert_array_equal(r["sig_idx"], si)
    np.testing.assert_array_equal(r["sig_val"], sv_h)
    np.testing.assert_array_equal(r["tfm_pca_rig"], tfm_h)
    np.testing.assert_allclose(r["sig_val"], sv_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["tfm_pca_rig"], tfm_o, atol=1e-9)


def test_calls_of_every_kind_share_one_arena(built):
    import _distmap_ref as DR
    import _icp_ref as IR
    import _immature_ref as MR
    import _trace_ref as TR
    import test_distmap_device as TD
    import test_icp_device as TI
    import test_immature_device as TM
    import test_ringkey_many as TK
    from direct_stereo_slam_amd import icp, synth, trace
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler
    from test_device_loopdet import make_job
    from test_trace_device import Frames

    ctx = Context(0)  # fresh: the session's context has an arena of whatever size the files before this one left it at
    trace_job, trace_target, trace_exp, _ = TR.case("defaults")
    frames = Frames(ctx, [trace_target])
    nine = np.arange(152, 161)
    icp_src, icp_tgt, _ = IR.ties(7)
    imm_job, imm_frames, imm_exp, imm_its = MR.case("scene")
    dm_cases = [DR.case(n) for n in ("small", "no_seeds", "small_b")]

    def trace_of_nine_points():  # no work region; the smallest arena the suite asks for
        got = trace.trace_points_batch(ctx, [frames.job(TR.subset(trace_job, nine))])[0]
        TR.assert_equal(got, TR.subset_result(trace_exp, nine))

    def the_four_small_calls():
        trace_of_nine_points()
        TI.assert_matches_checker(icp.icp(ctx, icp_src, icp_tgt, np.eye(4)), icp_src, icp_tgt, np.eye(4))  # the first work region
        MR.assert_equal(TM.run(ctx, [(imm_job, imm_frames)], gn_iterations=imm_its)[0], imm_exp)
        for c, g in zip(dm_cases, TD.run(ctx, (64, 48), [c[2] for c in dm_cases])):
            TD.check(g, c[3], c[4])

    the_four_small_calls()
    # a work region sized by the voxel grid, far larger than everything before it: the arena is re-allocated, every region moves
    _loop_descriptors_equal_host_forms_and_oracle(ctx, make_job(1, n_pts=6000))
    the_four_small_calls()  # inside a larger buffer that still holds what the descriptors left there

    rng = np.random.default_rng(5)
    seqs = [TK.Seq(ctx, n, margin=3, seed=400 + n) for n in (3, 300)]
    assert TK._drive(ctx, seqs, rng, 12) > 0
    TK._same_indexes(seqs, rng)

    # a refused call (a job that names both a tracker slot and a window frame) writes nothing and leaves the arena usable
    trk = TrackerAndScaler(ctx, TR.W, TR.H, 3, synth.KITTI_T_STEREO, (TR.FX, TR.FY, TR.CX, TR.CY))
    b = trace.TraceBatch([frames.job(TR.subset(trace_job, nine))])
    b.arr[0].target_tracker = trk.h
    before = {k: v.copy() for k, v in b.state[0][0].items()}
    with pytest.raises(DsmError):
        b.run(ctx)
    assert all(np.array_equal(b.state[0][0][k], before[k], equal_nan=k != "status") for k in before)
    assert (b.state[0][0]["steps"] == -1).all()
    trace_of_nine_points()

    for q in seqs:
        q.db.close(), q.twin.close()
    trk.close(), frames.close(), ctx.close()
