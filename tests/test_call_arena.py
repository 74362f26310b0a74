"""GPU: the staging arena the batched calls share (csrc/call_arena.hpp), on a fresh context of its own: calls of different kinds one
after the other, from the smallest arena the suite asks for, through a re-allocation that moves all three regions, to the same calls
again inside the grown buffer, and after a refused call; the template and frame calls that bind all three regions or the work region
alone, between calls that bind none; handles destroyed under a pending hand-over.  Every result is compared as its own test file compares it: against the
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


TW, TH, TNL = 64, 48, 3  # the template and frame calls below: levels of 64 x 48, 32 x 24 and 16 x 12


def _template_case(seed, npts):
    """points, planes and what tests/_template_ref.py makes of them"""
    import _template_ref as R

    rng = np.random.default_rng(seed)
    planes = [rng.uniform(0, 255, (TH >> l, TW >> l)).astype(np.float32) for l in range(TNL)]
    pu, pv = rng.uniform(0, TW - 1, npts).astype(np.float32), rng.uniform(0, TH - 1, npts).astype(np.float32)
    pid, pw = rng.uniform(0.05, 2.0, npts).astype(np.float32), rng.uniform(0.01, 1.0, npts).astype(np.float32)
    return dict(planes=planes, pu=pu, pv=pv, pid=pid, pw=pw, ref=R.make_coarse_depth(TW, TH, TNL, pu, pv, pid, pw, planes))


def test_template_and_frame_calls_share_the_arena(built):
    """dsm_set_refs_from_points (all three regions) and the single-tracker calls that bind the work region alone, on a fresh context:
    as its first call, between trace calls (in / out only), right after a call that moves every region, and right after a refused call."""
    import _template_ref as R
    import _trace_ref as TR
    from _scenes import regrad
    from direct_stereo_slam_amd import synth, trace
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler
    from test_device_loopdet import make_job
    from test_template_edges import _assert_template
    from test_trace_device import Frames

    ctx = Context(0)
    trace_job, trace_target, trace_exp, _ = TR.case("defaults")
    frames = Frames(ctx, [trace_target])  # (no arena call)
    nine = np.arange(152, 161)

    def trace_of_nine_points():  # in and out, no work region
        got = trace.trace_points_batch(ctx, [frames.job(TR.subset(trace_job, nine))])[0]
        TR.assert_equal(got, TR.subset_result(trace_exp, nine))

    K = (0.9 * TW, 0.9 * TW, TW / 2 - 0.5, TH / 2 - 0.5)
    trks = [TrackerAndScaler(ctx, TW, TH, TNL, synth.KITTI_T_STEREO, K) for _ in range(4)]
    cases = [_template_case(11, 700), _template_case(12, 45), _template_case(13, 300)]
    for trk, c in zip(trks, cases):
        trk.upload_intensity(0, c["planes"], 1.0)  # (straight copies: no arena call); trks[3] never gets a frame

    def job(trk, c, frame_id):
        return {"tracker": trk, "ref_frame_id": frame_id, "ref_aff": (0.0, 0.0), "ref_exposure": 1.0, "pu": c["pu"], "pv": c["pv"],
                "pidepth": c["pid"], "pweight": c["pw"]}

    def two_jobs_then_one(what, frame_id):
        ns = TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, [job(trks[0], cases[0], frame_id), job(trks[1], cases[1], frame_id + 1)])
        for j in (0, 1):
            assert trks[j].refFrameID == frame_id + j
            _assert_template(trks[j], ns[j], cases[j]["ref"], f"{what}: job {j} of two")
        trace_of_nine_points()
        ns = TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, [job(trks[2], cases[2], frame_id + 2)])
        assert trks[2].refFrameID == frame_id + 2
        _assert_template(trks[2], ns[0], cases[2]["ref"], f"{what}: one job")
        trace_of_nine_points()

    two_jobs_then_one("the context's first call", 10)  # the arena is allocated by dsm_set_refs_from_points

    # dsm_tracker_set_ref -> dsm_tracker_get_template, bit for bit: a level at capacity, a level of one entry, an empty level
    rng = np.random.default_rng(21)
    lists = [[rng.standard_normal(n).astype(np.float32) for n in (TW * TH, 1, 0)] for _ in range(4)]
    trks[3].setCoarseTrackingRef(5, (0.0, 0.0), 1.0, *lists)
    trace_of_nine_points()
    for l in range(TNL):
        got = trks[3].get_template(l)
        trace_of_nine_points()
        for k in range(4):
            assert got[k].shape == lists[k][l].shape
            np.testing.assert_array_equal(got[k].view(np.uint32), lists[k][l].view(np.uint32), err_msg=f"level {l}, list {k}")

    # dsm_tracker_upload_frame -> dsm_tracker_get_frame at the finest and the coarsest level
    dip = [regrad(d) for d in R.dip(cases[0]["planes"])]
    trks[3].upload_frame(1, dip, 1.0)
    trace_of_nine_points()
    for l in (0, TNL - 1):
        got = trks[3].get_frame(1, l)
        trace_of_nine_points()
        np.testing.assert_array_equal(got.view(np.uint32), dip[l].view(np.uint32), err_msg=f"level {l}")

    _loop_descriptors_equal_host_forms_and_oracle(ctx, make_job(1, n_pts=6000))  # moves all three regions
    two_jobs_then_one("after the re-allocation", 20)

    # refused: the second job's frame slot was never uploaded (DSM_ERR_STATE); nothing is written, the first job's tracker included
    fresh = TrackerAndScaler(ctx, TW, TH, TNL, synth.KITTI_T_STEREO, K)
    with pytest.raises(DsmError, match="dsm error -4"):
        TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, [job(trks[0], cases[2], 30), job(fresh, cases[1], 31)])
    two_jobs_then_one("after a refused call", 40)
    with pytest.raises(DsmError, match="dsm error -4"):
        TrackerAndScaler.setCoarseTrackingRefsFromPoints(ctx, [job(trks[0], cases[2], 50), job(fresh, cases[1], 51)])
    assert trks[0].refFrameID == 40 and fresh.refFrameID == -1
    _assert_template(trks[0], cases[0]["ref"].counts, cases[0]["ref"], "kept through a refused call")

    for t in trks + [fresh]:
        t.close()
    frames.close(), ctx.close()


def _big_tracker(ctx):
    from direct_stereo_slam_amd import synth
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    return TrackerAndScaler(ctx, 1248, 384, 3, synth.KITTI_T_STEREO, (700.0, 700.0, 623.5, 191.5))


def test_tracker_destroyed_under_a_pending_hand_over(built):
    """an asynchronous hand-over to the back buffers is still in flight when its tracker goes, then the context: both wait (drain)"""
    from direct_stereo_slam_amd.tracker import Context

    ctx = Context(0)
    trk = _big_tracker(ctx)
    rng = np.random.default_rng(3)
    images = [rng.uniform(0, 255, (384, 1248)).astype(np.float32) for _ in range(2)]  # pageable: copies on the copy stream
    ctx.upload_images([trk, trk], [2, 3], images, asynchronous=True)
    h, trk.h = trk.h, None
    assert ctx.L.dsm_tracker_destroy(h) == 0
    h, ctx.h = ctx.h, None
    assert ctx.L.dsm_context_destroy(h) == 0
    Context(0).close()  # the device takes the next context


def test_undistorter_destroyed_under_a_pending_hand_over(built):
    from direct_stereo_slam_amd.tracker import Context, Undistorter

    ctx = Context(0)
    trk = _big_tracker(ctx)
    und = Undistorter(ctx, (1248, 384), (1248, 384))  # passthrough
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (384, 1248), dtype=np.uint8) for _ in range(2)]
    ctx.upload_images_undistorted(und, [trk, trk], [2, 3], images, form="async")
    h, und.h = und.h, None
    assert ctx.L.dsm_undistorter_destroy(h) == 0
    trk.close()
    h, ctx.h = ctx.h, None
    assert ctx.L.dsm_context_destroy(h) == 0
    Context(0).close()
